"""What the cross-model step's tests rest on, checked without a GPU: the set-ups of tests/rnn_cm_mirror.py keep their decision margins (with
dropout off and under the kernels' masks at the pinned seeds), every planted fault of the mirror moves a checked quantity by at least 100 x the
bound the GPU test holds it to, unast_amd.train keeps refusing the cross-model step for model_type='rnn' while the explicit entry points
exist, and the C ABI header, unast_amd.ops and the documents agree on the new entry points."""
import functools
import os
import re

import pytest
import torch

from tests import rnn_cm_mirror as CM
from tests import rnn_step_mirror as SM
from tests.rnn_decoder_mirror import memory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTNS = ("luong", "lsa")
RUN_FLOOR, MARGIN32 = 2e-5, 16.0                      # the GPU test's bounds: 16 x e32, running statistics floored at 2e-5 of their scale


@functools.lru_cache(maxsize=None)
def _sd(attn, case):
    return CM.setup_state_dict(attn, case)


def _gen(attn, case, drops=False, fault=None, dtype=torch.float64):
    cs = CM.CASES[case]
    sd = _sd(attn, case)
    enc, h, c = memory(7, cs["B"], cs["Tk"], cs["lens_k"])
    mt = ms = None
    if drops:
        st, ss = CM.SETUP[attn][case][3]
        d = CM.DROPS
        mt = CM.masks_of(CM.text_sites(cs["B"], cs["max_text"], st, d["t_pre_drop"], d["d_drop"], d["t_post_drop"]))
        ms = CM.masks_of(CM.speech_sites(cs["B"], cs["max_speech"], 0, ss, d["s_pre_drop"], d["d_drop"], 0.0))   # (the post-net's masks decide nothing)
    t = CM.text_generate(SM._sub(sd, "text_m."), attn, enc, h, c, cs["lens_k"], cs["max_text"], mt, fault, dtype, sync_every=4)
    s = CM.speech_generate(SM._sub(sd, "speech_m."), attn, enc, h, c, cs["lens_k"], cs["max_speech"], ms, fault, dtype)
    return t, s


@pytest.mark.parametrize("drops", [False, True])
@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("attn", ATTNS)
def test_setups_keep_their_margins(attn, case, drops):
    t, s = _gen(attn, case, drops)
    cs = CM.CASES[case]
    lt, ls = t["lens"].tolist(), s["lens"].tolist()
    print(attn, case, drops, "text", lt, "gap %.3g" % t["gap"], "speech", ls, "stop margin %.3g" % s["stop_margin"])
    assert t["gap"] >= CM.MARGIN and s["stop_margin"] >= CM.MARGIN and t["live_pad"] == 0
    assert t["tokens"].shape[1] == max(lt) and all(int(t[bn + ".num_batches_tracked"]) == max(lt) for bn in CM.PRE_BN)
    if drops:
        return
    if case == "a":        # lengths differ, everything has stopped before max_len at a position that is no multiple of 4 (the over-run test's SYNC_EVERY)
        assert len(set(lt)) > 1 and max(lt) < cs["max_text"] and max(lt) % 4 and len(set(ls)) > 1 and max(ls) < cs["max_speech"] and max(ls) % 4
    else:                  # one sequence never stops: its length is max_len
        assert cs["max_text"] in lt and min(lt) < cs["max_text"] and cs["max_speech"] in ls and min(ls) < cs["max_speech"]


def _moved(ref, ref32, got, keys, floor=0.0):
    """The largest move of a quantity over the bound tests/test_gpu_rnn_cm.py holds it to: 16 x e32, e32 = the mirror run in fp32 against its fp64
    run on this set-up, floored at the fp32 unit roundoff of the largest value (its _bound), and at `floor` of the scale (its _close)."""
    worst = 0.0
    for k in keys:
        if ref[k].shape != got[k].shape:
            return float("inf")
        scale = ref[k].abs().max().item()
        e32 = max((ref32[k].double() - ref[k]).abs().max().item(), 2.0 ** -24 * scale)
        worst = max(worst, (ref[k] - got[k]).abs().max().item() / max(MARGIN32 * e32, floor * scale))
    return worst


@pytest.mark.parametrize("fault", CM.FAULTS)
@pytest.mark.parametrize("attn", ATTNS)
def test_planted_faults_move_what_the_gpu_test_checks(attn, fault):
    t0, s0 = _gen(attn, "a")
    t32, s32 = _gen(attn, "a", dtype=torch.float32)
    assert torch.equal(t32["tokens"], t0["tokens"]) and s32["lens"].tolist() == s0["lens"].tolist(), "the fp32 mirror must decide as the fp64 one"
    t1, s1 = _gen(attn, "a", fault=fault)
    stats = [bn + "." + n for bn in CM.PRE_BN for n in ("running_mean", "running_var")]
    exact = (not torch.equal(t0["tokens"], t1["tokens"]) if t0["tokens"].shape == t1["tokens"].shape else True) or t0["lens"].tolist() != t1["lens"].tolist() or \
        s0["lens"].tolist() != s1["lens"].tolist() or any(t0[bn + ".num_batches_tracked"] != t1[bn + ".num_batches_tracked"] for bn in CM.PRE_BN)
    moved = max(_moved(t0, t32, t1, stats, RUN_FLOOR), _moved(s0, s32, s1, ["pre", "post", "stop"]),
                _moved(s0, s32, s1, [bn + "." + n for bn in CM.POST_BN for n in ("running_mean", "running_var")], RUN_FLOOR))
    print("%s %-18s exact quantities differ: %s; largest move %.3g x its bound" % (attn, fault, exact, moved))
    assert moved >= 100.0, (fault, moved)


@pytest.mark.parametrize("attn", ATTNS)
def test_substep_generations_keep_their_margins_under_dropout(attn):
    """The dropout-on sub-step test of tests/test_gpu_rnn_cm.py: after set_seed(SETUP[attn]['cm'][3]) train_cm_step's two generations, under the masks
    of the sites predicted on the host, keep MARGIN in fp64, decide the same in fp32, and generate lengths that differ; and the whole sub-step of
    the mirror in fp32, under all eight tapes' masks, meets every gradient bound against its fp64 run (a set-up whose own fp32 run misses a bound
    cannot measure the kernels; measured 0.15 (luong) and 0.31 .. 0.45 (lsa, by the host's fp32 sums) of the bound)."""
    from tests import rnn_step_fixture as SF
    text, mel, tl, ml = CM.setup_batch()
    cs, seed = CM.CM_BATCH, CM.SETUP[attn]["cm"][3]
    masks = {k: CM.masks_of(v) for k, v in CM.cm_sites(seed).items()}
    assert sorted(masks) == ["gen_speech", "gen_text", "speech_mem", "text_mem"] and all(len(m) >= 2 for m in masks.values())
    res = []
    for dt in (torch.float64, torch.float32):
        mir = SM.Mirror(dict(_sd(attn, "cm")), attn, SF.args_of(attn, 0.0, **CM.DROPS), dtype=dt)
        res.append(CM.cm_step(mir, text, tl, mel, ml, 3, cs["max_text"], cs["max_speech"], masks, generations_only=True))
    (gt, gs), (gt32, gs32) = res
    print(attn, "text", gt["lens"].tolist(), "gap %.3g" % gt["gap"], "speech", gs["lens"].tolist(), "stop margin %.3g" % gs["stop_margin"])
    assert gt["gap"] >= CM.MARGIN and gs["stop_margin"] >= CM.MARGIN and gt["live_pad"] == 0
    assert torch.equal(gt32["tokens"], gt["tokens"]) and gs32["lens"].tolist() == gs["lens"].tolist()
    lt, ls = gt["lens"].tolist(), gs["lens"].tolist()
    assert len(set(lt)) > 1 and len(set(ls)) > 1
    masks = {k: CM.masks_of(v) for k, v in CM.cm_sites(seed, lt, ls).items()}
    assert sorted(masks) == sorted(CM.GEN_TAPES)
    mirs = []
    for dt in (torch.float64, torch.float32):
        mirs.append(SM.Mirror(dict(_sd(attn, "cm")), attn, SF.args_of(attn, 0.0, **CM.DROPS), dtype=dt))
        g = CM.cm_step(mirs[-1], text, tl, mel, ml, 3, cs["max_text"], cs["max_speech"], masks)
        assert g[0]["lens"].tolist() == lt and g[1]["lens"].tolist() == ls
    e32 = {k: SF.rel(mirs[1].grads[k].double().numpy(), g64.numpy()) for k, g64 in mirs[0].grads.items()}
    bounds, _ = SF.grad_bounds(e32, "a")
    worst = max(bounds, key=lambda k: e32[k] / bounds[k])
    print(attn, "the fp32 mirror's worst gradient: %.3g = %.3f of its bound (%s)" % (e32[worst], e32[worst] / bounds[worst], worst))
    assert e32[worst] <= bounds[worst]


def test_the_mirror_draws_the_substeps_seeds_as_next_seed_does():
    from unast_amd import utils
    saved = dict(utils._RNG)
    try:
        for seed in (0, 2, 26, 20241):
            utils._RNG["seed"], utils._RNG["counter"] = seed, 0
            assert [utils.next_seed() for _ in CM.GEN_TAPES] == [CM.cm_seeds(seed)[k] for k in CM.GEN_TAPES]
    finally:
        utils._RNG.update(saved)


def test_train_keeps_refusing_and_the_entry_points_exist():
    from unast_amd import train, train_rnn, train_rnn_step
    from tests.test_cpu_rnn_step import _config_args
    args = _config_args("rnn_d_lsa")
    assert args.cm_steps > 0
    for call in (lambda: train.train(args), lambda: train.train_cm_step({}, None, None, 0, 1, args),
                 lambda: train.train_step({}, None, None, None, {}, 0, args)):
        with pytest.raises(NotImplementedError, match="generate in train mode") as e:
            call()
        assert "train_rnn_step.train_cm_step" in str(e.value) and "train_rnn_step.train_step" in str(e.value)
    for mod, names in ((train_rnn, ("text_generate_train", "speech_generate_train", "SYNC_EVERY")), (train_rnn_step, ("train_cm_step", "train_step"))):
        for n in names:
            assert hasattr(mod, n), n
    assert (train_rnn.S_GEMB, train_rnn.S_SGPOST + 3) == (21, 34), "the generation's mask sites continue after 20, one id per site"
    assert train_rnn.prefix_row0(3, 1) == 0 and train_rnn.prefix_row0(3, 4) == 3 * (1 + 2 + 3) == CM.prefix_row0(3, 4)


def test_header_ops_and_documents_agree():
    from unast_amd import ops
    from unast_amd._lib import parse_header
    protos = parse_header()
    want = {"unast_prefix_gen_tiles": 2, "unast_prefix_gen_conv": 22, "unast_prefix_gen_finish": 27, "unast_prefix_gen_act_drop": 14,
            "unast_prefix_gen_end_text": 12, "unast_prefix_gen_end_speech": 13}
    assert {k: len(protos[k][1]) for k in want} == want
    for k in want:
        assert hasattr(ops, k[len("unast_"):]), k
    n = len(protos)
    for doc, pat in (("README.md", r"the C ABI \((\d+) entry points\)"), ("INTEGRATION.md", r"for every entry point \((\d+)\)")):
        m = re.search(pat, open(os.path.join(ROOT, doc)).read())
        assert m and int(m.group(1)) == n, (doc, m and m.group(1), n)
    src = open(os.path.join(ROOT, "unast_amd", "csrc", "prefix_gen.hip")).read()
    for k in want:
        assert 'extern "C" int %s(' % k in src, k
    assert "atomic" not in src.replace("no atomics", "").replace("No atomics", "") and "cooperative" not in src.lower()


# ---- the mirror against the reference's fixtures (tests/golden/rnn_cm_{luong,lsa}.npz) ------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "b", "a_eps"])
@pytest.mark.parametrize("attn", ATTNS)
def test_mirror_reproduces_the_reference_fixtures(attn, case):
    """rnn_cm_mirror.cm_step on a rnn_step_mirror.Mirror against the reference's own fp64 run: tokens, lengths, num_batches_tracked and key sets
    exactly; everything else far below any GPU bound (the agreement reached is printed)."""
    import json
    import numpy as np
    from tests import rnn_cm_fixture as CF
    from tests import rnn_step_fixture as SF
    fx, m = CF.fixture(attn), CF.meta(attn)
    cfx = CM.CM_FIXTURE[attn]["a" if case == "a_eps" else case]
    assert m["setups"] == json.loads(json.dumps(CM.CM_FIXTURE[attn])), "the fixture was generated from other set-ups"
    sd = CM.fixture_state_dict(attn, case)
    text, mel, tl, ml = CM.fixture_batch(cfx)
    mir = SM.Mirror(sd, attn, SF.args_of(attn, 0.0), eps_text=m["eps_cond"] if case == "a_eps" else 1e-5)
    gt, gs = CM.cm_step(mir, text, tl, mel, ml, 1, cfx["max_text"], cfx["max_speech"])
    assert gt["lens"].tolist() == fx[case + "/gen/text_lens"].tolist() and gs["lens"].tolist() == fx[case + "/gen/speech_lens"].tolist()
    assert torch.equal(gt["tokens"], torch.from_numpy(fx[case + "/gen/tokens"])) and gt["live_pad"] == 0
    gap, margin = fx[case + "/margins"].tolist()
    assert abs(gt["gap"] - gap) <= 1e-9 and abs(gs["stop_margin"] - margin) <= 1e-9 and min(gap, margin) >= CM.MARGIN
    worst = {}
    worst["frames"] = max(np.abs(gs[k].numpy() - fx["%s/gen/%s" % (case, k)]).max() for k in ("pre", "post", "stop"))
    worst["losses"] = max(abs(mir.losses[k][0] - float(fx["%s/loss/%s" % (case, k)])) / max(1.0, abs(float(fx["%s/loss/%s" % (case, k)]))) for k in CF.LOSS_KEYS)
    print({k: "%.3e" % (mir.losses[k][0] - float(fx["%s/loss/%s" % (case, k)])) for k in CF.LOSS_KEYS})
    ref, gnorm, e32 = CF.grads(attn, case)
    assert sorted(mir.grads) == sorted(ref), sorted(set(mir.grads) ^ set(ref))
    worst["grads"] = max(SF.rel(SF.sample(mir.grads[k].numpy(), m["g_sample"]), ref[k]) for k in ref if k not in SF.DEGENERATE)
    run, _ = CF.running(attn, case)
    worst["running"] = max(np.abs(SF.sample(mir.sd[k].numpy(), m["p_sample"]) - v).max() for k, v in run.items())
    nbt = json.loads(str(fx[case + "/num_batches_tracked"]))
    assert {k: int(mir.sd[k]) for k in nbt} == nbt
    norm = mir.optimizer_step(m["lr"], m["weight_decay"], m["grad_clip"], True)
    worst["norm"] = abs(norm - float(fx[case + "/norm"])) / norm
    state = SF.group(fx, case + "/state")
    worst["post-step state"] = max(np.abs(SF.sample(mir.sd[k].numpy(), m["p_sample"]) - v).max() for k, v in state.items())
    print(attn, case, {k: "%.2e" % v for k, v in worst.items()})
    assert worst["frames"] <= 1e-9 and worst["losses"] <= 1e-6 and worst["grads"] <= 1e-6 and worst["running"] <= 1e-9 and worst["norm"] <= 1e-7
    assert worst["post-step state"] <= 1e-7
