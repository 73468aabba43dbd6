"""Train-mode generation (unast_amd.train_rnn.text_generate_train / speech_generate_train) and the cross-model sub-step and step
(unast_amd.train_rnn_step.train_cm_step / train_step) on the GPU, against the fp64 mirror of tests/rnn_cm_mirror.py under the kernels' own masks.

The set-ups (seeded portable weights with 5h's trajectory gains, a random memory, dropout seeds) are tests/rnn_cm_mirror.SETUP: chosen on the CPU
so that every greedy decision of the mirror has a margin of MARGIN (tests/test_cpu_rnn_cm.py pins that); each test asserts the margins again
before it compares.  Case a: B = 3, lengths that differ, one EOS at position 1, every sequence stopped at a position that is no multiple of 4;
case b: B = 2 with max_len small enough that one sequence never stops.
Bounds: tokens, lengths and num_batches_tracked exactly; frames, stop logits 16 x e32 (e32 = the mirror run in fp32 against its fp64 run, as
tests/test_gpu_text_prefix_kernels.py takes it, floored at the fp32 unit roundoff of the largest value); running statistics max(2e-5, 16 x e32)
of their scale; losses 1e-3 x max(1, |ref|); gradients by tests/rnn_step_fixture.grad_bounds on the mirror's own e32 (decoder side
min(1e-3, 16 x max(common, own e32)), encoder side 1e-3, the three ill-conditioned text-prenet tensors max(1e-3, 16 x their own e32); the
degenerate conv biases in front of a BatchNorm have no bound there)."""
from collections import defaultdict
import functools

import numpy as np
import pytest
import torch

from tests import rnn_cm_fixture as CF
from tests import rnn_cm_mirror as CM
from tests import rnn_step_fixture as SF
from tests import rnn_step_mirror as SM
from tests.rnn_decoder_mirror import memory

pytestmark = pytest.mark.gpu
ATTNS = ("luong", "lsa")
MARGIN32 = 16.0


def _dev():
    return torch.device("cuda:0")


def _build(attn, case, drops, **over):
    from unast_amd import train
    args = SF.args_of(attn, 0.0, **(dict(CM.DROPS, **over) if drops else over))
    saved = train.DEVICE
    train.DEVICE = _dev()
    try:
        _, _, model, opt, sched = train.initialize_model(args)
    finally:
        train.DEVICE = saved
    sd = CM.setup_state_dict(attn, case)
    assert list(model.state_dict()) == list(sd)
    model.load_state_dict(sd)
    _zero_epoch()
    return model.train(), opt, args, sd


def _zero_epoch():
    """The device's RNG epoch is 0 outside graph replay, but a captured train step of an earlier test may have left its step number there: the
    generation seeds of rnn_cm_mirror.SETUP were chosen for epoch 0."""
    from unast_amd import ops
    ops.rng_epoch_counter().zero_()


@functools.lru_cache(maxsize=None)
def _memory(case):
    cs = CM.CASES[case]
    return memory(7, cs["B"], cs["Tk"], cs["lens_k"])


def _bound(ref64, ref32):
    e32 = max((ref32.double() - ref64).abs().max().item(), 2.0 ** -24 * ref64.abs().max().item())
    return MARGIN32 * e32, e32


def _close(name, got, ref64, ref32, floor=0.0):
    b, e32 = _bound(ref64, ref32)
    b = max(b, floor * ref64.abs().max().item())
    err = (got.detach().cpu().double() - ref64).abs().max().item()
    print("%-44s err %.3g, e32 %.3g, %.2f of its bound" % (name, err, e32, err / b))
    assert err <= b, (name, err, b)


def _generate(model, attn, case, seed_t, seed_s):
    from unast_amd import train_rnn as TR
    cs, dev = CM.CASES[case], _dev()
    enc, h, c = (torch.from_numpy(x).to(dev) for x in _memory(case))
    gt = TR.text_generate_train(model.text_m, ((h, c), enc), cs["lens_k"], max_len=cs["max_text"], seed=seed_t)
    gs = TR.speech_generate_train(model.speech_m, ((h, c), enc), cs["lens_k"], max_len=cs["max_speech"], seed=seed_s)
    torch.cuda.synchronize()
    return gt, gs


@pytest.mark.parametrize("drops", [False, True])
@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("attn", ATTNS)
def test_generation_against_the_mirror(attn, case, drops):
    model, opt, args, sd = _build(attn, case, drops)
    cs = CM.CASES[case]
    seed_t, seed_s = CM.SETUP[attn][case][3] if drops else (0, 0)
    nbt0 = int(model.text_m.prenet.batch_norm1.num_batches_tracked)
    gt, gs = _generate(model, attn, case, seed_t, seed_s)
    enc, h, c = _memory(case)
    # the kernels list exactly the sites the mirror's helper predicts (and none with dropout off)
    from unast_amd import ops
    CM._EPOCH[0] = int(ops.rng_epoch_counter())                                                  # (an earlier captured step may have left its step number there)
    try:
        want_t = CM.text_sites(cs["B"], cs["max_text"], seed_t, args.t_pre_drop, args.d_drop, args.t_post_drop)
        want_s = CM.speech_sites(cs["B"], cs["max_speech"], gs[0].shape[1], seed_s, args.s_pre_drop, args.d_drop, args.s_post_drop)
    finally:
        CM._EPOCH[0] = 0
    assert CM.plain(gt.sites) == CM.plain(want_t) and CM.plain(gs.sites) == CM.plain(want_s)
    tsd, ssd = SM._sub(sd, "text_m."), SM._sub(sd, "speech_m.")
    ref = {}
    for dt, tag in ((torch.float64, 64), (torch.float32, 32)):
        ref["t%d" % tag] = CM.text_generate(tsd, attn, enc, h, c, cs["lens_k"], cs["max_text"], CM.masks_of(gt.sites), dtype=dt)
        ref["s%d" % tag] = CM.speech_generate(ssd, attn, enc, h, c, cs["lens_k"], cs["max_speech"], CM.masks_of(gs.sites), dtype=dt)
    t64, s64, t32, s32 = ref["t64"], ref["s64"], ref["t32"], ref["s32"]
    print("mirror: text lens %s gap %.3g live PAD %d; speech lens %s stop margin %.3g" % (t64["lens"].tolist(), t64["gap"], t64["live_pad"], s64["lens"].tolist(),
                                                                                       s64["stop_margin"]))
    assert t64["gap"] >= CM.MARGIN and s64["stop_margin"] >= CM.MARGIN and t64["live_pad"] == 0, "the set-up lost its decision margins"
    assert torch.equal(t32["tokens"], t64["tokens"]) and torch.equal(s32["lens"], s64["lens"]), "the fp32 mirror must decide as the fp64 one"
    # ---- text
    assert gt.lens_host == t64["lens"].tolist() and gt[1].tolist() == gt.lens_host
    assert torch.equal(gt[0].cpu(), t64["tokens"]) and gt.live_pad == 0
    T = max(gt.lens_host)
    for k in range(3):
        bn, name = getattr(model.text_m.prenet, "batch_norm%d" % (k + 1)), CM.PRE_BN[k]
        assert int(bn.num_batches_tracked) == nbt0 + T == t64[name + ".num_batches_tracked"]
        _close(name + ".running_mean", bn.running_mean, t64[name + ".running_mean"], t32[name + ".running_mean"], 2e-5)
        _close(name + ".running_var", bn.running_var, t64[name + ".running_var"], t32[name + ".running_var"], 2e-5)
    # ---- speech
    assert gs.lens_host == s64["lens"].tolist()
    for i, k in enumerate(("pre", "post", "stop")):
        assert gs[i].shape == s64[k].shape
        _close("speech " + k, gs[i], s64[k], s32[k])
    for k, name in enumerate(CM.POST_BN):
        bn = model.speech_m.postnet.pre_batchnorm if k == 0 else model.speech_m.postnet.batch_norm_list[k - 1]
        assert int(bn.num_batches_tracked) == 1
        _close(name + ".running_mean", bn.running_mean, s64[name + ".running_mean"], s32[name + ".running_mean"], 2e-5)
        _close(name + ".running_var", bn.running_var, s64[name + ".running_var"], s32[name + ".running_var"], 2e-5)
    if drops:
        return                                                                                   # (the lengths' shape below is the dropout-off set-up's)
    if case == "b":
        assert cs["max_text"] in gt.lens_host and min(gt.lens_host) < cs["max_text"], "one sequence never stops: its length is max_len"
        assert cs["max_speech"] in gs.lens_host and min(gs.lens_host) < cs["max_speech"]
        assert gt.steps == cs["max_text"] and gs.steps == cs["max_speech"]
    else:
        assert len(set(gt.lens_host)) > 1 and max(gt.lens_host) < cs["max_text"] and len(set(gs.lens_host)) > 1
        # zero past each sequence's length
        for b, n in enumerate(gs.lens_host):
            assert gs[1][b, n:].abs().max().item() == 0.0 if n < gs[1].shape[1] else True


@pytest.mark.parametrize("attn", ATTNS)
def test_positions_after_the_exit_change_nothing(attn, monkeypatch):
    """Case a stops at a position that is no multiple of 4: with SYNC_EVERY = 4 the host launches positions after every sequence has stopped.
    Tokens, frames, lengths, running statistics and num_batches_tracked must equal the run that checks every position, to the bit."""
    from unast_amd import train_rnn as TR
    res = {}
    for every in (1, 4):
        monkeypatch.setattr(TR, "SYNC_EVERY", every)
        model, opt, args, sd = _build(attn, "a", False)
        gt, gs = _generate(model, attn, "a", 0, 0)
        state = {k: v.clone() for k, v in model.state_dict().items() if "batch_norm" in k or "batchnorm" in k}
        res[every] = (gt, gs, state)
    (gt1, gs1, st1), (gt4, gs4, st4) = res[1], res[4]
    assert gt1.steps == max(gt1.lens_host) and gs1.steps == max(gs1.lens_host)
    assert gt4.steps > gt1.steps and gs4.steps > gs1.steps and gt4.steps % 4 == 0 and gs4.steps % 4 == 0, (gt4.steps, gs4.steps)
    assert all(torch.equal(a, b) for a, b in zip(gt1, gt4)) and all(torch.equal(a, b) for a, b in zip(gs1, gs4))
    assert sorted(st1) == sorted(st4) and all(torch.equal(st1[k], st4[k]) for k in st1), [k for k in st1 if not torch.equal(st1[k], st4[k])]


@pytest.mark.parametrize("attn", ATTNS)
def test_two_runs_agree_to_the_bit_and_a_seed_changes_the_masks(attn):
    seed_t, seed_s = CM.SETUP[attn]["a"][3]
    runs = []
    for st, ss in ((seed_t, seed_s), (seed_t, seed_s), (seed_t + 1, seed_s + 1)):
        model, opt, args, sd = _build(attn, "a", True)
        gt, gs = _generate(model, attn, "a", st, ss)
        runs.append((gt, gs, {k: v.clone() for k, v in model.state_dict().items() if "batch_norm" in k or "batchnorm" in k}))
    (gt1, gs1, st1), (gt2, gs2, st2), (gt3, gs3, st3) = runs
    assert all(torch.equal(a, b) for a, b in zip(gt1, gt2)) and all(torch.equal(a, b) for a, b in zip(gs1, gs2)) and all(torch.equal(st1[k], st2[k]) for k in st1)
    assert gs3[0].shape != gs1[0].shape or not torch.equal(gs3[0], gs1[0]), "a different seed must change the masks"
    assert not torch.equal(st3["text_m.prenet.batch_norm3.running_mean"], st1["text_m.prenet.batch_norm3.running_mean"])


def _batch():
    text, mel, tl, ml = CM.setup_batch()
    return text, mel, torch.tensor(tl), torch.tensor(ml)


def _cm(model, args, batch, accum, max_text, max_speech, fixed_sums=True, seed=0):
    from unast_amd import config, train, utils
    from unast_amd import train_rnn_step as RS
    saved = (utils.is_deterministic(), config.DETERMINISTIC_SUMS, train.DEVICE, RS.RECORD, RS.TEXT_MAX_LEN, RS.SPEECH_MAX_LEN)
    utils.set_seed(seed)
    utils.set_deterministic(True, fixed_sums=fixed_sums)
    train.DEVICE, RS.RECORD, RS.TEXT_MAX_LEN, RS.SPEECH_MAX_LEN = _dev(), True, max_text, max_speech
    losses = defaultdict(list)
    try:
        train.freeze_model_parameters(model.discriminator)
        out = RS.train_cm_step(losses, model, batch, 0, accum, args)
        torch.cuda.synchronize()
    finally:
        utils.set_deterministic(saved[0], fixed_sums=saved[1])
        train.DEVICE, RS.RECORD, RS.TEXT_MAX_LEN, RS.SPEECH_MAX_LEN = saved[2:]
    return {k: float(v[0]) for k, v in losses.items()}, float(out)


@pytest.mark.parametrize("drops", [False, True])
@pytest.mark.parametrize("attn", ATTNS)
def test_cm_substep_against_the_mirror(attn, drops):
    """train_cm_step (identity permutation: is_deterministic()) against rnn_cm_mirror.cm_step on CM_BATCH, whose memories come from the encoders:
    with dropout 0, and at the configs' rates 0.5 / 0.3 / 0.1 under the kernels' own masks on all eight tapes, after set_seed(SETUP[attn]['cm'][3])
    (chosen on the CPU so that both generations keep MARGIN; tests/test_cpu_rnn_cm.py pins that).  The discriminator's own dropout (0.2, seeded
    inside its forward) is switched off: its sites are not on a tape."""
    model, opt, args, sd = _build(attn, "cm", drops)
    if drops:
        model.discriminator.dropout_p = 0.0
    cs = CM.CM_BATCH
    batch = _batch()
    seed = CM.SETUP[attn]["cm"][3] if drops else 0
    disc0 = {k: v.clone() for k, v in model.state_dict().items() if k.startswith("discriminator.")}
    losses, out = _cm(model, args, batch, 3, cs["max_text"], cs["max_speech"], seed=seed)
    rec = model._rnn_step_record
    gt, gs = rec["gen_text"], rec["gen_speech"]
    tapes = rec["tapes"]
    if drops:
        # the eight seeds reach the eight tapes in the order the mirror draws them: every tape lists the sites the CPU test predicted and pinned
        got_sites = dict(tapes, gen_text=gt, gen_speech=gs, **rec["mem_tapes"])
        assert rec["seeds"] == [CM.cm_seeds(seed)[k] for k in CM.GEN_TAPES]
        want_sites = CM.cm_sites(seed, gt.lens_host, gs.lens_host)
        assert sorted(want_sites) == sorted(CM.GEN_TAPES)
        for name, want in want_sites.items():
            assert CM.plain(got_sites[name].sites) == CM.plain(want), name
    masks = dict(gen_text=CM.masks_of(gt.sites), gen_speech=CM.masks_of(gs.sites))
    for name in ("text_enc", "speech_enc", "text_dec", "speech_dec"):
        masks[name] = CM.masks_of(tapes[name].sites)
    for name in ("speech_mem", "text_mem"):                                                     # the two encoders that ran without a backward
        masks[name] = CM.masks_of(rec["mem_tapes"][name].sites)
    text, mel, tl, ml = batch
    mir = SM.Mirror(sd, attn, args)
    mgt, mgs = CM.cm_step(mir, text, tl.tolist(), mel, ml.tolist(), 3, cs["max_text"], cs["max_speech"], masks)
    mir32 = SM.Mirror(sd, attn, args, dtype=torch.float32)
    mgt32, mgs32 = CM.cm_step(mir32, text, tl.tolist(), mel, ml.tolist(), 3, cs["max_text"], cs["max_speech"], masks)
    assert torch.equal(mgt32["tokens"], mgt["tokens"]) and mgs32["lens"].tolist() == mgs["lens"].tolist(), "the fp32 mirror must decide as the fp64 one"
    print("mirror: text lens %s gap %.3g live PAD %d; speech lens %s stop margin %.3g" % (mgt["lens"].tolist(), mgt["gap"], mgt["live_pad"], mgs["lens"].tolist(),
                                                                                       mgs["stop_margin"]))
    assert mgt["gap"] >= CM.MARGIN and mgs["stop_margin"] >= CM.MARGIN, "the sub-step's generations lost their decision margins"
    assert gt.lens_host == mgt["lens"].tolist() and torch.equal(gt[0].cpu(), mgt["tokens"]) and gs.lens_host == mgs["lens"].tolist()
    assert rec["live_pad"] == mgt["live_pad"] == model._rnn_cm_live_pad
    for k in ("t_cm", "s_cm", "d_cm"):
        ref = mir.losses[k][0]
        print("loss %-5s got %.6f ref %.6f" % (k, losses[k], ref))
        assert abs(losses[k] - ref) <= 1e-3 * max(1.0, abs(ref)), k
    assert abs(out - sum(mir.losses[k][0] for k in ("t_cm", "s_cm", "d_cm")) / 3) <= 1e-3 * max(1.0, abs(out))
    got = {k: p.grad.detach().cpu().double() for k, p in model.named_parameters() if not k.startswith("discriminator.") and p.grad is not None}
    assert sorted(got) == sorted(mir.grads), sorted(set(got) ^ set(mir.grads))
    e32 = {k: SF.rel(mir32.grads[k].double().numpy(), g.numpy()) for k, g in mir.grads.items()}
    bounds, common = SF.grad_bounds(e32, "a")
    errs = {k: SF.rel(got[k].numpy(), mir.grads[k].numpy()) for k in bounds}
    for k in sorted(errs, key=lambda k: errs[k] / bounds[k])[-4:] + [k for k in SF.ILL if k in errs]:
        print("grad %-64s %.3g = %.3f of its bound %.3g (mirror's own e32 %.2g)" % (k, errs[k], errs[k] / bounds[k], bounds[k], e32[k]))
    bad = {k: "%.2e > %.2e" % (errs[k], bounds[k]) for k in errs if errs[k] > bounds[k]}
    assert not bad, bad
    # the discriminator: frozen, no gradient, bit-unchanged
    assert all(p.grad is None or p.grad.abs().max().item() == 0.0 for p in model.discriminator.parameters())
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in disc0.items())
    # running statistics and counters of every BatchNorm
    for k, v in model.state_dict().items():
        if k.endswith("num_batches_tracked") and not k.startswith("discriminator."):
            assert int(v) == int(mir.sd[k]), (k, int(v), int(mir.sd[k]))
        elif k.endswith(("running_mean", "running_var")):
            _close(k, v, mir.sd[k].double(), mir32.sd[k], 2e-5)


@pytest.mark.parametrize("attn", ATTNS)
def test_step_with_every_substep_runs_twice_to_the_bit(attn):
    """A loop of three train_rnn_step.train_step iterations at ae_steps = cm_steps = sp_steps = d_steps = 1 with the configs' dropout rates (from the
    second on the generations run on weights the optimizer has moved and on rebuilt packs): finite losses under every key at every iteration, and
    two such loops from the same state under set_deterministic(True, fixed_sums=True) agree to the bit."""
    from unast_amd import config, train, utils
    from unast_amd import train_rnn_step as RS
    cs = CM.CM_BATCH
    batch = _batch()
    saved = (utils.is_deterministic(), config.DETERMINISTIC_SUMS, train.DEVICE, RS.TEXT_MAX_LEN, RS.SPEECH_MAX_LEN)
    outs = []
    try:
        utils.set_deterministic(True, fixed_sums=True)
        train.DEVICE, RS.TEXT_MAX_LEN, RS.SPEECH_MAX_LEN = _dev(), cs["max_text"], cs["max_speech"]
        for _ in range(2):
            model, opt, args, sd = _build(attn, "cm", True, cm_steps=1)
            utils.set_seed(3)
            losses = defaultdict(list)
            for it in range(3):
                RS.train_step(losses, model, opt, None, dict(unsup=[batch], cm=[batch], sup=[batch], disc=[batch]), it, args)
                torch.cuda.synchronize()
                assert all(len(v) == it + 1 and np.isfinite(float(v[it])) for v in losses.values()), (it, dict(losses))
            outs.append(({k: [float(x) for x in v] for k, v in losses.items()}, {k: v.clone() for k, v in model.state_dict().items()}))
    finally:
        utils.set_deterministic(saved[0], fixed_sums=saved[1])
        train.DEVICE, RS.TEXT_MAX_LEN, RS.SPEECH_MAX_LEN = saved[2:]
    (l1, s1), (l2, s2) = outs
    print(l1)
    assert sorted(l1) == sorted(("t_ae", "s_ae", "d_ae", "t_cm", "s_cm", "d_cm", "asr_", "tts_", "sp_d", "d"))
    assert all(len(v) == 3 and np.isfinite(v).all() for v in l1.values())
    assert l1 == l2 and all(torch.equal(s1[k], s2[k]) for k in s1), [k for k in s1 if not torch.equal(s1[k], s2[k])]
    assert any(not torch.equal(s1[k], sd[k].to(s1[k].device)) for k in s1 if k.startswith("text_m.encoder")), "the step moved the parameters"


def test_what_is_refused_before_a_launch():
    from unast_amd import train_rnn as TR
    model, opt, args, sd = _build("luong", "a", False)
    dev = _dev()
    enc, h, c = (torch.from_numpy(x).to(dev) for x in _memory("a"))
    with pytest.raises(ValueError, match="B >= 2"):
        TR.text_generate_train(model.text_m, ((h[:, :1], c[:, :1]), enc[:1]), [9], max_len=4)
    with pytest.raises(TypeError, match="TextRNN"):
        TR.text_generate_train(model.speech_m, ((h, c), enc), [9, 6, 4], max_len=4)
    with pytest.raises(TypeError, match="SpeechRNN"):
        TR.speech_generate_train(model.text_m, ((h, c), enc), [9, 6, 4], max_len=4)
    model.eval()
    with pytest.raises(RuntimeError, match="train mode"):
        TR.text_generate_train(model.text_m, ((h, c), enc), [9, 6, 4], max_len=4)
    model.train()
    with pytest.raises(NotImplementedError, match=r"train\(\) mode"):                        # the module's own infer_sequence keeps refusing train mode
        model.text_m.infer_sequence(((h, c), enc), None, max_len=4)


# ---- the sub-step and the optimizer step against the reference's fixtures (tests/golden/rnn_cm_{luong,lsa}.npz) -------------------------------------------
def _build_fixture(attn, case):
    from unast_amd import train
    args = SF.args_of(attn, 0.0, cm_steps=1)
    saved = train.DEVICE
    train.DEVICE = _dev()
    try:
        _, _, model, opt, sched = train.initialize_model(args)
    finally:
        train.DEVICE = saved
    sd = CM.fixture_state_dict(attn, case)
    assert list(model.state_dict()) == list(sd) == CF.meta(attn)["keys"]
    model.load_state_dict(sd)
    if case == "a_eps":
        for i in (1, 2, 3):
            getattr(model.text_m.prenet, "batch_norm%d" % i).eps = CF.meta(attn)["eps_cond"]
    _zero_epoch()
    return model.train(), opt, args, sd


@pytest.mark.parametrize("case", CF.CASES)
@pytest.mark.parametrize("attn", ATTNS)
def test_cm_substep_matches_the_reference_fixture(attn, case):
    """freeze(D); train_cm_step; optimizer_step against the reference's own run (dropout 0, identity permutation).  Bounds: tests/rnn_step_fixture.py's
     on this fixture's e32: tokens and lengths exactly; frames and stop logits 16 x e32; losses 1e-3 x max(1, |ref|); gradients decoder
    side min(1e-3, 16 x max(common, own e32)), encoder side 1e-3, the three ill-conditioned text-prenet tensors at 16 x their own e32 (eps = 1e-5;
    the weight of the check is on a_eps); running statistics max(2e-5, 16 x e32); num_batches_tracked exactly; post-step parameters by 5l's rule.

    Measured on an MI355X: all six cases meet every bound; worst gradient ratio to its bound 0.35 (luong a), 0.55 (luong b), 0.78 (lsa a); frames
    0.02 .. 0.22 of 16 x e32; post-step moves at most 0.50 of their allowance."""
    from unast_amd import train_rnn_step as RS
    fx, m = CF.fixture(attn), CF.meta(attn)
    cfx = CM.CM_FIXTURE[attn]["a" if case == "a_eps" else case]
    model, opt, args, sd = _build_fixture(attn, case)
    text, mel, tl, ml = CM.fixture_batch(cfx)
    batch = (text, mel, torch.tensor(tl), torch.tensor(ml))
    disc0 = {k: v.clone() for k, v in model.state_dict().items() if k.startswith("discriminator.")}
    losses, out = _cm(model, args, batch, 1, cfx["max_text"], cfx["max_speech"], fixed_sums=None)
    rec = model._rnn_step_record
    gt, gs = rec["gen_text"], rec["gen_speech"]
    tag = "%s %s" % (attn, case)
    # ---- the two generations
    assert gt.lens_host == fx[case + "/gen/text_lens"].tolist() and gs.lens_host == fx[case + "/gen/speech_lens"].tolist()
    assert torch.equal(gt[0].cpu(), torch.from_numpy(fx[case + "/gen/tokens"])) and rec["live_pad"] == 0
    if case == "b":
        assert cfx["max_text"] in gt.lens_host and cfx["max_speech"] in gs.lens_host, "a sequence that never stops has length max_len"
    for i, k in enumerate(("pre", "post", "stop")):
        want, e32 = fx["%s/gen/%s" % (case, k)], float(fx["e32/%s/gen/%s" % (case, k)])
        err = np.abs(gs[i].cpu().double().numpy() - want).max()
        print("%s generated %-4s err %.3g (e32 %.3g, %.2f of 16 x e32)" % (tag, k, err, e32, err / (CF.FRAME_MARGIN * e32)))
        assert err <= CF.FRAME_MARGIN * e32, k
    # ---- losses
    for k in CF.LOSS_KEYS:
        want = float(fx["%s/loss/%s" % (case, k)])
        print("%s loss %-5s %.6f ref %.6f err %.2e" % (tag, k, losses[k], want, abs(losses[k] - want)))
        assert abs(losses[k] - want) <= SF.LOSS_TOL * max(1.0, abs(want)), k
    # ---- gradients: the key set (None / absent where the reference leaves None: the discriminator), then the bounds
    ref, gnorm, e32 = CF.grads(attn, case)
    got = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None and not k.startswith("discriminator.")}
    assert sorted(got) == sorted(ref), sorted(set(got) ^ set(ref))
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in model.discriminator.parameters())
    bounds, common = SF.grad_bounds(e32, case)
    errs = {k: SF.rel(SF.sample(got[k].cpu().double().numpy(), m["g_sample"]), ref[k]) for k in bounds}
    for k in sorted(errs, key=lambda k: errs[k] / bounds[k])[-4:] + [k for k in SF.ILL if k in errs]:
        print("%s grad %-66s %.3g = %.3f of its bound %.3g (own e32 %.2g)" % (tag, k, errs[k], errs[k] / bounds[k], bounds[k], e32[k]))
    bad = {k: "%.2e > %.2e" % (errs[k], bounds[k]) for k in errs if errs[k] > bounds[k]}
    assert not bad, bad
    # ---- running statistics and counters after the sub-step
    run, run_e32 = CF.running(attn, case)
    state = model.state_dict()
    for k, want in run.items():
        g = SF.sample(state[k].cpu().double().numpy(), m["p_sample"])
        err, lim = np.abs(g - want).max(), CF.running_bound(want, run_e32[k])
        assert err <= lim, (k, err, lim)
    nbt = __import__("json").loads(str(fx[case + "/num_batches_tracked"]))
    assert {k: int(state[k]) for k in nbt} == nbt
    # ---- optimizer_step: the pre-clip norm, the moves (5l's rule), the discriminator untouched to the bit
    RS.optimizer_step(model, opt, args)
    ref_norm = float(fx[case + "/norm"])
    assert opt.last_stepped == ["text_m", "speech_m"] and abs(opt.grad_norm() - ref_norm) <= SF.NORM_TOL * ref_norm
    after = model.state_dict()
    worst = (0.0, None)
    for k, b in bounds.items():
        p0 = sd[k].double().numpy().reshape(-1)
        idx = SF.sample_index(p0.size, m["g_sample"])
        want = SF.adamw_first_steps(p0[idx], ref[k], ref_norm, m["lr"], m["weight_decay"], m["grad_clip"])
        g = after[k].cpu().double().numpy().reshape(-1)[idx]
        tol = m["lr"] * (SF.MOVE_TOL + SF.move_slack(ref[k], gnorm[k], p0.size, b)) + 4 * np.spacing(np.abs(p0[idx]).astype(np.float32)).astype(np.float64)
        ratio = float((np.abs(g - want) / tol).max())
        worst = max(worst, (ratio, k))
    print("%s post-step: worst |dp - dp_ref| / allowance %.3g (%s)" % (tag, worst[0], worst[1]))
    assert worst[0] <= 1.0, worst
    assert all(torch.equal(v, after[k]) for k, v in disc0.items()), "the frozen discriminator is bit-unchanged after the generator step"
