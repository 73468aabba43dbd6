"""CPU-side checks of TextRNN decoder training (unast_amd.train_rnn.text_decoder_forward / text_decoder_backward): the fp64 mirror
(tests/text_decoder_mirror.py) against the reference's fixtures (tests/golden/text_rnn_decoder_train_{luong,lsa}.npz,
tools/gen_golden_text_rnn_decoder_train.py), the prefix slab's geometry, the C ABI's new symbols, the refusals that need no GPU, and the
metrics of tests/test_gpu_text_rnn_decoder_train.py against three planted faults."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import dropout_mirror as DM
from tests import rnn_train_mirror as TM
from tests import rnn_weights
from tests import text_decoder_mirror as XM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRAD_CAP, GRAD_MARGIN = 1e-3, 16.0
FWD_TOL = 1e-3                               # x max|ref| (DESIGN 5i's forward bound)
# running statistics: T <= 10 sequential fp32 momentum updates (2^-24 each) of batch statistics of fp32-level conv outputs (1e-6 of their scale)
BUF_TOL = 2e-5
ATTNS = ["luong", "lsa"]
P_PRE, P_DEC, P_POST = 0.5, 0.3, 0.1         # t_pre_drop, d_drop, t_post_drop of the reference's RNN configs


@functools.lru_cache(maxsize=None)
def fixture(attn):
    z = np.load(os.path.join(GOLDEN, "text_rnn_decoder_train_%s.npz" % attn))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _sd(attn):
    m = rnn_weights.meta_of(fixture(attn))
    return rnn_weights.state_dict("text", m["text_keys"], m["text_shapes"], m["seed"], m["gains"])


def eps_of(attn, case):
    return rnn_weights.meta_of(fixture(attn))["eps_cond"] if case == "a_eps" else 1e-5


def case_a(attn):
    fx = fixture(attn)
    tgt = torch.from_numpy(fx["a_target"])
    V = fx["a/logits"].shape[2]
    cot = XM.cotangent(rnn_weights.meta_of(fx)["cot_seed"], tgt.shape[0], tgt.shape[1], V)
    return tgt, torch.from_numpy(fx["a_enc_output"]), torch.from_numpy(fx["a_h"]), torch.from_numpy(fx["a_c"]), fx["a_lens_k"], cot


def case_b(attn):
    fx = fixture(attn)
    text = torch.from_numpy(fx["b_text"])
    return text, fx["b_text_len"], XM.cotangent(rnn_weights.meta_of(fx)["cot_seed"] + 1, text.shape[0], text.shape[1], fx["b/logits"].shape[2])


@functools.lru_cache(maxsize=None)
def mirror_a(attn, case="a"):
    tgt, enc, h, c, lens_k, cot = case_a(attn)
    return XM.run(_sd(attn), attn, tgt, enc, h, c, lens_k, cot, eps=eps_of(attn, case))


@functools.lru_cache(maxsize=None)
def mirror_b(attn):
    text, lens, cot = case_b(attn)
    return XM.autoencoder(_sd(attn), attn, text, lens, cot)


def grad_bounds(fx, case, names):
    """The bounds of one case from the fixture's e32 figures: tests/text_decoder_mirror.grad_bounds (three ill-conditioned tensors at 16 x
    their own e32, uncapped) or, for the conditioned case, conditioned_bounds (every tensor at min(1e-3, 16 x common e32))."""
    e32 = {k: float(fx["e32/%s/grad/%s" % (case, k)]) for k in names}
    return (XM.conditioned_bounds if case == "a_eps" else XM.grad_bounds)(e32, GRAD_CAP, GRAD_MARGIN)


def _rel(got, ref):
    return np.abs(np.asarray(got) - ref).max() / max(np.abs(ref).max(), 1e-300)


def _check_grads_fp64(fx, case, grads, stride):
    worst = 0.0
    for k, g in grads.items():
        key = "%s/gsample/%s" % (case, k)
        if k in XM.DEGENERATE or k in TM.DEGENERATE:
            assert g.abs().max().item() <= 1e-9 and float(fx["%s/gnorm/%s" % (case, k)]) <= 1e-9
            continue
        gn = float(fx["%s/gnorm/%s" % (case, k)])
        worst = max(worst, abs(g.norm().item() - gn) / gn)
        if key in fx:
            worst = max(worst, _rel(TM.sample(g.numpy())[::stride], fx[key]))
    return worst


def _check_buffers(fx, case, r):
    worst, n = 0.0, 0
    for k, v in r.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(fx["%s/%s" % (case, k)]), k
            n += 1
        elif "running_" in k:
            worst = max(worst, _rel(v.numpy(), fx["%s/%s" % (case, k)]))
            n += 1
    assert n == 9
    return worst


@pytest.mark.parametrize("case", ["a", "a_eps"])
@pytest.mark.parametrize("attn", ATTNS)
def test_mirror_reproduces_the_reference_fixture_decoder_alone(attn, case):
    fx, r = fixture(attn), mirror_a(attn, case)
    assert sorted(r["grads"]) == sorted(XM.trained_keys(_sd(attn)))
    worst = max(_rel(r[k].numpy(), fx["%s/%s" % (case, k)]) for k in ("logits", "d_h", "d_c"))
    worst = max(worst, _rel(TM.sample(r["d_enc_output"].numpy()), fx[case + "/d_enc_output"]))
    worst = max(worst, _check_buffers(fx, case, r))
    worst = max(worst, _check_grads_fp64(fx, case, r["grads"], 1 if case == "a" else 2))
    print("%s %s text decoder mirror against the reference fixture: %.2e" % (attn, case, worst))
    assert worst <= 1e-9                       # measured 1e-12 .. 2e-11 (the zero-variance prefix amplifies fp64 rounding by 316 per stage)
    lens_k = fx["a_lens_k"]
    for b in range(len(lens_k)):
        assert r["d_enc_output"][b, int(lens_k[b]):].abs().sum().item() == 0.0
    assert int(fx[case + "/prenet.batch_norm1.num_batches_tracked"]) == int(_sd(attn)["prenet.batch_norm1.num_batches_tracked"]) + 9


@pytest.mark.parametrize("attn", ATTNS)
def test_mirror_reproduces_the_reference_fixture_autoencoder(attn):
    fx, r = fixture(attn), mirror_b(attn)
    worst = max(_rel(r[k].numpy(), fx["b/" + k]) for k in ("logits", "h", "c"))
    worst = max(worst, _rel(TM.sample(r["enc_output"].numpy()), fx["b/enc_output"]))
    worst = max(worst, _check_buffers(fx, "b", r))
    assert sorted(r["grads"]) == sorted(k[len("b/gnorm/"):] for k in fx if k.startswith("b/gnorm/"))
    worst = max(worst, _check_grads_fp64(fx, "b", r["grads"], 2))
    print("%s text autoencoder mirror against the reference fixture: %.2e" % (attn, worst))
    assert worst <= 1e-9


def test_fixtures_fit_the_size_limit_and_record_the_conditioning():
    for attn in ATTNS:
        assert os.path.getsize(os.path.join(GOLDEN, "text_rnn_decoder_train_%s.npz" % attn)) <= 900000
        fx = fixture(attn)
        for k in XM.ILL_CONDITIONED:                       # the reference's own fp32 run: ill-conditioned at eps = 1e-5, clean at eps = 0.1
            assert float(fx["e32/a/grad/" + k]) > 1e-4 and float(fx["e32/a_eps/grad/" + k]) < 2e-6, k


@pytest.mark.parametrize("B,T", [(2, 1), (2, 2), (3, 9)])
def test_prefix_layout(B, T):
    from unast_amd.train_rnn import prefix_layout, GAP
    lay = prefix_layout(B, T)
    assert GAP == 2 and lay.lens == [max(s, 1) for s in range(T)] and len(lay.off) == T
    kind = np.zeros(lay.total, np.int64)                    # 0 = untouched, 1 = live, 2 = gap
    for s in range(T):
        for b in range(B):
            r0 = lay.off[s] + b * (lay.lens[s] + GAP)
            assert (kind[r0:r0 + lay.lens[s] + GAP] == 0).all()          # no overlap
            kind[r0:r0 + lay.lens[s]] = 1
            kind[r0 + lay.lens[s]:r0 + lay.lens[s] + GAP] = 2
    assert (kind != 0).all()                                # no hole: the total is what the segments take
    assert (kind == 1).sum() == B * (1 + T * (T - 1) // 2)
    assert lay.total == B * (1 + T * (T - 1) // 2) + GAP * B * T
    assert kind[0] == 1 and (kind[-GAP:] == 2).all()        # the slab starts on a live row and ends in a gap
    # every live run is followed by exactly GAP gap rows: two sequences are never closer than a 5-tap conv's reach
    runs = np.flatnonzero(np.diff(np.concatenate([[2], kind])) != 0)
    for a, b_ in zip(runs, list(runs[1:]) + [lay.total]):
        if kind[a] == 2:
            assert b_ - a == GAP


def test_header_declares_the_prefix_entry_points():
    from unast_amd import _lib
    protos = _lib.parse_header()
    want = {"unast_prefix_bn_fwd": 26, "unast_prefix_bn_bwd": 23, "unast_prefix_embed_fwd": 16, "unast_prefix_embed_bwd": 11}
    for name, nargs in want.items():
        assert name in protos and len(protos[name][1]) == nargs, name
    # the entry points the slab reuses keep their argument counts
    old = {"unast_bn_fwd": 20, "unast_bn_bwd": 18, "unast_embed_fwd": 13, "unast_embed_bwd": 15, "unast_embed_bwd_det": 15, "unast_conv_fwd": 17,
           "unast_conv_dgrad": 14, "unast_conv_wgrad": 17, "unast_rnn_attn_step_train": 22, "unast_rnn_attn_step_bwd": 36, "unast_lstm_cell_train": 15,
           "unast_lstm_cell_bwd": 19}
    for name, nargs in old.items():
        assert len(protos[name][1]) == nargs, name


def test_text_decoder_refusals_without_a_gpu():
    from unast_amd import train_rnn
    from unast_amd.network import TextRNN, SpeechRNN
    tm, sm = TextRNN(rnn_weights.rnn_args("luong")), SpeechRNN(rnn_weights.rnn_args("lsa"))
    ids = torch.full((2, 6), 5, dtype=torch.int64)
    enc_outputs = ((torch.zeros(2, 2, 256), torch.zeros(2, 2, 256)), torch.zeros(2, 5, 512))
    with pytest.raises(TypeError):
        train_rnn.text_decoder_forward(sm.train(), ids, enc_outputs, [5, 3])
    with pytest.raises(RuntimeError, match="train"):
        train_rnn.text_decoder_forward(tm.eval(), ids, enc_outputs, [5, 3])
    tm.train()
    with pytest.raises(ValueError, match="B >= 2"):
        train_rnn.text_decoder_forward(tm, ids[:1], ((torch.zeros(2, 1, 256), torch.zeros(2, 1, 256)), torch.zeros(1, 5, 512)), [5])
    with pytest.raises(ValueError, match="T <= 512"):
        train_rnn.text_decoder_forward(tm, torch.zeros(2, 513, dtype=torch.int64), enc_outputs, [5, 3])
    with pytest.raises(ValueError, match="2 GiB"):
        train_rnn.text_decoder_forward(tm, torch.zeros(64, 512, dtype=torch.int64), enc_outputs, [5] * 64)
    with pytest.raises(ValueError, match="CUDA"):
        train_rnn.text_decoder_forward(tm, ids, enc_outputs, [5, 3])                  # a CPU model and CPU tensors
    with pytest.raises(TypeError):
        train_rnn.text_decoder_backward(object(), None)
    with pytest.raises(TypeError):
        train_rnn.text_decoder_backward(train_rnn.DecoderTape(), None)          # not from text_decoder_forward
    speech_tape = train_rnn.DecoderTape()
    speech_tape.entry = "decoder_forward"
    with pytest.raises(TypeError):
        train_rnn.text_decoder_backward(speech_tape, None)
    text_tape = train_rnn.DecoderTape()
    text_tape.entry = "text_decoder_forward"
    with pytest.raises(TypeError):
        train_rnn.decoder_backward(text_tape)
    text_tape.used = True
    with pytest.raises(RuntimeError, match="used"):
        train_rnn.text_decoder_backward(text_tape, None)
    # the existing interface still refuses train mode, and decoder_forward still refuses a TextRNN
    with pytest.raises(NotImplementedError):
        tm.decode_sequence(ids, [6, 6], enc_outputs, None)
    with pytest.raises(NotImplementedError, match="TextPrenet"):
        train_rnn.decoder_forward(tm, torch.zeros(2, 6, 80), enc_outputs, [5, 3])
    used = {train_rnn.S_EMB, train_rnn.S_NOISE, train_rnn.S_PRE1, train_rnn.S_PRE2, train_rnn.S_PRE3, train_rnn.S_EDROP, train_rnn.S_EDROP + 1,
            train_rnn.S_DPRE, train_rnn.S_DDROP, train_rnn.S_DOUT} | {train_rnn.S_POST + k for k in range(4)}
    new = {train_rnn.S_TEMB, train_rnn.S_TPRE, train_rnn.S_TPRE + 1, train_rnn.S_TPRE + 2, train_rnn.S_TPOST}
    assert len(new) == 5 and not (used & new)


def masks_for(B, T, E=256, seed=11):
    """Masks at the configs' probabilities on a case's shapes, from the kernels' RNG mirror, in the slab layout (any masks would do here)."""
    from unast_amd import train_rnn as TR
    R = TR.prefix_layout(B, T).total
    f = lambda stream, rows, cols, p: torch.from_numpy(DM.drop_factor(seed, stream, rows, cols, p))     # noqa: E731
    m = {"t_emb_dropout": f(TR.S_TEMB, R, E, P_PRE), "d_drop0": f(TR.S_DDROP, B * T, 256, P_DEC), "d_dropout1": f(TR.S_DOUT, B * T, 256, P_DEC),
         "t_post_dropout": f(TR.S_TPOST, B * T, 256, P_POST)}
    for i in range(3):
        m["t_dropout%d" % (i + 1)] = f(TR.S_TPRE + i, R, 256, P_PRE)
    return m


@pytest.mark.parametrize("attn,fault", [("luong", "sos_prefix"), ("lsa", "sos_prefix"), ("luong", "slab_stats"), ("lsa", "running_once")])
def test_the_metrics_see_the_planted_faults(attn, fault):
    """Each planted fault moves a checked quantity -- the logits, a gradient, or (for the running statistics' fault, which touches nothing
    else) a running statistic -- by at least 100 x the bound the GPU test applies, on case a's shapes under masks."""
    fx = fixture(attn)
    tgt, enc, h, c, lens_k, cot = case_a(attn)
    masks = masks_for(tgt.shape[0], tgt.shape[1])
    good = XM.run(_sd(attn), attn, tgt, enc, h, c, lens_k, cot, masks=masks)
    bad = XM.run(_sd(attn), attn, tgt, enc, h, c, lens_k, cot, masks=masks, fault=fault)
    names = [k for k in good["grads"] if k not in XM.DEGENERATE]
    bounds, _ = grad_bounds(fx, "a", names)
    ratio = {k: TM.normerr(bad["grads"][k], good["grads"][k]) / bounds[k] for k in names}
    for k in ("d_enc_output", "d_h", "d_c"):
        ratio[k] = TM.normerr(bad[k], good[k]) / min(GRAD_CAP, GRAD_MARGIN * float(fx["e32/a/rel/" + k]))
    ratio["logits"] = (bad["logits"] - good["logits"]).abs().max().item() / (FWD_TOL * good["logits"].abs().max().item())
    for k in good:
        if "running_" in k:
            ratio[k] = (bad[k] - good[k]).abs().max().item() / (BUF_TOL * max(1.0, good[k].abs().max().item()))
    if fault == "running_once":
        assert torch.equal(good["logits"], bad["logits"]) and all(torch.equal(good["grads"][k], bad["grads"][k]) for k in names)
        assert bad["prenet.batch_norm1.num_batches_tracked"] != good["prenet.batch_norm1.num_batches_tracked"]
    worst = max(ratio, key=ratio.get)
    print("%s %s: worst %s at %.0f x its bound" % (attn, fault, worst, ratio[worst]))
    assert ratio[worst] >= 100
