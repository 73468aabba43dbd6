"""unast_amd.train_rnn.text_decoder_forward / text_decoder_backward (TextRNN's teacher-forced train-mode decoder) on the GPU against the
reference's fixtures (tests/golden/text_rnn_decoder_train_{luong,lsa}.npz) and the fp64 mirror (tests/text_decoder_mirror.py, pinned to those
fixtures by tests/test_cpu_text_rnn_decoder_train.py).

Bounds: logits 1e-3 x max|ref|; running statistics 2e-5 x max(1, max|ref|) (BUF_TOL of the CPU test); every parameter gradient,
d_enc_output, d_h and d_c in per-tensor relative L2 norm against e32 = the reference's fp32-vs-fp64 error (dropout off: from the fixture) or
the mirror's under the same masks (dropout on):
  cases a, b       min(1e-3, 16 x e32) -- but the three tensors the zero-variance prefix [SOS] leaves ill-conditioned in fp32 (prenet.embed.weight,
                   prenet.conv1.conv.weight, prenet.batch_norm1.bias) at 16 x their OWN e32, uncapped (tests/text_decoder_mirror.grad_bounds);
  case a_eps       eps = 0.1 on the three prenet BatchNorms on both sides: EVERY tensor at min(1e-3, 16 x common e32) (conditioned_bounds).
The three prenet conv biases in front of a train-mode BatchNorm have mathematically zero gradients: max|g| <= 1e-6 x ||grad W|| of their conv
at eps = 0.1.  (At eps = 1e-5 the zero-variance segment multiplies rounding by 316 per stage and the bias gradient is the column sum of exactly
that residue; it is then held to the ill-conditioned tensors' own scale: 16 x e32 of conv1's weight, relative to ||grad W||.)"""
import math

import numpy as np
import pytest
import torch

from tests import dropout_mirror as DM
from tests import rnn_train_mirror as TM
from tests import rnn_weights
from tests import text_decoder_mirror as XM
from tests.test_cpu_text_rnn_decoder_train import (ATTNS, BUF_TOL, FWD_TOL, GRAD_CAP, GRAD_MARGIN, P_DEC, P_POST, P_PRE, case_a, case_b, eps_of, fixture,
                                                    mirror_a, mirror_b, _sd)

pytestmark = pytest.mark.gpu

DEG_ABS = 1e-6
REPEAT_TOL = 1e-5
DEC = ("prenet.", "decoder.", "postnet.")
TEXT_SITES = ["t_emb_dropout", "t_dropout1", "t_dropout2", "t_dropout3", "d_drop0", "d_dropout1", "t_post_dropout"]


def _dev():
    return torch.device("cuda:0")


def _model(attn, drops=None, eps=None, sd=None):
    from unast_amd.network import TextRNN
    args = rnn_weights.rnn_args(attn)
    if drops is not None:
        args.t_pre_drop = args.t_post_drop = args.e_drop = args.d_drop = drops
    m = TextRNN(args)
    sd = sd or _sd(attn)
    assert sorted(sd) == sorted(m.state_dict())
    m.load_state_dict(sd)
    if eps is not None:
        for i in (1, 2, 3):
            getattr(m.prenet, "batch_norm%d" % i).eps = eps
    return m.to(_dev()).train(), sd


def _f(t):
    return None if t is None else t.float().to(_dev())


def _run_a(model, attn, seed=0, accumulate=False):
    from unast_amd import train_rnn
    tgt, enc, h, c, lens_k, cot = case_a(attn)
    tape = train_rnn.text_decoder_forward(model, tgt.to(_dev()), ((_f(h), _f(c)), _f(enc)), lens_k, seed=seed)
    out = train_rnn.text_decoder_backward(tape, _f(cot), accumulate=accumulate)
    torch.cuda.synchronize()
    return tape, out


def _run_b(model, attn, seed=0):
    from unast_amd import train_rnn
    text, lens, cot = case_b(attn)
    etape = train_rnn.encoder_forward(model, text.to(_dev()), torch.from_numpy(np.asarray(lens)), seed=seed)
    dtape = train_rnn.text_decoder_forward(model, text.to(_dev()), etape, lens, seed=seed)
    d_enc, d_h, d_c = train_rnn.text_decoder_backward(dtape, _f(cot))
    train_rnn.encoder_backward(etape, d_enc, d_h, d_c, accumulate=True)
    torch.cuda.synchronize()
    return etape, dtape


def _grads(model, prefixes=DEC):
    return {k: p.grad.detach().cpu().double() for k, p in model.named_parameters() if k.startswith(prefixes)}


def _check_forward(tag, model, tape, ref, sd, updates):
    got = tape.logits.cpu().double().numpy()
    want = np.asarray(ref["logits"], dtype=np.float64)
    assert got.shape == want.shape
    err, mx = np.abs(got - want).max(), np.abs(want).max()
    print("%s logits err %.3g = %.3g of max|ref|" % (tag, err, err / mx))
    assert err <= FWD_TOL * mx
    n = 0
    for k, v in model.state_dict().items():
        if k.startswith("prenet.") and k.endswith(("running_mean", "running_var")):
            want = np.asarray(ref[k], dtype=np.float64)
            err = np.abs(v.cpu().double().numpy() - want).max()
            print("%s %-40s err %.3g (bound %.3g)" % (tag, k, err, BUF_TOL * max(1.0, np.abs(want).max())))
            assert err <= BUF_TOL * max(1.0, np.abs(want).max()), k
            n += 1
        if k.startswith("prenet.") and k.endswith("num_batches_tracked"):
            assert int(v) == int(sd[k]) + updates, (k, int(v))
            n += 1
    assert n == 9


def _check_grads(tag, got, ref, e32s, conditioned, deg_rel=DEG_ABS):
    """got / ref: {name: tensor} over parameters and returned cotangents; e32s: {name: e32} for the non-degenerate ones."""
    assert sorted(got) == sorted(ref), sorted(set(got) ^ set(ref))
    bounds, common = (XM.conditioned_bounds if conditioned else XM.grad_bounds)(e32s, GRAD_CAP, GRAD_MARGIN)
    errs = {k: TM.normerr(got[k], ref[k]) for k in e32s}
    for k in sorted(errs, key=lambda k: errs[k] / bounds[k])[-4:]:
        print("%s grad %-62s %.3g = %.2f of its bound %.3g (own e32 %.2g)" % (tag, k, errs[k], errs[k] / bounds[k], bounds[k], e32s[k]))
    worst = max(errs, key=lambda k: errs[k] / bounds[k])
    print("%s: common e32 %.3g, worst gradient %s %.3g, %.2f of its bound" % (tag, common, worst, errs[worst], errs[worst] / bounds[worst]))
    for k in XM.ILL_CONDITIONED:
        if k in errs:
            print("%s ill-conditioned %-40s err %.3g, own e32 %.3g, bound %.3g" % (tag, k, errs[k], e32s[k], bounds[k]))
    for k in XM.DEGENERATE:
        rel = got[k].abs().max().item() / got[k[:-4] + "weight"].norm().item()
        print("%s degenerate %s max|g| / ||grad W|| %.2e (bound %.2e)" % (tag, k, rel, deg_rel))
        assert rel <= deg_rel, (k, rel)
    bad = {k: "%.2e > %.2e" % (errs[k], bounds[k]) for k in errs if errs[k] > bounds[k]}
    assert not bad, bad


def _deg_rel(e32s, conditioned):
    return DEG_ABS if conditioned else max(DEG_ABS, GRAD_MARGIN * e32s["prenet.conv1.conv.weight"])


def _with_cots(grads, r):
    return dict(grads, d_enc_output=r["d_enc_output"], d_h=r["d_h"], d_c=r["d_c"])


# ---- 1. dropout off, against the reference fixtures -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "a_eps"])
@pytest.mark.parametrize("attn", ATTNS)
def test_decoder_alone_matches_the_reference_fixture(attn, case):
    fx, mir = fixture(attn), mirror_a(attn, case)
    model, sd = _model(attn, drops=0.0, eps=eps_of(attn, case) if case == "a_eps" else None)
    tape, (d_enc, d_h, d_c) = _run_a(model, attn)
    assert tape.sites == []
    B, T = fx["a_target"].shape
    assert tape.logits.shape == (B, T, 46) and d_enc.shape == (B, 12, 512) and d_h.shape == (2, B, 256) and d_c.shape == (2, B, 256)
    ref = {k[len(case) + 1:]: fx[k] for k in fx if k.startswith(case + "/") and "/g" not in k}
    _check_forward("%s %s" % (attn, case), model, tape, ref, sd, T)
    for b, n in enumerate(fx["a_lens_k"]):
        assert d_enc[b, int(n):].abs().sum().item() == 0.0, "d_enc_output rows past lens_k must be exactly zero"
    got = _with_cots(_grads(model), dict(d_enc_output=d_enc.cpu().double(), d_h=d_h.cpu().double(), d_c=d_c.cpu().double()))
    want = _with_cots(mir["grads"], mir)
    e32s = {k: float(fx["e32/%s/grad/%s" % (case, k)]) for k in mir["grads"] if k not in XM.DEGENERATE}
    e32s.update({k: float(fx["e32/%s/rel/%s" % (case, k)]) for k in ("d_enc_output", "d_h", "d_c")})
    assert all(got[k].shape == want[k].shape for k in got)
    _check_grads("%s %s" % (attn, case), got, want, e32s, case == "a_eps", _deg_rel(e32s, case == "a_eps"))
    assert all(p.grad is None for k, p in model.named_parameters() if not k.startswith(DEC))


@pytest.mark.parametrize("attn", ATTNS)
def test_autoencoder_matches_the_reference_fixture(attn):
    fx, mir = fixture(attn), mirror_b(attn)
    model, sd = _model(attn, drops=0.0)
    etape, dtape = _run_b(model, attn)
    ref = {k[2:]: fx[k] for k in fx if k.startswith("b/") and "/g" not in k}
    _check_forward(attn + " b", model, dtape, ref, sd, fx["b_text"].shape[1] + 1)          # the encoder's update, then the decoder's T
    got = _grads(model, ("prenet.", "encoder.", "decoder.", "postnet."))
    e32s = {k: float(fx["e32/b/grad/" + k]) for k in mir["grads"] if k not in XM.DEGENERATE}
    _check_grads(attn + " b", got, dict(mir["grads"]), e32s, False, _deg_rel(e32s, False))


# ---- 2. the configs' dropout rates, against the mirror under the kernels' own masks ---------------------------------------------------------------------
def _site_masks(tape):
    masks, streams = {}, set()
    for s in tape.sites:
        epoch = int(s.epoch.item())
        assert s.stream not in streams, "two sites share stream id %d" % s.stream
        streams.add(s.stream)
        keep = DM.keep_mask(s.seed, s.stream, s.rows, s.cols, s.p, epoch)
        masks[s.name] = torch.from_numpy(keep * float(DM.drop_scale(s.p)))
        rate, sdv = keep.mean(), math.sqrt(s.p * (1 - s.p) / keep.size)
        print("site %-18s p %.2f stream %2d [%d,%d]: keep rate %.4f (%.2f sd from 1 - p)" % (s.name, s.p, s.stream, s.rows, s.cols, rate, (rate - (1 - s.p)) / sdv))
        assert abs(rate - (1 - s.p)) <= 4 * sdv, (s.name, rate)
    return masks


def _check_sites(tape, B, T):
    from unast_amd.train_rnn import prefix_layout
    R = prefix_layout(B, T).total
    assert [s.name for s in tape.sites] == TEXT_SITES
    assert [s.p for s in tape.sites] == [P_PRE] * 4 + [P_DEC] * 2 + [P_POST]
    assert [(s.rows, s.cols) for s in tape.sites] == [(R, 256)] * 4 + [(B * T, 256)] * 3


@pytest.mark.parametrize("case", ["a", "a_eps"])
@pytest.mark.parametrize("attn", ATTNS)
def test_decoder_alone_with_dropout_matches_the_mirror_under_the_kernels_masks(attn, case):
    eps = eps_of(attn, case)
    model, sd = _model(attn, eps=eps if case == "a_eps" else None)
    tape, (d_enc, d_h, d_c) = _run_a(model, attn, seed=20240)
    tgt, enc, h, c, lens_k, cot = case_a(attn)
    _check_sites(tape, *tgt.shape)
    masks = _site_masks(tape)
    r64 = XM.run(sd, attn, tgt, enc, h, c, lens_k, cot, masks=masks, eps=eps)
    r32 = XM.run(sd, attn, tgt, enc, h, c, lens_k, cot, masks=masks, eps=eps, dtype=torch.float32)
    _check_forward("%s %s dropout" % (attn, case), model, tape, {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in r64.items() if k != "grads"}, sd, tgt.shape[1])
    got = _with_cots(_grads(model), dict(d_enc_output=d_enc.cpu().double(), d_h=d_h.cpu().double(), d_c=d_c.cpu().double()))
    want, w32 = _with_cots(r64["grads"], r64), _with_cots(r32["grads"], r32)
    e32s = {k: TM.normerr(w32[k], want[k]) for k in want if k not in XM.DEGENERATE}
    _check_grads("%s %s dropout" % (attn, case), got, want, e32s, case == "a_eps", _deg_rel(e32s, case == "a_eps"))


@pytest.mark.parametrize("attn", ATTNS)
def test_autoencoder_with_dropout_matches_the_mirror_under_the_kernels_masks(attn):
    model, sd = _model(attn)
    etape, dtape = _run_b(model, attn, seed=777)
    text, lens, cot = case_b(attn)
    _check_sites(dtape, *text.shape)
    assert not {s.stream for s in etape.sites} & {s.stream for s in dtape.sites}, "encoder and decoder sites must not share a stream id"
    em, dm = _site_masks(etape), _site_masks(dtape)
    r64 = XM.autoencoder(sd, attn, text, lens, cot, enc_masks=em, dec_masks=dm)
    r32 = XM.autoencoder(sd, attn, text, lens, cot, enc_masks=em, dec_masks=dm, dtype=torch.float32)
    _check_forward(attn + " b dropout", model, dtape, {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in r64.items() if not k.endswith("grads")}, sd,
                   text.shape[1] + 1)
    got = _grads(model, ("prenet.", "encoder.", "decoder.", "postnet."))
    e32s = {k: TM.normerr(r32["grads"][k], r64["grads"][k]) for k in r64["grads"] if k not in XM.DEGENERATE}
    _check_grads(attn + " b dropout", got, dict(r64["grads"]), e32s, False, _deg_rel(e32s, False))


# ---- 3. ASR wiring: a speech encoder's tape as the memory ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attn", ATTNS)
def test_speech_encoder_tape_as_memory(attn):
    from unast_amd import train_rnn
    from unast_amd.network import SpeechRNN
    from unast_amd.portable import synth_batch
    B, T, T_mel = 2, 5, 12
    model, sd = _model(attn)
    args = rnn_weights.rnn_args(attn)
    sm = SpeechRNN(args)
    ssd = sm.state_dict()
    sm.load_state_dict(rnn_weights.state_dict("speech", list(ssd), [list(v.shape) for v in ssd.values()], 77, []))
    sm = sm.to(_dev()).train()
    _, mel, _, _ = synth_batch(B, 12, T_mel, seed=3)
    mel = torch.from_numpy(mel[:, :T_mel].copy())
    mel[1, 9:] = 0.0
    lens = [T_mel, 9]
    tgt = torch.from_numpy(XM.tokens(5, B, T))
    cot = XM.cotangent(6, B, T, 46)
    etape = train_rnn.encoder_forward(sm, _f(mel), torch.tensor(lens), seed=3)
    dtape = train_rnn.text_decoder_forward(model, tgt.to(_dev()), etape, lens, seed=4)
    d_enc, d_h, d_c = train_rnn.text_decoder_backward(dtape, _f(cot))
    d_mel = train_rnn.encoder_backward(etape, d_enc, d_h, d_c)
    torch.cuda.synchronize()
    assert d_mel.shape == (B, T_mel, 80) and torch.isfinite(d_mel).all() and d_mel.abs().max().item() > 0.0
    assert d_enc[1, 9:].abs().sum().item() == 0.0
    masks = _site_masks(dtape)
    (h, c), enc = etape.hidden, etape.enc_output
    r64 = XM.run(sd, attn, tgt, enc.cpu(), h.cpu(), c.cpu(), lens, cot, masks=masks)
    r32 = XM.run(sd, attn, tgt, enc.cpu(), h.cpu(), c.cpu(), lens, cot, masks=masks, dtype=torch.float32)
    err = (dtape.logits.cpu().double() - r64["logits"]).abs().max().item()
    assert err <= FWD_TOL * r64["logits"].abs().max().item()
    got = _with_cots(_grads(model), dict(d_enc_output=d_enc.cpu().double(), d_h=d_h.cpu().double(), d_c=d_c.cpu().double()))
    want, w32 = _with_cots(r64["grads"], r64), _with_cots(r32["grads"], r32)
    e32s = {k: TM.normerr(w32[k], want[k]) for k in want if k not in XM.DEGENERATE}
    _check_grads(attn + " asr", got, want, e32s, False, _deg_rel(e32s, False))
    assert all(p.grad is not None for k, p in sm.named_parameters() if k.startswith(("prenet.", "encoder.")))


# ---- 4. accumulate, bit-equality, .grad in place, a tape's single use, the eval path afterwards ----------------------------------------------------------
@pytest.mark.parametrize("attn", ATTNS)
def test_accumulate_repeat_and_grads_in_place(attn):
    from unast_amd import config, train_rnn, utils
    model, _ = _model(attn)                                                                      # dropout on: the masks are part of what must repeat
    params = [p for k, p in model.named_parameters() if k.startswith(DEC)]
    for p in params:
        p.grad = torch.full_like(p, float("nan"))
    ptrs = [p.grad.data_ptr() for p in params]
    saved = (utils.is_deterministic(), config.DETERMINISTIC_SUMS)
    buffers = {k: v.clone() for k, v in model.state_dict().items() if "batch_norm" in k and "running" in k or "num_batches" in k}
    utils.set_deterministic(True, fixed_sums=True)
    try:
        tape1, out1 = _run_a(model, attn, seed=9)                                                # accumulate=False over NaN
        assert [p.grad.data_ptr() for p in params] == ptrs, "an existing dense fp32 .grad must stay in place"
        first = _grads(model)
        assert all(torch.isfinite(g).all() for g in first.values())
        with pytest.raises(RuntimeError, match="used"):
            train_rnn.text_decoder_backward(tape1, out1[0])
        model.load_state_dict(buffers, strict=False)                                             # the same running statistics for the second call
        tape2, out2 = _run_a(model, attn, seed=9)
        second = _grads(model)
    finally:
        utils.set_deterministic(*saved)
    for name, a, b in zip(("logits", "d_enc_output", "d_h", "d_c"), (tape1.logits,) + tuple(out1), (tape2.logits,) + tuple(out2)):
        assert torch.equal(a, b), name
    differ = [k for k in first if not torch.equal(first[k], second[k])]
    assert not differ, differ
    _run_a(model, attn, seed=9, accumulate=True)
    third = _grads(model)
    worst = max(TM.normerr(third[k], 2 * second[k]) for k in second if k not in XM.DEGENERATE)
    print("%s accumulate=True over a first result against twice the first: %.2e" % (attn, worst))
    assert worst <= REPEAT_TOL
    assert all(p.grad is None for k, p in model.named_parameters() if not k.startswith(DEC))
    assert tape1.saved_bytes() > 0
    # the eval path still refuses train mode and, in eval mode, answers from operands rebuilt after the running statistics moved
    tgt, enc, h, c, lens_k, _ = case_a(attn)
    with pytest.raises(NotImplementedError):
        model.decode_sequence(tgt.to(_dev()), None, ((_f(h), _f(c)), _f(enc)), None)
    mask = (torch.arange(enc.shape[1])[None, :] >= torch.from_numpy(np.asarray(lens_k))[:, None]).to(_dev())
    with torch.no_grad():
        model.eval()
        before = model.decode_sequence(tgt.to(_dev()), None, ((_f(h), _f(c)), _f(enc)), mask)
        assert "_rnn_pack" in model.__dict__
        model.train()
        _run_a(model, attn, seed=10)
        assert "_rnn_pack" not in model.__dict__, "the cached eval operands must be dropped: the running statistics moved"
        after = model.eval().decode_sequence(tgt.to(_dev()), None, ((_f(h), _f(c)), _f(enc)), mask)
    assert before.shape == after.shape and torch.isfinite(after).all()
    assert not torch.equal(before, after), "eval logits must follow the moved running statistics"


# ---- 5. a single position -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attn", ATTNS)
def test_single_position(attn):
    from unast_amd import train_rnn
    model, sd = _model(attn, eps=0.1)            # T = 1 is the [SOS] prefix alone (rows that differ by their dropout masks only): the conditioned setting
    tgt, enc, h, c, lens_k, _ = case_a(attn)
    tgt = tgt[:, :1]
    cot = XM.cotangent(3, tgt.shape[0], 1, 46)
    tape = train_rnn.text_decoder_forward(model, tgt.to(_dev()), ((_f(h), _f(c)), _f(enc)), lens_k, seed=5)
    d_enc, d_h, d_c = train_rnn.text_decoder_backward(tape, _f(cot))
    torch.cuda.synchronize()
    masks = {s.name: torch.from_numpy(DM.drop_factor(s.seed, s.stream, s.rows, s.cols, s.p, int(s.epoch.item()))) for s in tape.sites}      # (9 rows: no rate check)
    r64 = XM.run(sd, attn, tgt, enc, h, c, lens_k, cot, masks=masks, eps=0.1)
    r32 = XM.run(sd, attn, tgt, enc, h, c, lens_k, cot, masks=masks, eps=0.1, dtype=torch.float32)
    _check_forward(attn + " T=1", model, tape, {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in r64.items() if k != "grads"}, sd, 1)
    got = _with_cots(_grads(model), dict(d_enc_output=d_enc.cpu().double(), d_h=d_h.cpu().double(), d_c=d_c.cpu().double()))
    want, w32 = _with_cots(r64["grads"], r64), _with_cots(r32["grads"], r32)
    e32s = {k: TM.normerr(w32[k], want[k]) for k in want if k not in XM.DEGENERATE}
    _check_grads(attn + " T=1", got, want, e32s, True)
