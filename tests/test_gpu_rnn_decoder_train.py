"""unast_amd.train_rnn.decoder_forward / decoder_backward (SpeechRNN's teacher-forced train-mode decoder) on the GPU against the reference's
fixtures (tests/golden/rnn_decoder_train_{luong,lsa}.npz) and the fp64 mirror (tests/rnn_decoder_mirror.py, pinned to those fixtures by
tests/test_cpu_rnn_decoder_train.py).

Bounds: forward tensors 1e-3 x max|ref|; every parameter gradient, d_enc_output, d_h, d_c and d_mel min(1e-3, 16 x e32) in
per-tensor relative L2 norm, e32 = the reference's fp32-vs-fp64 error (dropout off: from the fixture) or the mirror's under the same masks
(dropout on), formed per case as tests/rnn_decoder_mirror.grad_bounds describes; worst cases are printed as multiples of e32.  The four
post-net conv biases in front of a train-mode BatchNorm have mathematically zero gradients: max|g| <= 1e-6 x ||grad W|| of their conv."""
import math

import numpy as np
import pytest
import torch

from tests import dropout_mirror as DM
from tests import rnn_decoder_mirror as RD
from tests import rnn_train_mirror as TM
from tests import rnn_weights
from tests.test_cpu_rnn_decoder_train import ATTNS, case_a, case_b, fixture, mirror_a, mirror_b, _sd

pytestmark = pytest.mark.gpu

PARITY = 1e-3
GRAD_CAP, GRAD_MARGIN = 1e-3, 16.0
DEG_ABS = 1e-6
REPEAT_TOL = 1e-5          # two runs of one backward where fp32 / fp64 atomics order the column sums (tests/test_gpu_rnn_train_model.py)
DEC = ("prenet.", "decoder.", "postnet.")


def _dev():
    return torch.device("cuda:0")


def _model(attn, drops=0.0):
    from unast_amd.network import SpeechRNN
    args = rnn_weights.rnn_args(attn)
    args.s_pre_drop = args.s_post_drop = args.e_drop = args.d_drop = drops
    m = SpeechRNN(args)
    sd = _sd(attn)
    assert sorted(sd) == sorted(m.state_dict())
    m.load_state_dict(sd)
    return m.to(_dev()).train(), sd


def _f(t):
    return None if t is None else t.float().to(_dev())


def _run_a(model, attn, seed=0, cot=True, accumulate=False):
    from unast_amd import train_rnn
    tgt, enc, h, c, lens_k, cots = case_a(attn)
    tape = train_rnn.decoder_forward(model, _f(tgt), ((_f(h), _f(c)), _f(enc)), lens_k, seed=seed)
    out = train_rnn.decoder_backward(tape, *((_f(x) for x in cots) if cot else ()), accumulate=accumulate)
    torch.cuda.synchronize()
    return tape, out


def _run_b(model, attn, seed=0, noise_in=False):
    from unast_amd import train_rnn
    mel, lens, cots = case_b(attn)
    etape = train_rnn.encoder_forward(model, _f(mel), torch.from_numpy(np.asarray(lens)), noise_in=noise_in, seed=seed)
    dtape = train_rnn.decoder_forward(model, _f(mel), etape, lens, seed=seed)
    d_enc, d_h, d_c = train_rnn.decoder_backward(dtape, *(_f(x) for x in cots))
    d_mel = train_rnn.encoder_backward(etape, d_enc, d_h, d_c, accumulate=True)
    torch.cuda.synchronize()
    return etape, dtape, (d_enc, d_h, d_c), d_mel


def _grads(model, prefixes=DEC):
    return {k: p.grad.detach().cpu().double() for k, p in model.named_parameters() if k.startswith(prefixes)}


def _fwd_close(name, got, ref, e32, rep):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err, mx = np.abs(got - ref).max(), np.abs(ref).max()
    rep.append("%-44s err %.3g = %.3g of max|ref| = %.1f x e32" % (name, err, err / mx, err / max(e32, 1e-300)))
    print(rep[-1])
    return err <= PARITY * mx


def _check_grads(tag, got, ref, e32s):
    """got / ref: {name: tensor} over parameters and returned cotangents; e32s: {name: e32} for the non-degenerate ones."""
    assert sorted(got) == sorted(ref), sorted(set(got) ^ set(ref))
    bounds, common = RD.grad_bounds(e32s, GRAD_CAP, GRAD_MARGIN)
    errs = {k: TM.normerr(got[k], ref[k]) for k in e32s}
    for k in sorted(errs, key=lambda k: errs[k] / bounds[k])[-4:]:
        print("%s grad %-66s %.3g = %.2f x e32 (own e32 %.2g)" % (tag, k, errs[k], errs[k] / common, e32s[k]))
    worst = max(errs, key=lambda k: errs[k] / bounds[k])
    print("%s: common e32 %.3g, worst gradient %s %.3g = %.2f x e32, %.2f of its bound" % (tag, common, worst, errs[worst], errs[worst] / common,
                                                                                          errs[worst] / bounds[worst]))
    for k in RD.DEGENERATE:
        if got[k[:-4] + "weight"].norm().item() == 0.0:                                          # no gradient reached the post-net at all
            assert got[k].abs().max().item() == 0.0, k
            continue
        rel = got[k].abs().max().item() / got[k[:-4] + "weight"].norm().item()
        print("%s degenerate %s max|g| / ||grad W|| %.2e" % (tag, k, rel))
        assert rel <= DEG_ABS, (k, rel)
    bad = {k: "%.2e > %.2e" % (errs[k], bounds[k]) for k in errs if errs[k] > bounds[k]}
    assert not bad, bad


def _check_forward(tag, model, tape, ref, e32_of, sd):
    rep, ok = [], []
    for k, got in (("pre", tape.pre), ("post", tape.post), ("stop", tape.stop)):
        ok.append(_fwd_close("%s %s" % (tag, k), got.cpu().numpy(), ref[k], e32_of(k), rep))
    for k, v in model.state_dict().items():
        if k.startswith("postnet.") and k.endswith(("running_mean", "running_var")):
            ok.append(_fwd_close("%s %s" % (tag, k), v.cpu().numpy(), ref[k], e32_of(k), rep))
        if k.startswith("postnet.") and k.endswith("num_batches_tracked"):
            assert int(v) == int(sd[k]) + 1
    assert all(ok), "\n".join(rep)


def _np(d):
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()}


# ---- 1. dropout off, against the reference fixtures -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attn", ATTNS)
def test_decoder_alone_matches_the_reference_fixture(attn):
    fx, mir = fixture(attn), mirror_a(attn)
    model, sd = _model(attn)
    tape, (d_enc, d_h, d_c) = _run_a(model, attn)
    assert tape.sites == []
    B, T, M = fx["a_target"].shape
    assert tape.pre.shape == (B, T, M) and tape.post.shape == (B, T, M) and tape.stop.shape == (B, T)
    assert d_enc.shape == (B, 12, 512) and d_h.shape == (2, B, 256) and d_c.shape == (2, B, 256)
    ref = {k[2:]: fx[k] for k in fx if k.startswith("a/") and "/g" not in k}
    _check_forward(attn + " a", model, tape, ref, lambda k: float(fx["e32/a/" + k]), sd)
    for b, n in enumerate(fx["a_lens_k"]):
        assert d_enc[b, int(n):].abs().sum().item() == 0.0, "d_enc_output rows past lens_k must be exactly zero"
    got = _grads(model)
    got.update(d_enc_output=d_enc.cpu().double(), d_h=d_h.cpu().double(), d_c=d_c.cpu().double())
    want = dict(mir["grads"], d_enc_output=mir["d_enc_output"], d_h=mir["d_h"], d_c=mir["d_c"])
    e32s = {k: float(fx["e32/a/grad/" + k]) for k in mir["grads"] if k not in RD.DEGENERATE}
    e32s.update({k: float(fx["e32/a/rel/" + k]) for k in ("d_enc_output", "d_h", "d_c")})
    assert all(got[k].shape == want[k].shape for k in got)
    _check_grads(attn + " a", got, want, e32s)
    assert all(p.grad is None for k, p in model.named_parameters() if not k.startswith(DEC))


@pytest.mark.parametrize("attn", ATTNS)
def test_autoencoder_matches_the_reference_fixture(attn):
    fx, mir = fixture(attn), mirror_b(attn)
    model, sd = _model(attn)
    etape, dtape, _, d_mel = _run_b(model, attn)
    ref = {k[2:]: fx[k] for k in fx if k.startswith("b/") and "/g" not in k}
    _check_forward(attn + " b", model, dtape, ref, lambda k: float(fx["e32/b/" + k]), sd)
    got = _grads(model, ("prenet.", "encoder.", "decoder.", "postnet."))
    got["d_mel"] = d_mel.cpu().double()
    want = dict(mir["grads"], d_mel=mir["d_mel"])
    e32s = {k: float(fx["e32/b/grad/" + k]) for k in mir["grads"] if k not in RD.DEGENERATE}
    e32s["d_mel"] = float(fx["e32/b/rel/d_mel"])
    _check_grads(attn + " b", got, want, e32s)


# ---- 2. dropout 0.5 at every site, against the mirror under the kernels' own masks -------------------------------------------------------------------
def _site_masks(tape):
    masks, streams = {}, set()
    for s in tape.sites:
        epoch = int(s.epoch.item())
        assert s.stream not in streams, "two sites share stream id %d" % s.stream
        streams.add(s.stream)
        if s.kind == "row":
            keep = DM.row_keep(s.seed, s.stream, s.rows, s.p, epoch)
            masks[s.name] = torch.from_numpy(keep.astype(np.float64))
        else:
            keep = DM.keep_mask(s.seed, s.stream, s.rows, s.cols, s.p, epoch)
            masks[s.name] = torch.from_numpy(keep * float(DM.drop_scale(s.p)))
        rate, sdv = keep.mean(), math.sqrt(s.p * (1 - s.p) / keep.size)
        print("site %-18s p %.2f stream %2d [%d,%d]: keep rate %.4f (%.2f sd from 1 - p)" % (s.name, s.p, s.stream, s.rows, s.cols, rate, (rate - (1 - s.p)) / sdv))
        assert abs(rate - (1 - s.p)) <= 4 * sdv, (s.name, rate)
    return masks


DEC_SITES = ["d_prenet_dropout", "d_drop0", "d_dropout1", "post_dropout0", "post_dropout1", "post_dropout2", "post_dropout3"]


@pytest.mark.parametrize("attn", ATTNS)
def test_decoder_alone_with_dropout_matches_the_mirror_under_the_kernels_masks(attn):
    model, sd = _model(attn, drops=0.5)
    tape, (d_enc, d_h, d_c) = _run_a(model, attn, seed=20240)
    assert [s.name for s in tape.sites] == DEC_SITES and all(s.seed == 20240 and s.p == 0.5 for s in tape.sites)
    masks = _site_masks(tape)
    tgt, enc, h, c, lens_k, cots = case_a(attn)
    r64 = RD.run(sd, attn, tgt, enc, h, c, lens_k, cots, masks=masks)
    r32 = RD.run(sd, attn, tgt, enc, h, c, lens_k, cots, masks=masks, dtype=torch.float32)
    fe = lambda k: (r32[k].double() - r64[k]).abs().max().item()                                 # noqa: E731
    _check_forward(attn + " a dropout", model, tape, _np({k: v for k, v in r64.items() if k != "grads"}), fe, sd)
    got = _grads(model)
    got.update(d_enc_output=d_enc.cpu().double(), d_h=d_h.cpu().double(), d_c=d_c.cpu().double())
    want = dict(r64["grads"], d_enc_output=r64["d_enc_output"], d_h=r64["d_h"], d_c=r64["d_c"])
    w32 = dict(r32["grads"], d_enc_output=r32["d_enc_output"], d_h=r32["d_h"], d_c=r32["d_c"])
    e32s = {k: TM.normerr(w32[k], want[k]) for k in want if k not in RD.DEGENERATE}
    _check_grads(attn + " a dropout", got, want, e32s)


@pytest.mark.parametrize("attn", ATTNS)
def test_autoencoder_with_dropout_matches_the_mirror_under_the_kernels_masks(attn):
    model, sd = _model(attn, drops=0.5)
    etape, dtape, _, d_mel = _run_b(model, attn, seed=777)
    assert [s.name for s in etape.sites] == ["dropout2", "e_drop0"] and [s.name for s in dtape.sites] == DEC_SITES
    assert not {s.stream for s in etape.sites} & {s.stream for s in dtape.sites}, "encoder and decoder sites must not share a stream id"
    em, dm = _site_masks(etape), _site_masks(dtape)
    mel, lens, cots = case_b(attn)
    r64 = RD.autoencoder(sd, attn, mel, lens, cots, enc_masks=em, dec_masks=dm)
    r32 = RD.autoencoder(sd, attn, mel, lens, cots, enc_masks=em, dec_masks=dm, dtype=torch.float32)
    fe = lambda k: (r32[k].double() - r64[k]).abs().max().item()                                 # noqa: E731
    _check_forward(attn + " b dropout", model, dtape, _np({k: v for k, v in r64.items() if not k.endswith("grads")}), fe, sd)
    got = _grads(model, ("prenet.", "encoder.", "decoder.", "postnet."))
    got["d_mel"] = d_mel.cpu().double()
    want, w32 = dict(r64["grads"], d_mel=r64["d_mel"]), dict(r32["grads"], d_mel=r32["d_mel"])
    e32s = {k: TM.normerr(w32[k], want[k]) for k in want if k not in RD.DEGENERATE}
    _check_grads(attn + " b dropout", got, want, e32s)


# ---- 3. accumulate, repeatability, .grad in place, a tape's single use --------------------------------------------------------------------------------
@pytest.mark.parametrize("attn", ATTNS)
def test_accumulate_repeat_and_grads_in_place(attn):
    from unast_amd import config, train_rnn
    model, _ = _model(attn)
    params = [p for k, p in model.named_parameters() if k.startswith(DEC)]
    for p in params:
        p.grad = torch.full_like(p, float("nan"))
    ptrs = [p.grad.data_ptr() for p in params]
    saved = config.DETERMINISTIC_SUMS
    config.DETERMINISTIC_SUMS = True                                                             # bias gradients by the fixed-order column sum
    try:
        tape1, out1 = _run_a(model, attn)                                                        # accumulate=False over NaN
        assert [p.grad.data_ptr() for p in params] == ptrs, "an existing dense fp32 .grad must stay in place"
        first = _grads(model)
        assert all(torch.isfinite(g).all() for g in first.values())
        with pytest.raises(RuntimeError, match="used"):
            train_rnn.decoder_backward(tape1)
        tape2, out2 = _run_a(model, attn)
        second = _grads(model)
    finally:
        config.DETERMINISTIC_SUMS = saved
    # two identical calls with the fixed-order column sums on: every output, every returned cotangent and every gradient agree to the bit
    # (the BatchNorm kernels keep fp64 atomics in their statistics; their order moves bits far below fp32 resolution, unast_amd.ops.deterministic_sums,
    # as tests/test_gpu_graph.py holds the whole train step to)
    for name, a, b in zip(("pre", "post", "stop", "d_enc_output", "d_h", "d_c"), (tape1.pre, tape1.post, tape1.stop) + tuple(out1),
                          (tape2.pre, tape2.post, tape2.stop) + tuple(out2)):
        assert torch.equal(a, b), name
    differ = [k for k in first if not torch.equal(first[k], second[k])]
    assert not differ, differ
    _run_a(model, attn, accumulate=True)
    third = _grads(model)
    worst = max(TM.normerr(third[k], 2 * second[k]) for k in second if k not in RD.DEGENERATE)
    print("%s accumulate=True over a first result against twice the first: %.2e" % (attn, worst))
    assert worst <= REPEAT_TOL
    assert all(p.grad is None for k, p in model.named_parameters() if not k.startswith(DEC))
    # cotangents left None are zeros: nothing reaches the gradients or the encoder
    _, out0 = _run_a(model, attn, cot=False)
    assert all(g.abs().max().item() == 0.0 for g in _grads(model).values()) and all(t.abs().max().item() == 0.0 for t in out0)
    # the eval path still answers, from operands rebuilt after the running statistics moved
    tgt, enc, h, c, lens_k, _ = case_a(attn)
    with pytest.raises(NotImplementedError):
        model.decode_sequence(_f(tgt), None, ((_f(h), _f(c)), _f(enc)), None)
    with torch.no_grad():
        mask = torch.arange(enc.shape[1])[None, :] >= torch.from_numpy(np.asarray(lens_k))[:, None]
        pre, _, _, _ = model.eval().decode_sequence(_f(tgt), None, ((_f(h), _f(c)), _f(enc)), mask.to(_dev()))
    assert TM.normerr(pre.cpu(), tape1.pre.cpu()) <= 1e-4                                        # no dropout, and pre does not pass a BatchNorm


# ---- 4. the smallest shapes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attn", ATTNS)
@pytest.mark.parametrize("B,T", [(1, 4), (3, 1), (1, 1)])
def test_single_position_and_single_sequence(attn, B, T):
    from unast_amd import train_rnn
    model, sd = _model(attn, drops=0.5)
    tgt, enc, h, c, lens_k, _ = case_a(attn)
    tgt, enc, h, c = tgt[:B, :T], enc[:B], h[:, :B], c[:, :B]
    lens_k = [7] if B == 1 else list(lens_k)
    if B == 1:
        enc = enc.clone()
        enc[:, 7:] = 0.0
    cots = RD.cotangents(3, B, T, tgt.shape[2])
    if B * T == 1:
        # the post-net's BatchNorm then normalises over two rows (the go frame and one frame): x_hat is +-1 whatever the input, its input
        # gradient is what rounding leaves, and torch's own fp32 run of this case is 1e-2 from its fp64 run -- beyond the 1e-3 cap, so the
        # gradient through `post` is no yardstick here.  The forward is checked in full, the backward from pre and stop only (d_post = None).
        cots = (cots[0], torch.zeros_like(cots[1]), cots[2])
    tape = train_rnn.decoder_forward(model, _f(tgt), ((_f(h), _f(c)), _f(enc)), lens_k, seed=5)
    d_enc, d_h, d_c = train_rnn.decoder_backward(tape, _f(cots[0]), None if B * T == 1 else _f(cots[1]), _f(cots[2]))
    torch.cuda.synchronize()
    masks = _site_masks(tape) if B * T > 1 else {s.name: torch.from_numpy(DM.drop_factor(s.seed, s.stream, s.rows, s.cols, s.p, int(s.epoch.item())))
                                                  for s in tape.sites}
    r64 = RD.run(sd, attn, tgt, enc, h, c, lens_k, cots, masks=masks)
    r32 = RD.run(sd, attn, tgt, enc, h, c, lens_k, cots, masks=masks, dtype=torch.float32)
    for k, got in (("pre", tape.pre), ("post", tape.post), ("stop", tape.stop)):
        assert np.abs(got.cpu().double().numpy() - r64[k].numpy()).max() <= PARITY * max(r64[k].abs().max().item(), 1e-30), k
    got = _grads(model)
    got.update(d_enc_output=d_enc.cpu().double(), d_h=d_h.cpu().double(), d_c=d_c.cpu().double())
    want = dict(r64["grads"], d_enc_output=r64["d_enc_output"], d_h=r64["d_h"], d_c=r64["d_c"])
    w32 = dict(r32["grads"], d_enc_output=r32["d_enc_output"], d_h=r32["d_h"], d_c=r32["d_c"])
    # (one position attends from the given h: the LSTM's recurrent weights of layer 1 see it, nothing is degenerate but the conv biases;
    #  a tensor whose fp64 gradient is exactly zero -- a single live key -- must be exactly zero here as well)
    zero = [k for k in want if k not in RD.DEGENERATE and want[k].abs().max().item() == 0.0]
    assert all(got[k].abs().max().item() == 0.0 for k in zero), zero
    e32s = {k: TM.normerr(w32[k], want[k]) for k in want if k not in RD.DEGENERATE and k not in zero}
    _check_grads("%s B %d T %d" % (attn, B, T), got, want, e32s)
    if B * T == 1:
        # the post-net backward over its two rows all the same: launched, finite, the right shapes, the degenerate conv biases at zero
        full = RD.cotangents(3, B, T, tgt.shape[2])
        tape = train_rnn.decoder_forward(model, _f(tgt), ((_f(h), _f(c)), _f(enc)), lens_k, seed=5)
        outs = train_rnn.decoder_backward(tape, *(_f(x) for x in full))
        torch.cuda.synchronize()
        assert [tuple(t.shape) for t in outs] == [(1, 12, 512), (2, 1, 256), (2, 1, 256)] and all(torch.isfinite(t).all() for t in outs)
        g2 = _grads(model)
        assert all(torch.isfinite(g).all() and g.shape == sd[k].shape for k, g in g2.items())
        assert all(g2[k].abs().max().item() > 0.0 for k in g2 if k.startswith("postnet.") and k.endswith("conv.weight"))
        for k in RD.DEGENERATE:
            assert g2[k].abs().max().item() <= DEG_ABS * g2[k[:-4] + "weight"].norm().item(), k
