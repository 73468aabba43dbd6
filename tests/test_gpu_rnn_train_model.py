"""unast_amd.train_rnn (encoder_forward / encoder_backward of TextRNN and SpeechRNN) on the GPU against the reference's fixture
(tests/golden/rnn_encoder_train.npz) and the fp64 mirror (tests/rnn_train_mirror.py, pinned to that fixture by tests/test_cpu_rnn_train.py).

Bounds: forward tensors 1e-3 x max|ref| (the project's parity bar; the multiples of the reference's own fp32 error are printed); every
parameter gradient and d_mel min(GRAD_CAP, GRAD_MARGIN x e32) in per-tensor relative L2 norm, e32 = the largest fp32-vs-fp64 error of the
reference (dropout off: from the fixture) or of the mirror under the same masks (dropout on) over the non-degenerate gradients, as
tests/test_gpu_vocoder_train.py forms it.  The three conv biases in front of a train-mode BatchNorm have mathematically zero gradients:
max|g| <= 1e-6 x ||grad W|| of their conv, that test's absolute bound."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import dropout_mirror as DM
from tests import rnn_train_mirror as TM
from tests import rnn_weights

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARITY = 1e-3
GRAD_CAP, GRAD_MARGIN = 1e-3, 16.0
DEG_ABS = 1e-6
REPEAT_TOL = 1e-5          # two runs of one backward: fp32 atomics in the column sums and split-K order (tests/test_gpu_vocoder_train.py)
SIDES = ["text", "speech"]


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _fixture(name="rnn_encoder_train"):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def _model(side, attn="luong", drops=0.0, fixture="rnn_encoder_train"):
    from unast_amd.network import TextRNN, SpeechRNN
    args = rnn_weights.rnn_args(attn)
    args.t_pre_drop = args.s_pre_drop = args.e_drop = drops
    m = (TextRNN if side == "text" else SpeechRNN)(args)
    own = m.state_dict()                                      # weights are rebuilt from names: the encoders' are the same under either attention
    meta = rnn_weights.meta_of(_fixture(fixture))
    sd = rnn_weights.state_dict(side, list(own), [list(v.shape) for v in own.values()], meta["seed"], meta["gains"])
    m.load_state_dict(sd)
    return m.to(_dev()).train(), sd


def _inputs(side):
    fx = _fixture()
    xk, lk = ("text", "text_len") if side == "text" else ("mel", "mel_len")
    x = torch.from_numpy(fx[xk])
    return x, fx[lk], TM.cotangents(rnn_weights.meta_of(fx)["cot_seed"], x.shape[0], x.shape[1])


def _run(model, x, lens, cot, **kw):
    from unast_amd import train_rnn
    dev = _dev()
    tape = train_rnn.encoder_forward(model, x.to(dev), torch.from_numpy(np.asarray(lens)), **kw)
    r1, r2, r3 = (t.float().to(dev) for t in cot)
    d_mel = train_rnn.encoder_backward(tape, r1, r2, r3)
    torch.cuda.synchronize()
    return tape, d_mel


def _grads(model):
    return {k: p.grad.detach().cpu().double() for k, p in model.named_parameters() if k.startswith(("prenet.", "encoder."))}


def _fwd_close(name, got, ref, e32, rep):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err, mx = np.abs(got - ref).max(), np.abs(ref).max()
    rep.append("%-34s err %.3g = %.3g of max|ref|%s" % (name, err, err / mx, "" if e32 is None else " = %.1f x e32" % (err / max(e32, 1e-300))))
    print(rep[-1])
    return err <= PARITY * mx


def _check_grads(tag, got, ref, e32, d_mel=None, d_mel_ref=None):
    names = [k for k in ref if k not in TM.DEGENERATE]
    assert sorted(got) == sorted(ref)
    bound = min(GRAD_CAP, GRAD_MARGIN * e32)
    errs = {k: TM.normerr(got[k], ref[k]) for k in names}
    if d_mel is not None:
        errs["d_mel"] = TM.normerr(d_mel, d_mel_ref)
    for k in sorted(errs, key=errs.get)[-4:]:
        print("%s grad %-40s %.3g = %.2f x e32" % (tag, k, errs[k], errs[k] / e32))
    worst = max(errs, key=errs.get)
    print("%s: e32 %.3g, bound %.3g, worst gradient %s %.3g (%.2f x e32)" % (tag, e32, bound, worst, errs[worst], errs[worst] / e32))
    for k in TM.DEGENERATE:
        if k in got:
            rel = got[k].abs().max().item() / got[k[:-4] + "weight"].norm().item()
            print("%s degenerate %s max|g| / ||grad W|| %.2e" % (tag, k, rel))
            assert rel <= DEG_ABS, (k, rel)
    assert errs[worst] <= bound, {k: "%.2e" % e for k, e in errs.items() if e > bound}


# ---- 1. dropout off, against the reference fixture ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
def test_dropout_off_matches_reference_fixture(side):
    fx = _fixture()
    x, lens, cot = _inputs(side)
    model, sd = _model(side)
    tape, d_mel = _run(model, x, lens, cot)
    assert tape.sites == []
    (h, c), eo = tape.hidden, tape.enc_output
    B, T = x.shape[:2]
    assert eo.shape == (B, T, 512) and h.shape == (2, B, 256) and c.shape == (2, B, 256) and tape.pad_mask.dtype == torch.bool
    want_mask = x.eq(0) if side == "text" else torch.arange(T)[None, :] >= torch.from_numpy(lens)[:, None]
    assert torch.equal(tape.pad_mask.cpu(), want_mask)
    for b in range(B):
        assert torch.equal(eo[b, int(lens[b]):], torch.zeros_like(eo[b, int(lens[b]):]))
    rep, ok = [], []
    e = lambda k: float(fx["e32/%s/%s" % (side, k)])                                             # noqa: E731
    ok.append(_fwd_close(side + " h", h.cpu(), fx[side + "/h"], e("h"), rep))
    ok.append(_fwd_close(side + " c", c.cpu(), fx[side + "/c"], e("c"), rep))
    ok.append(_fwd_close(side + " enc_output", TM.sample(eo.cpu().numpy()), fx[side + "/enc_output"], e("enc_output"), rep))
    for k, v in model.state_dict().items():
        if k.startswith("prenet.") and k.endswith(("running_mean", "running_var")):
            ok.append(_fwd_close(side + " " + k, v.cpu(), fx[side + "/" + k], e(k), rep))
        if k.startswith("prenet.") and k.endswith("num_batches_tracked"):
            assert int(v) == int(sd[k]) + 1
    assert all(ok), "\n".join(rep)
    mirror = TM.run(side, sd, x, lens, cot)
    names = [k for k in mirror["grads"] if k not in TM.DEGENERATE]
    e32 = max(float(fx["e32/%s/grad/%s" % (side, k)]) for k in names)
    got = _grads(model)
    assert all(got[k].shape == sd[k].shape for k in got)
    if side == "text":
        assert d_mel is None and got["prenet.embed.weight"][0].abs().max().item() == 0.0          # the padding_idx row
        _check_grads(side, got, mirror["grads"], e32)
    else:
        _check_grads(side, got, mirror["grads"], e32, d_mel.cpu().double(), mirror["d_mel"])
    assert all(p.grad is None for k, p in model.named_parameters() if not k.startswith(("prenet.", "encoder.")))


@pytest.mark.parametrize("side", SIDES)
def test_encoder_does_not_depend_on_the_attention_type(side):
    x, lens, cot = _inputs(side)
    res = []
    for attn in ("luong", "lsa"):
        model, _ = _model(side, attn)
        tape, d_mel = _run(model, x, lens, cot)
        res.append((tape.enc_output, tape.hidden[0], tape.hidden[1], d_mel, model))
    a, b = res
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    # (gradients: equal up to the order of fp32 atomics in the column sums and split-K partials)
    ga, gb = _grads(a[4]), _grads(b[4])
    worst = max(TM.normerr(gb[k], ga[k]) for k in ga if k not in TM.DEGENERATE)
    print("%s luong vs lsa gradients: %.2e" % (side, worst))
    assert worst <= REPEAT_TOL


# ---- 2. dropout and noise on, at the configs' values -----------------------------------------------------------------------------------------
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
        n = keep.size
        rate, sd = keep.mean(), math.sqrt(s.p * (1 - s.p) / n)
        print("site %-12s p %.2f stream %d [%d,%d]: keep rate %.4f (%.2f sd from 1 - p)" % (s.name, s.p, s.stream, s.rows, s.cols, rate, (rate - (1 - s.p)) / sd))
        assert abs(rate - (1 - s.p)) <= 4 * sd, (s.name, rate)
    return masks


@pytest.mark.parametrize("side", SIDES)
def test_dropout_and_noise_on_match_the_mirror_under_the_kernels_masks(side):
    x, lens, cot = _inputs(side)
    model, sd = _model(side, drops=0.5)
    tape, d_mel = _run(model, x, lens, cot, noise_in=True, seed=20240)
    want = {"text": ["emb_dropout", "noise", "dropout1", "dropout2", "dropout3", "e_drop0"], "speech": ["noise", "dropout2", "e_drop0"]}[side]
    assert [s.name for s in tape.sites] == want
    assert all(s.seed == 20240 for s in tape.sites) and all(s.p == (TM.NOISE_P if s.name == "noise" else 0.5) for s in tape.sites)
    masks = _site_masks(tape)
    r64 = TM.run(side, sd, x, lens, cot, masks=masks)
    r32 = TM.run(side, sd, x, lens, cot, masks=masks, dtype=torch.float32)
    rep, ok = [], []
    for k in ("h", "c", "enc_output"):
        got = (tape.hidden[0] if k == "h" else tape.hidden[1] if k == "c" else tape.enc_output).cpu().numpy()
        ok.append(_fwd_close(side + " " + k, got, r64[k].numpy(), (r32[k].double() - r64[k]).abs().max().item(), rep))
    for k, v in model.state_dict().items():
        if k.startswith("prenet.") and k.endswith(("running_mean", "running_var")):
            ok.append(_fwd_close(side + " " + k, v.cpu().numpy(), r64[k].numpy(), (r32[k].double() - r64[k]).abs().max().item(), rep))
    assert all(ok), "\n".join(rep)
    names = [k for k in r64["grads"] if k not in TM.DEGENERATE]
    e32 = max(TM.normerr(r32["grads"][k], r64["grads"][k]) for k in names)
    if side == "text":
        _check_grads(side + " dropout", _grads(model), r64["grads"], e32)
    else:
        _check_grads(side + " dropout", _grads(model), r64["grads"], e32, d_mel.cpu().double(), r64["d_mel"])


# ---- 3. accumulate -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
def test_accumulate_overwrite_and_single_use(side):
    from unast_amd import train_rnn
    x, lens, cot = _inputs(side)
    dev = _dev()
    model, _ = _model(side)
    enc_params = [p for k, p in model.named_parameters() if k.startswith(("prenet.", "encoder."))]
    for p in enc_params:
        p.grad = torch.full_like(p, float("nan"))
    ptrs = [p.grad.data_ptr() for p in enc_params]
    tape, _ = _run(model, x, lens, cot)                                                          # accumulate=False over NaN
    assert [p.grad.data_ptr() for p in enc_params] == ptrs, "an existing dense fp32 .grad must stay in place"
    first = _grads(model)
    assert all(torch.isfinite(g).all() for g in first.values())
    with pytest.raises(RuntimeError):
        train_rnn.encoder_backward(tape, *(t.float().to(dev) for t in cot))
    tape2 = train_rnn.encoder_forward(model, x.to(dev), torch.from_numpy(np.asarray(lens)))
    train_rnn.encoder_backward(tape2, *(t.float().to(dev) for t in cot), accumulate=True)
    torch.cuda.synchronize()
    second = _grads(model)
    worst = max(TM.normerr(second[k], 2 * first[k]) for k in first if k not in TM.DEGENERATE)
    print("%s accumulate=True over a first result against twice the first: %.2e" % (side, worst))
    assert worst <= REPEAT_TOL
    assert all(p.grad is None for k, p in model.named_parameters() if not k.startswith(("prenet.", "encoder.")))
    # a cotangent left None means zero: nothing but d_h reaches the gradients, enc_output's share is gone
    tape3 = train_rnn.encoder_forward(model, x.to(dev), torch.from_numpy(np.asarray(lens)))
    train_rnn.encoder_backward(tape3)
    torch.cuda.synchronize()
    assert all(g.abs().max().item() == 0.0 for g in _grads(model).values())


# ---- 3b. the three operand caches ---------------------------------------------------------------------------------------------------------------
def test_operand_caches_rebuild_on_their_own_tensors_only_and_drop_together():
    """Each of the three packs is cached in its slot of the model's __dict__, keyed on the version counters of its own tensor list: the same
    object until one of those tensors is written in place, untouched by a write outside the list; drop_cached_operands clears every slot."""
    from types import SimpleNamespace
    from unast_amd import rnn, train_rnn, train_rnn_step
    assert rnn.PACK_SLOTS == ("_rnn_pack", "_rnn_train_pack", "_rnn_decoder_train_pack")
    tm, sm = _model("text")[0], _model("speech")[0]
    for m, side, dec_cls, outside in ((tm, "text", train_rnn.TextDecoderPack, tm.postnet.fc1.weight),
                                      (sm, "speech", train_rnn.DecoderPack, sm.postnet.linear_project.weight)):
        caches = (("_rnn_pack", lambda: rnn.pack_of(m, side), m.decoder.linear_projection.linear_layer.bias),
                  ("_rnn_train_pack", lambda: train_rnn.train_pack_of(m, side), m.encoder.reduce_h_W.bias),
                  ("_rnn_decoder_train_pack", lambda: train_rnn.decoder_pack_of(m, dec_cls), next(m.postnet.parameters())))
        for slot, get, own in caches:
            first = get()
            assert get() is first and m.__dict__[slot][1] is first, slot
            with torch.no_grad():
                own.add_(0)
            second = get()
            assert second is not first and get() is second, slot
        enc_pack = train_rnn.train_pack_of(m, side)
        with torch.no_grad():
            outside.add_(0)                                   # a postnet parameter: not in the encoder train pack's list
        assert train_rnn.train_pack_of(m, side) is enc_pack
        assert set(rnn.PACK_SLOTS) <= set(m.__dict__)
    train_rnn_step.drop_cached_operands(SimpleNamespace(text_m=tm, speech_m=sm))
    assert not set(rnn.PACK_SLOTS) & (set(tm.__dict__) | set(sm.__dict__))


# ---- 4. the eval path is untouched -----------------------------------------------------------------------------------------------------------------
def test_eval_encode_after_a_train_call():
    from unast_amd.network import TextRNN
    fx = _fixture("rnn_values_luong")
    dev = _dev()
    x, lens, _ = _inputs("text")
    model, sd = _model("text", fixture="rnn_values_luong")
    text, text_len = torch.from_numpy(fx["text"]).to(dev), torch.from_numpy(fx["text_len"])
    model.eval()
    with torch.no_grad():
        (_, eo0), _ = model.encode(text, text_len)
    err0 = np.abs(eo0.cpu().double().numpy() - fx["text_enc_out"]).max()
    assert err0 <= PARITY * np.abs(fx["text_enc_out"]).max()
    model.train()
    from unast_amd import train_rnn
    train_rnn.encoder_forward(model, x.to(dev), torch.from_numpy(np.asarray(lens)))
    model.eval()
    with torch.no_grad():
        (_, eo1), _ = model.encode(text, text_len)
        assert not torch.equal(eo0, eo1), "the eval operands were not rebuilt after the running statistics moved"
        fresh = TextRNN(rnn_weights.rnn_args("luong"))
        fresh.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
        (_, eo2), _ = fresh.to(dev).eval().encode(text, text_len)
        assert torch.equal(eo1, eo2)
        model.load_state_dict(sd)                                                               # statistics back where the fixture has them
        (_, eo3), _ = model.encode(text, text_len)
    assert torch.equal(eo3, eo0)
    with pytest.raises(NotImplementedError):
        model.train().encode(text, text_len)
    # the speech model has no statistics to move: after a train-mode call its eval encode is still the fixture's
    sm, _ = _model("speech", fixture="rnn_values_luong")
    xs, ls, _ = _inputs("speech")
    train_rnn.encoder_forward(sm, xs.to(dev), torch.from_numpy(np.asarray(ls)))
    with torch.no_grad():
        (_, eo), _ = sm.eval().encode(torch.from_numpy(fx["mel"]).to(dev), torch.from_numpy(fx["mel_len"]))
    assert np.abs(eo.cpu().double().numpy() - fx["speech_enc_out"]).max() <= PARITY * np.abs(fx["speech_enc_out"]).max()
