"""unast_lstm_seq_fwd_train / unast_lstm_seq_bwd (csrc/rnn.hip) against torch's own packed nn.LSTM in fp64 with autograd, on the CPU.

The cases are those of tests/test_gpu_rnn_kernels.py (D = 32 inputs, xproj = x W_ih^T rounded to fp32: the kernel's input).  The kernel's
result is the gradient of that xproj input, which nn.LSTM does not expose at D = 32, so the yardstick LSTM takes xproj itself as its input
through a W_ih that selects each direction's 1024 columns (entries 1 and 0: every product and sum of that contraction is exact in fp64 and in
fp32), with the case's W_hh and biases.  Its input gradient is then d xproj, its weight_hh gradients are dW_hh.  The scalar is
L = <y, R1> + <h_n, R2> + <c_n, R3> with seeded cotangents (R2 = R3 = 0 when the final-state cotangents are absent).

Bound, per tensor and relative to max|ref|: min(GRAD_CAP, GRAD_MARGIN x e32) (tests/test_gpu_vocoder_train.py), e32 = the largest such error
of torch's fp32 nn.LSTM backward against the fp64 one over the case's tensors (one figure per case, as that test forms it).  dW_hh is formed
in fp64 on the host from the kernel's dxproj and hprev.  Measured multiples of e32 are printed.
"""
import functools

import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from tests.test_gpu_rnn_kernels import _lstm_case

pytestmark = pytest.mark.gpu

H = 256
TILE = 16
GRAD_CAP, GRAD_MARGIN = 1e-3, 16.0
NAN = float("nan")


def _dev():
    return torch.device("cuda:0")


def _cotangents(case, finals):
    B, T = case["xproj"].shape[:2]
    ndir = case["whh"].shape[0]
    g = torch.Generator().manual_seed(4242 + 100 * B + 10 * T + ndir)
    r1, r2, r3 = torch.randn(B, T, ndir * H, generator=g), torch.randn(B, ndir * H, generator=g), torch.randn(B, ndir * H, generator=g)
    return r1, (r2 if finals else None), (r3 if finals else None)


def _torch_backward(case, finals, dtype):
    """(d xproj [B,T,ndir*1024], dW_hh [ndir,1024,256]) of torch's packed nn.LSTM in `dtype` (module docstring)."""
    xproj, whh = case["xproj"], case["whh"]
    B, T, _ = xproj.shape
    ndir = whh.shape[0]
    lstm = torch.nn.LSTM(ndir * 4 * H, H, num_layers=1, bidirectional=ndir == 2, batch_first=True).to(dtype)
    sfx = ["", "_reverse"][:ndir]
    with torch.no_grad():
        for d, s in enumerate(sfx):
            sel = torch.zeros(4 * H, ndir * 4 * H, dtype=dtype)
            sel[:, d * 4 * H:(d + 1) * 4 * H] = torch.eye(4 * H, dtype=dtype)
            getattr(lstm, "weight_ih_l0" + s).copy_(sel)
            getattr(lstm, "weight_hh_l0" + s).copy_(whh[d].to(dtype))
            getattr(lstm, "bias_ih_l0" + s).copy_(case["b_ih"][d * 4 * H:(d + 1) * 4 * H].to(dtype))
            getattr(lstm, "bias_hh_l0" + s).copy_(case["b_hh"][d * 4 * H:(d + 1) * 4 * H].to(dtype))
    x = xproj.detach().to(dtype).clone().requires_grad_(True)                                    # a leaf of its own: the case is shared
    out, (hn, cn) = lstm(pack_padded_sequence(x, case["lens"], batch_first=True, enforce_sorted=False))
    y, _ = pad_packed_sequence(out, batch_first=True, total_length=T)
    r1, r2, r3 = _cotangents(case, finals)
    L = (y * r1.to(dtype)).sum()
    if finals:
        L = L + (hn.permute(1, 0, 2).reshape(B, ndir * H) * r2.to(dtype)).sum() + (cn.permute(1, 0, 2).reshape(B, ndir * H) * r3.to(dtype)).sum()
    L.backward()
    dwhh = torch.stack([getattr(lstm, "weight_hh_l0" + s).grad for s in sfx])
    return x.grad.double(), dwhh.double()


def _rel(got, ref):
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


@functools.lru_cache(maxsize=None)
def _reference(B, T, ndir, lens_key, finals):
    """fp64 gradients of the case, and e32: the fp32 nn.LSTM backward's own error against them (computed once per case)."""
    case = _lstm_case(B, T, ndir, lens_key=lens_key)
    d64, w64 = _torch_backward(case, finals, torch.float64)
    d32, w32 = _torch_backward(case, finals, torch.float32)
    return dict(dxproj=d64, dwhh=w64, e32=max(_rel(d32, d64), _rel(w32, w64)))


def _forward_train(case):
    from unast_amd import ops
    dev = _dev()
    xproj = case["xproj"].to(dev)
    B, T, _ = xproj.shape
    ndir = case["whh"].shape[0]
    whh = case["whh"].to(dev)
    full = lambda *s: torch.full(s, NAN, device=dev)                                           # noqa: E731
    y, hn, cn = full(B, T, ndir * H), full(B, ndir * H), full(B, ndir * H)
    saved, hprev = full(B, T, ndir, 5, H), full(B, T, ndir * H)          # saved rows at t >= lens[b] stay NaN: the backward must not read them
    lens = case["lens"].to(dev, torch.int32)
    ops.lstm_seq_fwd_train(xproj, ops.lstm_whh_fragments(whh), case["b_ih"].to(dev), case["b_hh"].to(dev), lens, y, hn, cn, saved, hprev)
    return dict(y=y, hn=hn, cn=cn, saved=saved, hprev=hprev, lens=lens, whh=whh)


def _backward(case, fwd, finals):
    from unast_amd import ops
    dev = _dev()
    B, T, _ = case["xproj"].shape
    ndir = case["whh"].shape[0]
    r1, r2, r3 = _cotangents(case, finals)
    dy = r1.clone()
    for b in range(B):
        dy[b, int(case["lens"][b]):] = NAN                                                      # padding rows of dy are never read
    dxproj = torch.full((B, T, ndir * 4 * H), NAN, device=dev)                                  # the kernel writes every element
    ops.lstm_seq_bwd(dy.to(dev), ops.lstm_whh_fragments_bwd(fwd["whh"]), fwd["saved"], fwd["lens"], dxproj,
                     dhfinal=r2.to(dev) if finals else None, dcfinal=r3.to(dev) if finals else None)
    torch.cuda.synchronize()
    return dxproj


def _check_backward(B, T, ndir, lens_key=None, finals=True):
    case = _lstm_case(B, T, ndir, lens_key=lens_key)
    ref = _reference(B, T, ndir, lens_key, finals)
    fwd = _forward_train(case)
    dxproj = _backward(case, fwd, finals).cpu().double()
    hprev = fwd["hprev"].cpu().double()
    assert torch.isfinite(dxproj).all() and torch.isfinite(hprev).all()
    for b in range(B):
        n = int(case["lens"][b])
        assert torch.equal(dxproj[b, n:], torch.zeros_like(dxproj[b, n:])), "padding rows of dxproj of sequence %d are not exactly zero" % b
        assert torch.equal(hprev[b, n:], torch.zeros_like(hprev[b, n:])), "padding rows of hprev of sequence %d are not exactly zero" % b
    dwhh = torch.stack([dxproj[:, :, d * 4 * H:(d + 1) * 4 * H].reshape(B * T, 4 * H).T @ hprev[:, :, d * H:(d + 1) * H].reshape(B * T, H)
                        for d in range(ndir)])
    bound = min(GRAD_CAP, GRAD_MARGIN * ref["e32"])
    ex, ew = _rel(dxproj, ref["dxproj"]), _rel(dwhh, ref["dwhh"])
    print("lstm_seq_bwd B=%d T=%d ndir=%d finals=%d: dxproj %.3g (%.2f x e32)  dW_hh %.3g (%.2f x e32)  e32 %.3g  bound %.3g"
          % (B, T, ndir, finals, ex, ex / ref["e32"], ew, ew / ref["e32"], ref["e32"], bound))
    assert (ref["dwhh"].abs().max().item() > 0) == (T > 1)                                       # T = 1: h_{t-1} = 0, so dW_hh = 0 on both sides
    assert ex <= bound and ew <= bound, (ex, ew, bound)


# ---- 1. the train forward saves, and changes nothing ------------------------------------------------------------------------------------
def _check_forward_bits(case):
    from unast_amd import ops
    dev = _dev()
    fwd = _forward_train(case)
    B, T, _ = case["xproj"].shape
    ndir = case["whh"].shape[0]
    y, hn, cn = (torch.full(s, NAN, device=dev) for s in ((B, T, ndir * H), (B, ndir * H), (B, ndir * H)))
    ops.lstm_seq_fwd(case["xproj"].to(dev), ops.lstm_whh_fragments(fwd["whh"]), case["b_ih"].to(dev), case["b_hh"].to(dev), fwd["lens"], y, hn, cn)
    torch.cuda.synchronize()
    assert torch.equal(fwd["y"], y) and torch.equal(fwd["hn"], hn) and torch.equal(fwd["cn"], cn)
    # hprev is y one step earlier in the direction's own order; the saved cell state of a sequence's last forward step is cfinal
    yc, hp, saved = y.cpu(), fwd["hprev"].cpu(), fwd["saved"].cpu()
    for b in range(B):
        n = int(case["lens"][b])
        assert torch.equal(hp[b, 1:n, :H], yc[b, :n - 1, :H]) and torch.equal(hp[b, 0, :H], torch.zeros(H))
        assert torch.equal(saved[b, n - 1, 0, 4], cn[b, :H].cpu())
        if ndir == 2:
            assert torch.equal(hp[b, :n - 1, H:], yc[b, 1:n, H:]) and torch.equal(hp[b, n - 1, H:], torch.zeros(H))
            assert torch.equal(saved[b, 0, 1, 4], cn[b, H:].cpu())
        assert torch.isnan(saved[b, n:]).all(), "saved rows at t >= lens[b] are documented as not written"


@pytest.mark.parametrize("ndir", [1, 2])
@pytest.mark.parametrize("T", [1, 9, 64])
@pytest.mark.parametrize("B", [1, 3, TILE + 1])
def test_lstm_seq_fwd_train_is_bit_identical_to_the_eval_forward(B, T, ndir):
    _check_forward_bits(_lstm_case(B, T, ndir))


def test_lstm_seq_fwd_train_bits_past_the_longest_sequence():
    _check_forward_bits(_lstm_case(3, 9, 2, lens_key=(5, 1, 3)))


# ---- 2. / 3. backward against fp64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("finals", [True, False])
@pytest.mark.parametrize("ndir", [1, 2])
@pytest.mark.parametrize("T", [1, 9, 64])
@pytest.mark.parametrize("B", [1, 3, TILE + 1])
def test_lstm_seq_bwd_matches_fp64_autograd(B, T, ndir, finals):
    """B = 17: the second tile holds one live row; T = 1: only the final-state cotangents (and dy) reach the gates; every case with B > 1
    holds a sequence of length 1 inside a longer tile (tests/test_gpu_rnn_kernels.py _lens)."""
    _check_backward(B, T, ndir, finals=finals)


@pytest.mark.parametrize("finals", [True, False])
def test_lstm_seq_bwd_past_the_longest_sequence(finals):
    """max(lens) < T: steps past every sequence of the tile write zero rows and skip the product."""
    _check_backward(3, 9, 2, lens_key=(5, 1, 3), finals=finals)


@pytest.mark.parametrize("ndir", [1, 2])
def test_lstm_seq_bwd_full_tile(ndir):
    """B = 16 exactly: one tile with no padding row."""
    _check_backward(TILE, 9, ndir)


def test_lstm_seq_bwd_t1_final_states_only():
    """T = 1 with dy = 0: the final-state cotangents alone reach the gates."""
    from unast_amd import ops
    case = _lstm_case(3, 1, 2)
    fwd = _forward_train(case)
    dev = _dev()
    _, r2, r3 = _cotangents(case, True)
    dx = torch.full((3, 1, 2 * 4 * H), NAN, device=dev)
    ops.lstm_seq_bwd(torch.zeros(3, 1, 2 * H, device=dev), ops.lstm_whh_fragments_bwd(fwd["whh"]), fwd["saved"], fwd["lens"], dx, dhfinal=r2.to(dev), dcfinal=r3.to(dev))
    dx0 = torch.full((3, 1, 2 * 4 * H), NAN, device=dev)
    ops.lstm_seq_bwd(torch.zeros(3, 1, 2 * H, device=dev), ops.lstm_whh_fragments_bwd(fwd["whh"]), fwd["saved"], fwd["lens"], dx0)
    torch.cuda.synchronize()
    assert torch.equal(dx0, torch.zeros_like(dx0))
    s = fwd["saved"].double()                                                                   # [3,1,2,5,256]
    i, f, g, o, c = (s[:, 0, :, k].reshape(3, 2 * H) for k in range(5))
    tc = torch.tanh(c)
    dct = r3.to(dev).double() + r2.to(dev).double() * o * (1 - tc * tc)
    want = torch.stack([dct * g * i * (1 - i), torch.zeros_like(i), dct * i * (1 - g * g), r2.to(dev).double() * tc * o * (1 - o)], 1)   # [3,4,512]
    want = want.reshape(3, 4, 2, H).permute(0, 2, 1, 3).reshape(3, 1, 2 * 4 * H)
    assert _rel(dx.double(), want) <= 1e-6


# ---- 4. 800 steps ----------------------------------------------------------------------------------------------------------------------------
def test_lstm_seq_bwd_does_not_drift_over_800_steps():
    _check_backward(2, 800, 2, lens_key=(800, 797))


# ---- 5. reproducible ---------------------------------------------------------------------------------------------------------------------------
def test_lstm_seq_bwd_is_reproducible_to_the_bit():
    case = _lstm_case(TILE + 1, 64, 2)
    fwd = _forward_train(case)
    a = _backward(case, fwd, True)
    b = _backward(case, fwd, True)
    assert torch.equal(a, b)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_lstm_seq_train_entry_points_refuse_other_widths_and_shapes():
    from unast_amd import ops
    from unast_amd._lib import lib
    dev = _dev()
    z = lambda *s: torch.zeros(*s, device=dev)                                                  # noqa: E731
    with pytest.raises(ValueError):
        ops.lstm_whh_fragments_bwd(z(1, 512, 128))
    B, T = 2, 3
    lens = torch.tensor([3, 2], dtype=torch.int32, device=dev)
    wf, wt = ops.lstm_whh_fragments(z(2, 1024, 256)), ops.lstm_whh_fragments_bwd(z(2, 1024, 256))
    ok = dict(dy=z(B, T, 512), saved=z(B, T, 2, 5, 256), dxproj=z(B, T, 2048))
    bad = [dict(ok, dy=z(B, T, 256)), dict(ok, saved=z(B, T, 2, 4, 256)), dict(ok, dxproj=z(B, T, 1024)), dict(ok, dxproj=z(B, T, 4096)[:, :, ::2])]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.lstm_seq_bwd(kw["dy"], wt, kw["saved"], lens, kw["dxproj"])
    with pytest.raises(ValueError):
        ops.lstm_seq_bwd(ok["dy"], wf, ok["saved"], lens, ok["dxproj"])                         # the forward's fragment order
    with pytest.raises(ValueError):
        ops.lstm_seq_bwd(ok["dy"], wt, ok["saved"], lens, ok["dxproj"], dhfinal=z(B, 256))
    with pytest.raises(ValueError):
        ops.lstm_seq_fwd_train(z(B, T, 2048), wf, z(2048), z(2048), lens, z(B, T, 512), z(B, 512), z(B, 512), z(B, T, 2, 5, 128), z(B, T, 512))
    with pytest.raises(ValueError):
        ops.lstm_seq_fwd_train(z(B, T, 2048), wf, z(2048), z(2048), lens, z(B, T, 512), z(B, 512), z(B, 512), ok["saved"], z(B, T, 256))
    p = lambda t: t.data_ptr()                                                                  # noqa: E731
    # the C entry points return the package's error code before any launch
    assert lib().unast_lstm_seq_bwd(p(ok["dy"]), None, None, p(wt), p(ok["saved"]), p(lens), p(ok["dxproj"]), B, T, 2, 128, None) < 0
    assert lib().unast_lstm_seq_bwd(p(ok["dy"]), None, None, p(wt), p(ok["saved"]), p(lens), p(ok["dxproj"]), B, T, 3, 256, None) < 0
    assert lib().unast_lstm_seq_fwd_train(p(z(B, T, 2048)), p(wf), p(z(2048)), p(z(2048)), p(lens), p(z(B, T, 512)), p(z(B, 512)), p(z(B, 512)),
                                          p(ok["saved"]), p(z(B, T, 512)), B, T, 2, 128, None) < 0
