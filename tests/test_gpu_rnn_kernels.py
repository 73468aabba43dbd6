"""csrc/rnn.hip against fp64 references: unast_lstm_seq_fwd against torch's own packed nn.LSTM, unast_rnn_attn_step against the mirror's
step function (tests/rnn_mirror.py), unast_lstm_cell / unast_tanh_rows against the formulas.  Hidden 256, as the kernels are built."""
import functools

import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from tests import rnn_mirror as M

pytestmark = pytest.mark.gpu

H = 256
TILE = 16                                  # sequences per workgroup of lstm_seq_fwd
Y_TOL, STATE_TOL = 2e-5, 5e-5              # tests/test_gpu_lstm128.py: FWD_TOL on y, BWD_TOL on the final states (absolute, O(1) values)
ATTN_TOL = 1e-5                            # x max|ref|: the bound tests/test_gpu_decode.py applies to decode_attn


def _dev():
    return torch.device("cuda:0")


def _lens(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = T
    if B > 1:
        lens[-1] = 1
    return lens


@functools.lru_cache(maxsize=None)
def _lstm_case(B, T, ndir, lens_key=None, seed=0):
    """Inputs and the fp64 packed nn.LSTM results of one case (computed once per case)."""
    torch.manual_seed(1000 * seed + 100 * B + 10 * T + ndir)
    D = 32
    lstm = torch.nn.LSTM(D, H, num_layers=1, bidirectional=ndir == 2, batch_first=True)      # fp32 values, so the fp64 copy is exact
    x = torch.randn(B, T, D)
    lens = torch.tensor(lens_key) if lens_key is not None else _lens(B, T, seed + B + T)
    ref = torch.nn.LSTM(D, H, num_layers=1, bidirectional=ndir == 2, batch_first=True).double()
    ref.load_state_dict({k: v.double() for k, v in lstm.state_dict().items()})
    with torch.no_grad():
        out, (hn, cn) = ref(pack_padded_sequence(x.double(), lens, batch_first=True, enforce_sorted=False))
        y, _ = pad_packed_sequence(out, batch_first=True, total_length=T)
    sfx = ["", "_reverse"][:ndir]
    w_ih = torch.cat([getattr(lstm, "weight_ih_l0" + s) for s in sfx]).detach()
    xproj = (x.double() @ w_ih.double().T).float()                                             # [B,T,ndir*4H]: the kernel's input
    whh = torch.stack([getattr(lstm, "weight_hh_l0" + s) for s in sfx]).detach()
    b_ih = torch.cat([getattr(lstm, "bias_ih_l0" + s) for s in sfx]).detach()
    b_hh = torch.cat([getattr(lstm, "bias_hh_l0" + s) for s in sfx]).detach()
    return dict(xproj=xproj, whh=whh, b_ih=b_ih, b_hh=b_hh, lens=lens, y=y, hn=hn.permute(1, 0, 2).reshape(B, ndir * H),
                cn=cn.permute(1, 0, 2).reshape(B, ndir * H))


def _run_lstm(case):
    from unast_amd import ops
    dev = _dev()
    xproj = case["xproj"].to(dev)
    B, T, _ = xproj.shape
    ndir = case["whh"].shape[0]
    wfrag = ops.lstm_whh_fragments(case["whh"].to(dev))
    y = torch.full((B, T, ndir * H), float("nan"), device=dev)                                  # the kernel writes every element
    hn, cn = torch.full((B, ndir * H), float("nan"), device=dev), torch.full((B, ndir * H), float("nan"), device=dev)
    ops.lstm_seq_fwd(xproj, wfrag, case["b_ih"].to(dev), case["b_hh"].to(dev), case["lens"].to(dev, torch.int32), y, hn, cn)
    torch.cuda.synchronize()
    return y.cpu().double(), hn.cpu().double(), cn.cpu().double()


def _check_lstm(case):
    y, hn, cn = _run_lstm(case)
    B, T = y.shape[:2]
    ey, eh, ec = (y - case["y"]).abs().max().item(), (hn - case["hn"]).abs().max().item(), (cn - case["cn"]).abs().max().item()
    print("lstm_seq_fwd B=%d T=%d ndir=%d: |dy|=%.3g |dh_n|=%.3g |dc_n|=%.3g" % (B, T, case["whh"].shape[0], ey, eh, ec))
    for b in range(B):
        assert torch.equal(y[b, int(case["lens"][b]):], torch.zeros_like(y[b, int(case["lens"][b]):])), "padding rows of sequence %d are not exactly zero" % b
    assert ey <= Y_TOL and eh <= STATE_TOL and ec <= STATE_TOL, (ey, eh, ec)


@pytest.mark.parametrize("ndir", [1, 2])
@pytest.mark.parametrize("T", [1, 9, 64])
@pytest.mark.parametrize("B", [1, 3, TILE + 1])
def test_lstm_seq_fwd_matches_torch_packed_lstm(B, T, ndir):
    _check_lstm(_lstm_case(B, T, ndir))


def test_lstm_seq_fwd_pads_past_the_longest_sequence():
    """max(lens) < T: the steps past every sequence of the tile write zeros and leave the states alone."""
    _check_lstm(_lstm_case(3, 9, 2, lens_key=(5, 1, 3)))


def test_lstm_seq_fwd_does_not_drift_over_800_steps():
    _check_lstm(_lstm_case(2, 800, 2, lens_key=(800, 797)))


def test_lstm_seq_fwd_refuses_other_widths():
    from unast_amd import ops
    dev = _dev()
    with pytest.raises(ValueError):
        ops.lstm_whh_fragments(torch.zeros(1, 512, 128, device=dev))


# ---- attention ------------------------------------------------------------------------------------------------------------------------
def _attn_inputs(B, Tk, A, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale)       # noqa: E731
    lens = [Tk, 1, max(1, Tk // 2)][:B]
    return dict(Wq=r(A, H, scale=0.1), mem=r(B, Tk, A), v=r(A), enc=r(B, Tk, 512), lens=lens,
                conv_w=r(32, 2, 31, scale=0.3), dense_w=r(A, 32, scale=0.3), hs=[r(B, H) for _ in range(5)])


# key counts around the conv's half width (15) and width (31), one past the 256 threads of a workgroup; the other widths at two of them
_ATTN_SHAPES = [(Tk, 32) for Tk in (1, 15, 16, 31, 32, 47, 300)] + [(31, 64), (300, 64), (31, 4), (300, 4)]


@pytest.mark.parametrize("Tk,A", _ATTN_SHAPES)
@pytest.mark.parametrize("mode", ["luong", "lsa"])
def test_rnn_attn_step_matches_the_mirror(mode, Tk, A):
    from unast_amd import ops
    dev = _dev()
    B = 3
    p = _attn_inputs(B, Tk, A, seed=7 * Tk + A)
    d = {k: v.to(dev) for k, v in p.items() if torch.is_tensor(v)}
    lens_d = torch.tensor(p["lens"], dtype=torch.int32, device=dev)
    prev_d, cum_d = torch.zeros(B, Tk, device=dev), torch.zeros(B, Tk, device=dev)
    prev, cum = torch.zeros(B, Tk, dtype=M.F64), torch.zeros(B, Tk, dtype=M.F64)
    f64 = {k: v.double() for k, v in p.items() if torch.is_tensor(v)}
    steps = 5 if mode == "lsa" else 2
    for i in range(steps):
        h = p["hs"][i]
        ctx_d = torch.full((B, 512), float("nan"), device=dev)
        if mode == "lsa":
            ops.rnn_attn_step(ops.ATTN_LSA, h.to(dev), d["Wq"], d["mem"], d["v"], d["enc"], lens_d, ctx_d, prev=prev_d, cum=cum_d,
                              conv_w=d["conv_w"], dense_w=d["dense_w"])
        else:
            prev_d.fill_(float("nan"))
            ops.rnn_attn_step(ops.ATTN_LUONG, h.to(dev), d["Wq"], d["mem"], d["v"], d["enc"], lens_d, ctx_d, prev=prev_d)
        torch.cuda.synchronize()
        ctx, w, cum_new = M.attn_step(mode, h.double(), f64["Wq"], f64["mem"], f64["v"], f64["enc"], p["lens"], prev, cum, f64["conv_w"], f64["dense_w"])
        got_w, got_ctx = prev_d.cpu().double(), ctx_d.cpu().double()
        ew, ec = (got_w - w).abs().max().item(), (got_ctx - ctx).abs().max().item()
        print("rnn_attn_step %s Tk=%d A=%d step %d: |dw|=%.3g of %.3g, |dctx|=%.3g of %.3g" % (mode, Tk, A, i, ew, w.abs().max(), ec, ctx.abs().max()))
        for b in range(B):
            assert torch.equal(got_w[b, p["lens"][b]:], torch.zeros(Tk - p["lens"][b], dtype=M.F64)), "masked weights must be exactly zero"
        assert (got_w.sum(1) - 1).abs().max().item() <= 1e-6
        assert ew <= ATTN_TOL * w.abs().max().item() and ec <= ATTN_TOL * ctx.abs().max().item()
        if mode == "lsa":
            ecum = (cum_d.cpu().double() - cum_new).abs().max().item()
            assert ecum <= ATTN_TOL * cum_new.abs().max().item(), ecum
            prev, cum = w, cum_new


def test_rnn_attn_step_validates_its_arguments():
    from unast_amd import ops
    dev = _dev()
    z = lambda *s: torch.zeros(*s, device=dev)                                 # noqa: E731
    lens = torch.ones(2, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):                                            # attn_dim not a multiple of 4
        ops.rnn_attn_step(ops.ATTN_LUONG, z(2, H), z(6, H), z(2, 8, 6), z(6), z(2, 8, 512), lens, z(2, 512))
    with pytest.raises(ValueError):                                            # LSA without its state
        ops.rnn_attn_step(ops.ATTN_LSA, z(2, H), z(8, H), z(2, 8, 8), z(8), z(2, 8, 512), lens, z(2, 512))
    with pytest.raises(ValueError):                                            # encoder width
        ops.rnn_attn_step(ops.ATTN_LUONG, z(2, H), z(8, H), z(2, 8, 8), z(8), z(2, 8, 256), lens, z(2, 512))


# ---- cell update ----------------------------------------------------------------------------------------------------------------------
def test_lstm_cell_and_tanh_rows_match_the_formulas():
    """Bound: sigmoid / tanh / two products and a sum on O(1) fp32 values -- a few fp32 roundings (6e-8 each), taken as 1e-6 absolute."""
    from unast_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    B = 3
    gates, c = torch.randn(B, 4 * H, generator=g) * 2, torch.randn(B, H, generator=g)
    buf = torch.zeros(B, 4 * H + 8, device=dev)                                # gates as a column slice of a wider buffer
    buf[:, :4 * H] = gates.to(dev)
    c_d, h_d = c.to(dev), torch.full((B, H), float("nan"), device=dev)
    ops.lstm_cell(buf[:, :4 * H], c_d, h_d)
    h_ref, c_ref = M.lstm_cell(gates.double(), c.double())
    assert (h_d.cpu().double() - h_ref).abs().max().item() <= 1e-6
    assert (c_d.cpu().double() - c_ref).abs().max().item() <= 1e-6
    x = torch.randn(B, 300, generator=g) * 3
    x_d = torch.zeros(B, 304, device=dev)
    x_d[:, :300] = x.to(dev)
    ops.tanh_rows(x_d[:, :300])
    assert (x_d[:, :300].cpu().double() - torch.tanh(x.double())).abs().max().item() <= 1e-6
    assert torch.equal(x_d[:, 300:].cpu(), torch.zeros(B, 4))


# ---- the step's fp32 contraction ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(1, 46, 256), (3, 81, 256), (3, 1024, 768), (33, 1024, 256), (3, 256, 512), (2, 256, 80), (3, 8, 1024)])
def test_rnn_linear_keeps_fp32_products(M, N, K):
    """Y = act(X W^T + bias + R) against fp64.  Bound per element: a lane adds K/64 products, six reduction levels follow, bias and R two more
    roundings -- at most K/64 + 8 <= 24 roundings of 2^-24 relative to sum |x_k w_k| + |bias| + |R|; taken as 32 x 2^-24 of that sum.
    (The split-bf16 contraction it stands in for is at 2^-17.)  Also: rows as a column slice of a wider buffer, rows at a device-resident position."""
    from unast_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(M * 7 + N + K)
    X, W, b, R = torch.randn(M, K + 8, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    Xd, Wd, bd, Rd = X.to(dev), W.to(dev), b.to(dev), R.to(dev)
    x64, mag = X[:, :K].double(), X[:, :K].double().abs() @ W.double().abs().T
    tol = 32 * 2.0 ** -24
    Y = torch.full((M, N + 3), float("nan"), device=dev)
    ops.rnn_linear(Xd[:, :K], Wd, bd, Y, R=Rd)
    ref = x64 @ W.double().T + b.double() + R.double()
    assert ((Y[:, :N].cpu().double() - ref).abs() <= tol * (mag + b.double().abs() + R.double().abs())).all()
    assert torch.isnan(Y[:, N:]).all()
    ops.rnn_linear(Xd[:, :K], Wd, None, Y, act=1)
    ref = torch.relu(x64 @ W.double().T)
    assert ((Y[:, :N].cpu().double() - ref).abs() <= tol * mag).all()
    # rows taken from / written to position 2 of [M, 4, .] buffers
    pos = torch.tensor([2], dtype=torch.int64, device=dev)
    xf = torch.randn(M, 4, K, generator=g).to(dev)
    yf = torch.zeros(M, 4, N + 2, device=dev)
    ops.rnn_linear(None, Wd, bd, None, pos=pos, x_frames=xf, y_frames=yf)
    ref = xf[:, 2].cpu().double() @ W.double().T + b.double()
    mag2 = xf[:, 2].cpu().double().abs() @ W.double().abs().T + b.double().abs()
    assert ((yf[:, 2, :N].cpu().double() - ref).abs() <= tol * mag2).all()
    assert torch.equal(yf[:, [0, 1, 3]].cpu(), torch.zeros(M, 3, N + 2)) and torch.equal(yf[:, 2, N:].cpu(), torch.zeros(M, 2))


def test_rnn_linear_refuses_long_rows():
    from unast_amd import ops
    dev = _dev()
    with pytest.raises(ValueError):
        ops.rnn_linear(torch.zeros(2, 1280, device=dev), torch.zeros(8, 1280, device=dev), None, torch.zeros(2, 8, device=dev))
