"""Dropout and noise sites of the train step against fp64 math under the SAME masks: every kernel's dropped elements are compared with the
host mirror of the mask RNG (tests/dropout_mirror.py) element for element, and its forward / backward with fp64 torch autograd that
multiplies by exactly that mask, at the tolerance of the same entry point's dropout-off test."""

import pytest
import torch

from tests import dropout_mirror as M
from tests import ragged_ref

pytestmark = pytest.mark.gpu
D = torch.device("cuda:0")
SEED = 0x5EED1234


def relerr(a, b):
    b = b.double().cpu()
    return ((a.double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def factor(seed, stream, rows, cols, p, epoch=0):
    return torch.from_numpy(M.drop_factor(seed, stream, rows, cols, p, epoch))


def keep(seed, stream, rows, cols, p, epoch=0):
    return torch.from_numpy(M.keep_mask(seed, stream, rows, cols, p, epoch))


def assert_zero_pattern(got, kp, pre=None):
    """The zeros of a kernel output are exactly the mirror's dropped elements (kp: keep mask), plus, behind a ReLU, the elements whose
    fp64 pre-activation `pre` is <= 0 -- except kept elements within 1e-4 of zero, where fp32 rounding may decide the sign."""
    nz = got.cpu() != 0
    exp = kp.clone()
    sure = torch.ones_like(kp)
    if pre is not None:
        exp &= pre > 0
        sure = ~kp | (pre.abs() > 1e-4)
    assert bool((~nz[~kp]).all()), "an element the mirror drops is nonzero"
    assert torch.equal(nz[sure], exp[sure]), int((nz[sure] != exp[sure]).sum())


# ---- attention ---------------------------------------------------------------------------------------------
def attention_ref(q, k, v, lens_k, causal, H, drop):
    """fp64 attention with dropout on the normalised probabilities (drop: [B, H, Tq, Tk] factor); LSE is that of the undropped scores."""
    o, lse = ragged_ref.attention_ref(q, k, v, lens_k, causal, H, drop)
    return o, lse, None


@pytest.fixture
def fwd_variant_restore():
    from unast_amd._lib import lib
    old = lib().unast_attn_fwd_variant(-1)
    yield lib().unast_attn_fwd_variant
    lib().unast_attn_fwd_variant(old)


@pytest.mark.parametrize("B,Tq,Tk,causal", [(2, 40, 40, True), (3, 150, 37, False), (2, 33, 257, False), (1, 257, 257, True), (2, 96, 96, False)])
def test_attention_dropout_against_fp64(B, Tq, Tk, causal, monkeypatch, fwd_variant_restore):
    """Both forward kernels, fp32 and pre-split operands; the one-pass backward, the two-kernel backward (ATTN_FUSED_BWD = False and the
    fixed-sums mode) and the two-term one-pass form; self-attention with dQ / dK / dV as column slices of one [N, 3E] buffer, cross-attention
    with Tq != Tk, odd Tk and ragged key lengths."""
    from unast_amd import config, ops
    H, E, p, sid = 4, 256, 0.1, 7
    g = torch.Generator().manual_seed(B * 1000 + Tq + Tk)
    self_attn = Tq == Tk
    qkv = torch.randn(B, Tq, 3 * E, generator=g, dtype=torch.float64)
    kvsrc = qkv if self_attn else torch.randn(B, Tk, 3 * E, generator=g, dtype=torch.float64)
    lens = torch.randint(max(1, Tk // 2), Tk + 1, (B,), generator=g)
    lens[0] = Tk
    drop = factor(SEED, sid, B * H * Tq, Tk, p).view(B, H, Tq, Tk)
    q = qkv[..., :E].clone().requires_grad_(True)
    k = kvsrc[..., E:2 * E].clone().requires_grad_(True)
    v = kvsrc[..., 2 * E:].clone().requires_grad_(True)
    o_ref, lse_ref, _ = attention_ref(q, k, v, lens, causal, H, drop)
    do = torch.randn(B, Tq, E, generator=g, dtype=torch.float64)
    o_ref.backward(do)

    qd = qkv.float().to(D).view(B * Tq, 3 * E)
    kd = kvsrc.float().to(D).view(B * Tk, 3 * E)
    dOd = do.float().to(D).view(B * Tq, E)
    lens_d = lens.to(torch.int32).to(D)
    split = {}
    for name, t in (("q", qd), ("k", kd), ("dO", dOd)):
        split[name] = torch.empty_like(t)
        ops.split_f32(t.reshape(-1), split[name].view(-1))
    modes = [("one-pass", True, False, 1), ("two-kernel", False, False, 1), ("fixed-sums", True, True, 1), ("two-term", True, False, 2)]
    for presplit in (False, True):
        Qs, Ks, dOs = (split["q"], split["k"], split["dO"]) if presplit else (qd, kd, dOd)
        Q_, K_, V_ = Qs[:, :E], Ks[:, E:2 * E], Ks[:, 2 * E:]
        for variant in (0, 1):
            fwd_variant_restore(variant)
            O = torch.full((B * Tq, E), float("nan"), device=D)
            LSE = torch.full((B, H, Tq), float("nan"), device=D)
            ops.attn_fwd(Q_, K_, V_, O, LSE, lens_d, B, H, Tq, Tk, causal, drop_p=p, seed=SEED, stream_id=sid, nsplit=3, qkv_split=presplit)
            assert relerr(O.view(B, Tq, E), o_ref.detach()) < 5e-5, (presplit, variant)
            assert relerr(LSE, lse_ref.detach()) < 5e-5, (presplit, variant)
        for name, fused, fixed, terms in modes:
            monkeypatch.setattr(config, "ATTN_FUSED_BWD", fused)
            monkeypatch.setattr(config, "DETERMINISTIC_SUMS", fixed)
            monkeypatch.setattr(config, "ATTN_BWD_TERMS", terms)
            ws = torch.empty(B, H, Tq, device=D)
            if self_attn:
                dqkv = torch.full((B * Tq, 3 * E), float("nan"), device=D)
                dQ, dK, dV = dqkv[:, :E], dqkv[:, E:2 * E], dqkv[:, 2 * E:]
            else:
                dQ = torch.full((B * Tq, E), float("nan"), device=D)
                dkv = torch.full((B * Tk, 2 * E), float("nan"), device=D)
                dK, dV = dkv[:, :E], dkv[:, E:]
            ops.attn_bwd(Q_, K_, V_, O, dOs, LSE, ws, dQ, dK, dV, lens_d, B, H, Tq, Tk, causal, drop_p=p, seed=SEED, stream_id=sid,
                         nsplit=3, qkv_split=presplit)
            for got, ref, what in ((dQ.reshape(B, Tq, E), q.grad, "dQ"), (dK.reshape(B, Tk, E), k.grad, "dK"), (dV.reshape(B, Tk, E), v.grad, "dV")):
                err = relerr(got, ref)
                if terms == 2:          # test_attention_backward_two_term_mode_stays_within_its_bound, now with dropout on
                    nrm = ((got.double().cpu() - ref).norm() / ref.norm()).item()
                    assert err < 4e-3 and nrm < 3e-3, (name, presplit, what, err, nrm)
                else:
                    assert err < 5e-5, (name, presplit, what, err)


@pytest.mark.parametrize("B,Tq,Tk,causal", [(2, 40, 40, True), (3, 150, 37, False), (1, 257, 257, True)])
def test_attention_forward_mask_is_the_mirror(B, Tq, Tk, causal, fwd_variant_restore):
    """Q = 0 makes P uniform over the valid keys; V one-hot over a block of 64 keys then puts keep(q, key) * scale / n_valid(q) into
    output column key % 64 of every head: the kernels' dropped probabilities, read off directly, equal the mirror's mask."""
    from unast_amd import ops
    H, E, p, sid = 4, 256, 0.25, 3
    g = torch.Generator().manual_seed(Tq + Tk)
    lens = torch.randint(max(1, Tk // 2), Tk + 1, (B,), generator=g)
    lens[0] = Tk
    lens_d = lens.to(torch.int32).to(D)
    kp = keep(SEED, sid, B * H * Tq, Tk, p).view(B, H, Tq, Tk)
    valid = (torch.arange(Tk)[None, None, :] < lens[:, None, None]).expand(B, Tq, Tk).clone()
    if causal:
        valid &= torch.arange(Tk)[None, None, :] <= torch.arange(Tq)[None, :, None]
    Q = torch.zeros(B * Tq, E, device=D)
    K = torch.randn(B * Tk, E, generator=g).to(D)
    for variant in (0, 1):
        fwd_variant_restore(variant)
        for k0 in range(0, Tk, 64):
            V = torch.zeros(B, Tk, H, 64)
            for i in range(min(64, Tk - k0)):
                V[:, k0 + i, :, i] = 1.0
            O = torch.empty(B * Tq, E, device=D)
            LSE = torch.empty(B, H, Tq, device=D)
            ops.attn_fwd(Q, K, V.view(B * Tk, E).to(D), O, LSE, lens_d, B, H, Tq, Tk, causal, drop_p=p, seed=SEED, stream_id=sid)
            got = O.cpu().view(B, Tq, H, 64).permute(0, 2, 1, 3)[..., :min(64, Tk - k0)] != 0
            cols = slice(k0, min(Tk, k0 + 64))
            exp = kp[..., cols] & valid[:, None, :, cols]
            assert torch.equal(got, exp), (variant, k0, int((got != exp).sum()))


def test_attention_backward_skips_padded_queries(monkeypatch):
    """lens_q (the encoder's ENC_SKIP_PAD_GRADS path): queries past the length carry a zero dO; the one-pass backward skips their tiles
    and still gives the fp64 gradients under dropout, dQ of the skipped rows zero."""
    from unast_amd import config, ops
    monkeypatch.setattr(config, "ATTN_FUSED_BWD", True)
    monkeypatch.setattr(config, "DETERMINISTIC_SUMS", False)
    B, T, H, E, p, sid = 3, 150, 4, 256, 0.1, 12
    g = torch.Generator().manual_seed(99)
    qkv = torch.randn(B, T, 3 * E, generator=g, dtype=torch.float64)
    lens = torch.tensor([150, 37, 101])
    q = qkv[..., :E].clone().requires_grad_(True); k = qkv[..., E:2 * E].clone().requires_grad_(True); v = qkv[..., 2 * E:].clone().requires_grad_(True)
    drop = factor(SEED, sid, B * H * T, T, p).view(B, H, T, T)
    o_ref, _, _ = attention_ref(q, k, v, lens, False, H, drop)
    do = torch.randn(B, T, E, generator=g, dtype=torch.float64) * (torch.arange(T)[None, :] < lens[:, None])[..., None]
    o_ref.backward(do)
    qd = qkv.float().to(D).view(B * T, 3 * E)
    lens_d = lens.to(torch.int32).to(D)
    O = torch.empty(B * T, E, device=D); LSE = torch.empty(B, H, T, device=D)
    ops.attn_fwd(qd[:, :E], qd[:, E:2 * E], qd[:, 2 * E:], O, LSE, lens_d, B, H, T, T, False, drop_p=p, seed=SEED, stream_id=sid)
    dqkv = torch.full((B * T, 3 * E), float("nan"), device=D)
    ws = torch.empty(B, H, T, device=D)
    ops.attn_bwd(qd[:, :E], qd[:, E:2 * E], qd[:, 2 * E:], O, do.float().to(D).view(B * T, E), LSE, ws, dqkv[:, :E], dqkv[:, E:2 * E],
                 dqkv[:, 2 * E:], lens_d, B, H, T, T, False, drop_p=p, seed=SEED, stream_id=sid, lens_q=lens_d)
    d3 = dqkv.view(B, T, 3 * E)
    for got, ref in ((d3[..., :E], q.grad), (d3[..., E:2 * E], k.grad), (d3[..., 2 * E:], v.grad)):
        assert relerr(got, ref) < 5e-5
    assert bool((d3[1, 37:, :E] == 0).all())


# ---- GEMM and row-panel epilogues --------------------------------------------------------------------------
def _gemm_ref(x, W, b, act, fac):
    y = x.double() @ W.double().t() + b.double()
    if act:
        y = torch.relu(y)
    return y * fac


@pytest.mark.parametrize("M,N,K", [(333, 1024, 256), (257, 81, 256), (70, 46, 256), (129, 256, 80)])
def test_gemm_epilogue_dropout(M, N, K):
    """linear_fwd(act = 1, dropout) through the tile GEMM into a strided column slice, the activation-stationary row panel and the
    32 x 32 panel: dropped elements equal the mirror's (row and column within the output view), values fp64 within 3e-5."""
    from unast_amd import config, ops
    from unast_amd.planes import Planes
    p, sid = 0.3, 4
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g); W = torch.randn(N, K, generator=g) * 0.05; b = torch.randn(N, generator=g) * 0.1 + 0.5
    fac = factor(SEED, sid, M, N, p)
    kp = keep(SEED, sid, M, N, p)
    pre = x.double() @ W.double().t() + b.double()
    ref = _gemm_ref(x, W, b, True, fac)
    xd, Wd, bd = x.to(D), W.to(D), b.to(D)
    ld = (N + 3) // 4 * 4
    wide = torch.full((M, 3 * ld), 5.0, device=D)
    out = wide[:, ld:ld + N]
    ops.linear_fwd(xd, Wd, bd, out, act=1, drop_p=p, seed=SEED, stream_id=sid)
    assert_zero_pattern(out, kp, pre)
    assert relerr(out, ref) < 3e-5
    assert bool((wide[:, :ld] == 5.0).all()) and bool((wide[:, 2 * ld:] == 5.0).all())
    pl = Planes([Wd])
    for rows in ((config.PANEL_ROWS, 2128) if N % 64 == 0 and K == 256 else (config.PANEL_ROWS,)):          # the shipped row panel, the 32 x 32 panel
        y = torch.full((M + 3, ld), 5.0, device=D)
        ops.panel_gemm(xd, pl.ref(0), y[:M], N, bias=bd, act=1, drop_p=p, seed=SEED, stream_id=sid, rows_per_wg=rows)
        torch.cuda.synchronize()
        assert relerr(y[:M, :N], ref) < 3e-5, rows
        assert_zero_pattern(y[:M, :N], kp, pre)
        assert bool((y[M:] == 5.0).all())


@pytest.mark.parametrize("rows", [333, 64, 1000])
def test_gate_bits_and_gated_input_gradient(rows, monkeypatch):
    """The FFN's keep bits: linear1 (act = 1, dropout) writes one bit per hidden element; linear2's input gradient gated by those bits
    and scaled by 1 / (1 - p) equals the one gated by the activation itself (tile GEMM, G > 0) bit for bit, and the fp64 gradient of
    dropout(relu(.)) under the mirror's mask -- through the wrappers the FFN uses (linear_fwd / linear_dgrad with gate_bits, the shipped
    rows per workgroup) and through panel_gemm at 64 and 128 rows per workgroup.  The reference's ReLU gate is the fp64 sign except within
    1e-4 of zero, where the kernel's own fp32 sign decides (one flipped gate would put a whole element of dY W2 into the difference)."""
    from unast_amd import config, ops
    from unast_amd.planes import Planes
    monkeypatch.setattr(config, "PANEL_MIN_ROWS", 1)
    E, F, p, sid = 256, 1024, 0.1, 6
    Mr = rows
    g = torch.Generator().manual_seed(Mr)
    x = torch.randn(Mr, E, generator=g); W1 = torch.randn(F, E, generator=g) * 0.05; b1 = torch.randn(F, generator=g) * 0.1
    W2 = torch.randn(E, F, generator=g) * 0.05; da = torch.randn(Mr, E, generator=g)
    fac = factor(SEED, sid, Mr, F, p)
    kp = fac != 0
    pre = x.double() @ W1.double().t() + b1.double()
    xd, W1d, b1d, W2d, dad = x.to(D), W1.to(D), b1.to(D), W2.to(D), da.to(D)
    p1, p2t = Planes([W1d]), Planes([W2d], transposed=True)

    def planes(w, transposed=False):
        if w.data_ptr() == W1d.data_ptr() and not transposed:
            return p1.ref(0)
        if w.data_ptr() == W2d.data_ptr() and transposed:
            return p2t.ref(0)
        return None
    monkeypatch.setattr(ops, "_weight_planes", planes)
    assert ops.panel_serves(Mr, E, W1d) and ops.panel_serves(Mr, E, W2d, transposed=True)
    gsc = 1.0 / (1.0 - p)
    for rpw in (None, 64, 128):
        h = torch.empty(Mr, F, device=D)
        bits = torch.zeros(ops.gate_bits_bytes(Mr, F), dtype=torch.uint8, device=D)
        du = torch.full((Mr, F), float("nan"), device=D)
        if rpw is None:             # the FFN's calls (functional.ffn_sublayer), config.PANEL_ROWS rows per workgroup
            ops.linear_fwd(xd, W1d, b1d, h, act=1, drop_p=p, seed=SEED, stream_id=sid, gate_bits=bits)
            ops.linear_dgrad(dad, W2d, du, gate_scale=gsc, gate_bits=bits)
        else:
            ops.panel_gemm(xd, p1.ref(0), h, F, bias=b1d, act=1, drop_p=p, seed=SEED, stream_id=sid, rows_per_wg=rpw, gate_bits=bits)
            ops.panel_gemm(dad, p2t.ref(0), du, F, gate_scale=gsc, rows_per_wg=rpw, gate_bits=bits)
        assert_zero_pattern(h, kp, pre)
        relu_on = torch.where(pre.abs() > 1e-4, pre > 0, h.cpu() > 0)
        du_ref = (da.double() @ W2.double()) * relu_on.double() * fac
        assert relerr(du, du_ref) < 3e-5, (rpw, relerr(du, du_ref))
        assert_zero_pattern(du, kp, pre)
        du2 = torch.empty(Mr, F, device=D)
        ops.linear_dgrad(dad, W2d, du2, G=h, gate_scale=gsc)
        assert torch.equal(du, du2), (rpw, float((du - du2).abs().max()))


# ---- residual + LayerNorm ----------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(333, 256), (300, 1024), (65, 768)])
def test_residual_dropout_layernorm_forward_and_both_backwards(M, K, monkeypatch):
    """z = R + dropout(x W^T + b), y = LN(z): the LayerNorm epilogue (tile GEMM + LayerNorm and the row panel, K <= 256 and K-streamed);
    its backward dz = LN'(dy), dz_drop = dropout(dz) by layernorm_bwd and by linear_dgrad_lnbwd (dy = g @ W2 + R2 in one launch):
    one mask in all four, the mirror's; values fp64 within the tolerances of the dropout-off tests."""
    from unast_amd import config, ops
    from unast_amd.planes import Planes
    monkeypatch.setattr(config, "PANEL_MIN_ROWS", 1)
    E, p, sid = 256, 0.1, 9
    g = torch.Generator().manual_seed(M + K)
    x = torch.randn(M, K, generator=g, dtype=torch.float64); W = torch.randn(E, K, generator=g, dtype=torch.float64) * 0.03
    b = torch.randn(E, generator=g, dtype=torch.float64) * 0.1; R = torch.randn(M, E, generator=g, dtype=torch.float64)
    gm = (torch.rand(E, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True); bt = torch.randn(E, generator=g, dtype=torch.float64).requires_grad_(True)
    fac = factor(SEED, sid, M, E, p)
    kp = keep(SEED, sid, M, E, p)
    z_ref = (R + (x @ W.t() + b) * fac).requires_grad_(True)
    y_ref = torch.nn.functional.layer_norm(z_ref, (E,), gm, bt, 1e-5)
    dy = torch.randn(M, E, generator=g, dtype=torch.float64)
    y_ref.backward(dy)
    dzd_ref = z_ref.grad * fac
    xd, Wd, bd, Rd, gmd, btd = (t.detach().float().to(D) for t in (x, W, b, R, gm, bt))
    pl = Planes([Wd])
    for form in ("tile", "panel"):
        z = torch.empty(M, E, device=D); y = torch.empty(M, E, device=D); mean = torch.empty(M, device=D); rstd = torch.empty(M, device=D)
        if form == "tile":
            ops.linear_fwd(xd, Wd, bd, z, drop_p=p, seed=SEED, stream_id=sid, R=Rd, ln=(gmd, btd, y, mean, rstd, 1e-5))
        else:
            ops.panel_gemm(xd, pl.ref(0), z, E, bias=bd, R=Rd, drop_p=p, seed=SEED, stream_id=sid, ln=(gmd, btd, y, mean, rstd, 1e-5))
        torch.cuda.synchronize()
        assert relerr(z, z_ref.detach()) < 3e-5 and relerr(y, y_ref.detach()) < 3e-5, form
        assert torch.equal(z.cpu() == Rd.cpu(), ~kp), form              # a dropped element leaves z = R exactly
    # backward 1: layernorm_bwd on dy (statistics of the fp32 image of z_ref, so that both sides differentiate the same z)
    zd = z_ref.detach().float().to(D)
    ops.layernorm_fwd(zd, gmd, btd, torch.empty(M, E, device=D), mean, rstd, 1e-5)
    dz = torch.empty(M, E, device=D); dzd = torch.empty(M, E, device=D); dg = torch.zeros(E, device=D); db = torch.zeros(E, device=D)
    ops.layernorm_bwd(dy.float().to(D), zd, gmd, mean, rstd, dz, dzd, dg, db, drop_p=p, seed=SEED, stream_id=sid)
    from unast_amd.engine import join_streams
    join_streams(); torch.cuda.synchronize()
    assert relerr(dz, z_ref.grad) < 1e-5 and relerr(dzd, dzd_ref) < 1e-5
    assert relerr(dg, gm.grad) < 1e-5 and relerr(db, bt.grad) < 1e-5
    assert torch.equal(dzd.cpu() != 0, kp)
    # backward 2: the same LayerNorm backward in the epilogue of an input-gradient GEMM (contraction 1024 > 256)
    F = 1024
    G = torch.randn(M, F, generator=g, dtype=torch.float64); W2 = torch.randn(F, E, generator=g, dtype=torch.float64) * 0.03
    R2 = torch.randn(M, E, generator=g, dtype=torch.float64)
    dy2 = G @ W2 + R2
    z2 = z_ref.detach().clone().requires_grad_(True)
    gm2 = gm.detach().clone().requires_grad_(True); bt2 = bt.detach().clone().requires_grad_(True)
    torch.nn.functional.layer_norm(z2, (E,), gm2, bt2, 1e-5).backward(dy2)
    W2d = W2.float().to(D)
    pt = Planes([W2d], transposed=True)
    monkeypatch.setattr(ops, "_weight_planes", lambda w, transposed=False: pt.ref(0) if transposed and w.data_ptr() == W2d.data_ptr() else None)
    dz2 = torch.empty(M, E, device=D); dzd2 = torch.empty(M, E, device=D); dg2 = torch.zeros(E, device=D); db2 = torch.zeros(E, device=D)
    assert ops.linear_dgrad_lnbwd(G.float().to(D), W2d, R2.float().to(D), zd, mean, rstd, gmd, dz2, dzd2, dg2, db2, drop_p=p, seed=SEED, stream_id=sid)
    join_streams(); torch.cuda.synchronize()
    assert relerr(dz2, z2.grad) < 3e-5 and relerr(dzd2, z2.grad * fac) < 3e-5
    assert relerr(dg2, gm2.grad) < 3e-5 and relerr(db2, bt2.grad) < 3e-5
    assert torch.equal(dzd2.cpu() != 0, kp)


# ---- BatchNorm ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("fused_sums", [False, True], ids=["own-sums", "conv-sums"])
def test_batchnorm_dropout_against_fp64(act, fused_sums):
    """dropout(act(BN_train(x))) at p = 0.5, as conv_bn_act runs it: column sums from the producer (have_sums) or the kernel's own,
    backward into a pre-zeroed workspace (ws_zeroed)."""
    from unast_amd import ops
    rows, C, p, sid = 517, 256, 0.5, 11
    g = torch.Generator().manual_seed(2 + act)
    x = (torch.randn(rows, C, generator=g, dtype=torch.float64) * 1.5 + 0.7).requires_grad_(True)
    w = (1 + 0.2 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_(True)
    b = (0.1 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_(True)
    fac = factor(SEED, sid, rows, C, p)
    pre = torch.nn.functional.batch_norm(x, None, None, w, b, True, 0.1, 1e-5)
    y_ref = (torch.relu(pre) if act == 1 else (torch.tanh(pre) if act == 2 else pre)) * fac
    dy = torch.randn(rows, C, generator=g, dtype=torch.float64)
    y_ref.backward(dy)
    xd, wd, bd = x.detach().float().to(D), w.detach().float().to(D), b.detach().float().to(D)
    y = torch.empty(rows, C, device=D); mean = torch.empty(C, device=D); rstd = torch.empty(C, device=D)
    rmd = torch.zeros(C, device=D); rvd = torch.ones(C, device=D)
    ws = torch.zeros(2 * C, dtype=torch.float64, device=D)
    if fused_sums:
        xf = xd.double()
        ws[:C] = xf.sum(0); ws[C:] = (xf * xf).sum(0)
    ops.bn_fwd(xd, wd, bd, y, mean, rstd, rmd, rvd, ws, act, drop_p=p, seed=SEED, stream_id=sid, have_sums=fused_sums)
    assert relerr(y, y_ref.detach()) < 1e-5
    assert_zero_pattern(y, fac != 0, pre.detach() if act == 1 else None)
    dyd = dy.float().to(D).clone(); dx = torch.empty(rows, C, device=D); dg = torch.zeros(C, device=D); db = torch.zeros(C, device=D)
    wsb = torch.zeros(2 * C, dtype=torch.float64, device=D)
    ops.bn_bwd(dyd, xd, mean, rstd, wd, bd, dx, dg, db, wsb, act, drop_p=p, seed=SEED, stream_id=sid, ws_zeroed=True)
    assert relerr(dx, x.grad) < 2e-5
    assert relerr(dg, w.grad) < 2e-5 and relerr(db, b.grad) < 2e-5


# ---- positional encoding, embedding, noise -----------------------------------------------------------------
def test_posenc_dropout_in_a_row_block():
    """posenc_fwd / posenc_bwd with dropout, the output a row block of a larger buffer (the paired encoder call): rows count from the
    block's first row, in both passes; the backward gated by the producing ReLU."""
    from unast_amd import ops
    from unast_amd.portable import positional_table
    B, T, Dm, p, sid = 3, 17, 256, 0.1, 5
    N = B * T
    g = torch.Generator().manual_seed(3)
    pe = torch.from_numpy(positional_table(64, Dm))
    x = torch.randn(N, Dm, generator=g)
    fac = factor(SEED, sid, N, Dm, p)
    ref = (x.double().view(B, T, Dm) * 16.0 + pe.double()[None, :T]).view(N, Dm) * fac
    big = torch.full((3 * N, Dm), 9.0, device=D)
    ops.posenc_fwd(x.to(D), pe.to(D), big[N:2 * N], T, 16.0, drop_p=p, seed=SEED, stream_id=sid)
    assert relerr(big[N:2 * N], ref) < 1e-6
    assert torch.equal(big[N:2 * N].cpu() != 0, fac != 0)
    assert bool((big[:N] == 9.0).all()) and bool((big[2 * N:] == 9.0).all())
    dy = torch.randn(N, Dm, generator=g)
    dbig = torch.zeros(3 * N, Dm, device=D)
    dbig[N:2 * N] = dy.to(D)
    dx = torch.empty(N, Dm, device=D)
    ops.posenc_bwd(dbig[N:2 * N], x.to(D), dx, 16.0, drop_p=p, seed=SEED, stream_id=sid)
    assert relerr(dx, dy.double() * 16.0 * fac * (x > 0).double()) < 1e-6


@pytest.mark.parametrize("shift_sos", [-1, 1])
@pytest.mark.parametrize("fixed", [False, True], ids=["atomics", "fixed-sums"])
def test_embedding_dropout_and_noise(shift_sos, fixed, monkeypatch):
    """embed_fwd / embed_bwd (both gradient kernels) with dropout and noise_fn's row mask: out = E[id] * mask / (1 - p) * keep_row, the
    gradient its exact adjoint (padding row 0 excluded)."""
    from unast_amd import config, ops
    monkeypatch.setattr(config, "DETERMINISTIC_SUMS", fixed)
    B, T, V, Dm, p, pn, sid, sn = 3, 40, 46, 256, 0.1, 0.3, 2, 3
    N = B * T
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, V, (B, T), generator=g)
    E = torch.randn(V, Dm, generator=g)
    src = ids if shift_sos < 0 else torch.cat([torch.full((B, 1), shift_sos, dtype=torch.long), ids[:, :-1]], 1)
    fac = factor(SEED, sid, N, Dm, p) * torch.from_numpy(M.row_keep(SEED, sn, N, pn)).double()[:, None]
    out = torch.empty(N, Dm, device=D)
    ops.embed_fwd(ids.to(D), E.to(D), out, T, shift_sos=shift_sos, drop_p=p, seed=SEED, stream_id=sid, noise_p=pn, noise_stream=sn)
    ref = E.double()[src.view(-1)] * fac
    assert relerr(out, ref) < 1e-6 and torch.equal(out.cpu() != 0, fac != 0)
    dout = torch.randn(N, Dm, generator=g)
    dE = torch.zeros(V, Dm, device=D)
    ops.embed_bwd(ids.to(D), dout.to(D), dE, T, shift_sos=shift_sos, drop_p=p, seed=SEED, stream_id=sid, noise_p=pn, noise_stream=sn)
    dref = torch.zeros(V, Dm, dtype=torch.float64).index_add_(0, src.view(-1), dout.double() * fac)
    dref[0] = 0
    assert relerr(dE, dref) < 1e-6


def test_rowmask_is_the_mirror_row_mask():
    from unast_amd import ops
    rows, Dm, p, sid = 4099, 80, 0.3, 2
    x = torch.randn(rows, Dm).to(D) + 10.0
    y = torch.empty_like(x)
    ops.rowmask(x, y, p, SEED, sid)
    kr = torch.from_numpy(M.row_keep(SEED, sid, rows, p))
    assert torch.equal(y.cpu(), x.cpu() * kr[:, None].float())


@pytest.mark.parametrize("slope", [1.0, 0.2])
def test_leaky_dropout_forward_and_backward(slope):
    from unast_amd import ops
    rows, Dm, p, sid = 300, 81, 0.5, 8           # D odd: the column index runs across float4 boundaries
    g = torch.Generator().manual_seed(8)
    x = torch.randn(rows, Dm, generator=g); dy = torch.randn(rows, Dm, generator=g)
    fac = factor(SEED, sid, rows, Dm, p)
    y = torch.empty(rows, Dm, device=D)
    ops.leaky_dropout(x.to(D), None, y, slope, drop_p=p, seed=SEED, stream_id=sid)
    assert relerr(y, torch.nn.functional.leaky_relu(x.double(), slope) * fac) < 1e-6 and torch.equal(y.cpu() != 0, fac != 0)
    dx = torch.empty(rows, Dm, device=D)
    ops.leaky_dropout(x.to(D), dy.to(D), dx, slope, drop_p=p, seed=SEED, stream_id=sid)
    assert relerr(dx, dy.double() * torch.where(x > 0, 1.0, slope).double() * fac) < 1e-6


# ---- decoding kernels at a nonzero RNG epoch ----------------------------------------------------------------
@pytest.fixture
def rng_epoch():
    from unast_amd import ops
    ctr = ops.rng_epoch_counter()
    ctr.fill_(5)
    torch.cuda.synchronize()
    yield 5
    ctr.fill_(0)
    torch.cuda.synchronize()


def test_decode_kernels_draw_the_mirror_masks_at_the_epoch(rng_epoch):
    from unast_amd import ops
    B, H, Tcap, p, sid = 5, 4, 37, 0.25, 2
    E = 64 * H
    g = torch.Generator().manual_seed(7)
    q = torch.randn(B, E, generator=g); kv = torch.randn(B, Tcap, 2 * E, generator=g)
    lens = torch.tensor([37, 1, 20, 36, 9], dtype=torch.int32)
    O = torch.zeros(B, E, device=D)
    kvd = kv.to(D).view(B * Tcap, 2 * E)
    ops.decode_attn(q.to(D), kvd[:, :E], kvd[:, E:], Tcap, O, H, lens=lens.to(D), drop_p=p, seed=SEED, stream_id=sid)
    fac = factor(SEED, sid, B * H, Tcap, p, epoch=rng_epoch).view(B, H, Tcap)
    ref = torch.zeros(B, E, dtype=torch.float64)
    for b in range(B):
        n = int(lens[b])
        for h in range(H):
            s = kv[b, :n, 64 * h:64 * h + 64].double() @ q[b, 64 * h:64 * h + 64].double() / 8.0
            ref[b, 64 * h:64 * h + 64] = (torch.softmax(s, 0) * fac[b, h, :n]) @ kv[b, :n, E + 64 * h:E + 64 * h + 64].double()
    assert relerr(O, ref) < 3e-5
    M_, N, K = 33, 81, 256
    x = torch.randn(M_, K, generator=g); W = torch.randn(N, K, generator=g) * 0.1; b = torch.randn(N, generator=g)
    R = torch.zeros(M_, 84); R[:, :N] = torch.randn(M_, N, generator=g)
    y = torch.zeros(M_, 84, device=D)
    ops.decode_linear(x.to(D), W.to(D), b.to(D), y, act=1, drop_p=p, seed=SEED, stream_id=sid + 1, R=R.to(D))
    torch.cuda.synchronize()
    fl = factor(SEED, sid + 1, M_, N, p, epoch=rng_epoch)
    pre = torch.relu(x.double() @ W.double().t() + b.double())
    assert relerr(y[:, :N], pre * fl + R[:, :N].double()) < 3e-5
    assert_zero_pattern(y[:, :N].cpu() - R[:, :N], fl != 0, x.double() @ W.double().t() + b.double())


def test_decode_linear_prologue_dropouts_at_the_epoch(rng_epoch):
    """The rows decode_linear produces in its prologue (xn_out): LayerNorm + dropout, embedding dropout + positional encoding + dropout,
    positional encoding + dropout -- row = sequence m, col = input feature k, RNG epoch mixed in -- against fp64 math under the mirror's
    masks; the contraction of those rows against fp64 as well."""
    from unast_amd import ops
    B, K, N, T, V, p, sc = 7, 256, 96, 12, 46, 0.2, 16.0
    g = torch.Generator().manual_seed(21)
    W, b = torch.randn(N, K, generator=g) * 0.1, torch.randn(N, generator=g)
    Wd, bd = W.to(D), b.to(D)
    pos = torch.tensor([5], dtype=torch.int64, device=D)
    pe = torch.randn(40, K, generator=g)
    # LayerNorm + dropout
    z = torch.randn(B, K, generator=g) * 2 + .5
    gam, bet = torch.rand(K, generator=g) + .5, torch.randn(K, generator=g)
    f1 = factor(SEED, 8, B, K, p, epoch=rng_epoch)
    ref = torch.nn.functional.layer_norm(z.double(), (K,), gam.double(), bet.double(), 1e-5) * f1
    y, xn = torch.zeros(B, N, device=D), torch.zeros(B, K, device=D)
    ops.decode_linear(z.to(D), Wd, bd, y, ln=(gam.to(D), bet.to(D)), ln_drop=(p, 8), xn_out=xn, seed=SEED)
    torch.cuda.synchronize()
    assert relerr(xn, ref) < 1e-5 and torch.equal(xn.cpu() != 0, f1 != 0)
    assert relerr(y, ref @ W.double().t() + b.double()) < 3e-5
    # embedding: dropout(dropout(E[token]) * scale + pe[pos])
    tokens = torch.randint(0, V, (B, T), generator=g)
    emb = torch.randn(V, K, generator=g)
    fa, fb = factor(SEED, 3, B, K, p, epoch=rng_epoch), factor(SEED, 4, B, K, p, epoch=rng_epoch)
    ref = (emb.double()[tokens[:, 5]] * fa * sc + pe.double()[5]) * fb
    y, xn = torch.zeros(B, N, device=D), torch.zeros(B, K, device=D)
    ops.decode_linear(None, Wd, bd, y, embed=(tokens.to(D), emb.to(D), pe.to(D), sc, (p, 3), (p, 4)), xn_out=xn, seed=SEED, pos=pos)
    torch.cuda.synchronize()
    assert relerr(xn, ref) < 1e-6 and torch.equal(xn.cpu() != 0, fb != 0)
    assert relerr(y, ref @ W.double().t() + b.double()) < 3e-5
    # positional encoding of given rows
    frames = torch.randn(B, K, generator=g)
    fc = factor(SEED, 6, B, K, p, epoch=rng_epoch)
    ref = (frames.double() * sc + pe.double()[5]) * fc
    y, xn = torch.zeros(B, N, device=D), torch.zeros(B, K, device=D)
    ops.decode_linear(frames.to(D), Wd, bd, y, posenc=(pe.to(D), sc, (p, 6)), xn_out=xn, seed=SEED, pos=pos)
    torch.cuda.synchronize()
    assert relerr(xn, ref) < 1e-6 and torch.equal(xn.cpu() != 0, fc != 0)
    assert relerr(y, ref @ W.double().t() + b.double()) < 3e-5
