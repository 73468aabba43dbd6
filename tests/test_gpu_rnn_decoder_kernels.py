"""The kernels of SpeechRNN decoder training (csrc/rnn.hip: unast_rnn_attn_step_train, unast_rnn_attn_step_bwd, unast_lstm_cell_train,
unast_lstm_cell_bwd, unast_tanh_bwd) against fp64 autograd of the same step and against the eval kernels' bits.

Gradient bound: min(1e-3, 16 x e32) in per-tensor relative L2 norm, e32 = the error of torch's fp32 CPU run of the same case against its fp64
run (the largest over the case's tensors, floored at fp32's 2^-24: a lucky fp32 run is no yardstick); each worst case is printed as a
multiple of e32."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F = torch.nn.functional
CAP, MARGIN, EPS32 = 1e-3, 16.0, 2.0 ** -24


def _dev():
    return torch.device("cuda:0")


def _g(t):
    return None if t is None else t.float().to(_dev()).contiguous()


def attn_ref(mode, h, Wq, mem, v, enc, lens, prev, cum, conv_w, dense_w):
    """One attention step for one sequence batch, torch ops in the operands' dtype (src/module.py:421-497).  v, conv_w, dense_w carry a
    leading batch dimension so that autograd yields the per-sequence partial sums."""
    B, Tk, A = mem.shape
    pq = torch.einsum("bk,ak->ba", h, Wq)
    pq.retain_grad()
    x = pq[:, None, :] + mem
    if mode == 1:
        loc = torch.stack([F.conv1d(torch.stack([prev[b], cum[b]])[None], conv_w[b], padding=15)[0].t() @ dense_w[b].t() for b in range(B)])
        x = x + loc
    e = torch.einsum("bta,ba->bt", torch.tanh(x), v)
    pad = torch.arange(Tk)[None, :] >= torch.as_tensor(lens)[:, None]
    w = torch.softmax(e.masked_fill(pad, float("-inf")), 1)
    return torch.bmm(w[:, None], enc)[:, 0], w, pq


def _case(mode, B, Tk, A, lens, seed):
    r = np.random.RandomState(seed)
    t = lambda *s, sc=1.0: torch.from_numpy(r.standard_normal(s) * sc)                           # noqa: E731
    d = dict(h=t(B, 256, sc=0.5), Wq=t(A, 256, sc=0.1), mem=t(B, Tk, A, sc=0.5), v=t(A, sc=0.7), enc=t(B, Tk, 512, sc=0.5),
             dctx=t(B, 512), dwa=t(B, Tk), dwb=t(B, Tk, sc=0.5))
    if mode == 1:
        prev = torch.softmax(t(B, Tk), 1)
        d.update(prev=prev, cum=prev * 2.5 + torch.softmax(t(B, Tk), 1), conv_w=t(32, 2, 31, sc=0.2), dense_w=t(A, 32, sc=0.3))
    live = torch.arange(Tk)[None, :] < torch.as_tensor(lens)[:, None]
    for k in ("mem", "enc"):
        d[k] = d[k] * live[:, :, None]
    for k in ("dwa", "dwb", "prev", "cum"):
        if k in d:
            d[k] = d[k] * live
    return d, live


def _ref_grads(mode, d, lens, dtype):
    B = d["h"].shape[0]
    lf = lambda x: x.to(dtype).clone().requires_grad_(True)                                      # noqa: E731
    h, Wq, mem, enc = lf(d["h"]), lf(d["Wq"]), lf(d["mem"]), d["enc"].to(dtype)
    v = lf(d["v"][None].expand(B, -1))
    prev = cum = conv_w = dense_w = None
    if mode == 1:
        prev, cum = lf(d["prev"]), lf(d["cum"])
        conv_w, dense_w = lf(d["conv_w"][None].expand(B, -1, -1, -1)), lf(d["dense_w"][None].expand(B, -1, -1))
    ctx, w, pq = attn_ref(mode, h, Wq, mem, v, enc, lens, prev, cum, conv_w, dense_w)
    dw_in = (d["dwa"] + d["dwb"]).to(dtype) if mode == 1 else torch.zeros_like(w)
    ((ctx * d["dctx"].to(dtype)).sum() + (w * dw_in).sum()).backward()
    out = dict(ctx=ctx.detach(), w=w.detach(), d_h=h.grad, d_q=pq.grad, d_mem=mem.grad, dv=v.grad)
    if mode == 1:
        out.update(d_prev=prev.grad, d_cum=cum.grad, ddense=dense_w.grad, dconv=conv_w.grad)
    return out


def _nerr(got, ref):
    ref = ref.double()
    return ((got.double().cpu() - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def _lens_for(B, Tk):
    edge = 257 if Tk > 257 else 65 if Tk > 65 else max(1, Tk - 1)                                # just past a block / a wave edge
    if B == 2:
        return [Tk, Tk - 255]                                                                    # a full row of keys and a ragged last block
    return [Tk, 1, edge][:B] if B > 1 else [Tk]


CASES = [(mode, B, Tk, A) for mode in (0, 1) for Tk in (1, 31, 64, 65, 300) for B, A in ((3, 32), (1, 64))] + [(0, 3, 300, 64), (1, 3, 300, 64)]
CASES += [(0, 2, 2048, 64), (1, 2, 2048, 64)]                 # the largest memory and width the entry points take: the 53 KB LDS launch


@pytest.mark.parametrize("mode,B,Tk,A", CASES)
def test_attn_step_bwd_matches_fp64_autograd(mode, B, Tk, A):
    from unast_amd import ops
    dev = _dev()
    lens = _lens_for(B, Tk)
    d, live = _case(mode, B, Tk, A, lens, seed=100 * Tk + 10 * B + mode)
    r64, r32 = _ref_grads(mode, d, lens, torch.float64), _ref_grads(mode, d, lens, torch.float32)
    names = [k for k in r64 if k not in ("ctx", "w")]
    e32 = max(EPS32, max(_nerr(r32[k], r64[k]) for k in names))
    bound = min(CAP, MARGIN * e32)
    # the kernel's inputs: NaN wherever a key is padding -- it must never read there
    nan = float("nan")
    g = {k: _g(v) for k, v in d.items()}
    dead = (~live).to(dev)
    for k in ("mem", "enc"):
        g[k][dead] = nan
    for k in ("dwa", "dwb", "prev", "cum"):
        if k in g:
            g[k][dead] = nan
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    # forward on the GPU (zeros in place of NaN for the forward's prev / cum: it reads the halo), then the saved weights feed the backward
    ctx, w = torch.empty(B, 512, device=dev), torch.full((B, Tk), nan, device=dev)
    fz = lambda t: torch.nan_to_num(t, nan=0.0) if t is not None else None                       # noqa: E731
    cum_out = torch.empty(B, Tk, device=dev) if mode == 1 else None
    ops.rnn_attn_step_train(mode, g["h"], g["Wq"], fz(g["mem"]), g["v"], fz(g["enc"]), lens_t, ctx, w, prev_in=fz(g.get("prev")), cum_in=fz(g.get("cum")),
                            cum_out=cum_out, conv_w=g.get("conv_w"), dense_w=g.get("dense_w"))
    assert torch.equal(w[dead], torch.zeros_like(w[dead]))
    # accuracy: zeroed accumulators, every tensor at the bound as it stands
    z = lambda *s: torch.zeros(*s, device=dev)                                                   # noqa: E731
    d_mem, dv = z(B, Tk, A), z(B, A)
    d_mem[dead] = 3.0                                                                            # rows of padded keys: must come back untouched
    d_h, d_q = torch.full((B, 256), nan, device=dev), torch.full((B, A), nan, device=dev)
    kw = {}
    if mode == 1:
        kw = dict(prev=g["prev"], cum=g["cum"], conv_w=g["conv_w"], dense_w=g["dense_w"], d_w_a=g["dwa"], d_w_b=g["dwb"], carry=False,
                  ddense_part=z(B, A, 32), dconv_part=z(B, 32, 2, 31), d_prev=torch.full((B, Tk), nan, device=dev),
                  d_cum=torch.full((B, Tk), nan, device=dev))
    ws = ops.rnn_attn_step_bwd_ws(B, Tk, A, dev)
    ws.fill_(nan)
    ops.rnn_attn_step_bwd(mode, g["dctx"], w, g["h"], g["Wq"], g["mem"], g["v"], g["enc"], lens_t, d_h, d_q, d_mem, dv, ws, **kw)
    torch.cuda.synchronize()
    assert torch.equal(d_mem[dead], torch.full_like(d_mem[dead], 3.0)), "d_mem rows of padded keys must not be touched"
    got = dict(d_h=d_h, d_q=d_q, d_mem=torch.where(dead[:, :, None], torch.zeros_like(d_mem), d_mem), dv=dv)
    if mode == 1:
        got.update(d_prev=kw["d_prev"], d_cum=kw["d_cum"], ddense=kw["ddense_part"], dconv=kw["dconv_part"])
        assert kw["d_prev"][dead].abs().sum().item() == 0.0 and kw["d_cum"][dead].abs().sum().item() == 0.0
    errs = {}
    for k in names:
        ref = r64[k] * live[:, :, None] if k == "d_mem" else r64[k] * live if k in ("d_prev", "d_cum") else r64[k]
        if ref.norm().item() <= 1e-9:                                                            # a single live key: the weights are the constant 1
            assert got[k].abs().max().item() <= 1e-6, k
            continue
        errs[k] = _nerr(got[k], ref)
    assert all(torch.isfinite(v).all() for v in got.values())
    ctx_err = (ctx.double().cpu() - r64["ctx"]).abs().max().item() / r64["ctx"].abs().max().item()
    worst = max(errs, key=errs.get) if errs else None
    print("mode %d B %d Tk %d A %d lens %s: e32 %.2e bound %.2e; forward ctx %.2e; worst %s %.2e = %.2f x e32; all: %s"
          % (mode, B, Tk, A, lens, e32, bound, ctx_err, worst, errs.get(worst, 0.0), errs.get(worst, 0.0) / e32,
             {k: "%.2f" % (e / e32) for k, e in errs.items()}))
    assert ctx_err <= 1e-3
    assert not errs or errs[worst] <= bound, {k: "%.2e" % e for k, e in errs.items() if e > bound}
    # '+=': a second call into pre-filled accumulators gives prefill + the first result to 2 ulp of the larger of prefill and sum (one fp32
    # rounding of the add; a second one where the compiler fuses the last product into it); padded d_mem rows stay as they were; with carry,
    # d_cum += d_w_b on the live keys
    gen = torch.Generator(device="cpu").manual_seed(7)
    fill = lambda t: torch.randn(t.shape, generator=gen).to(dev)                                 # noqa: E731
    d_mem0, dv0 = fill(d_mem), fill(dv)
    d_mem2, dv2, d_h2, d_q2 = d_mem0.clone(), dv0.clone(), torch.empty_like(d_h), torch.empty_like(d_q)
    kw2 = {}
    if mode == 1:
        dd0, dc0 = fill(kw["ddense_part"]), fill(kw["dconv_part"])
        kw2 = dict(kw, carry=True, ddense_part=dd0.clone(), dconv_part=dc0.clone(), d_prev=torch.empty(B, Tk, device=dev), d_cum=torch.empty(B, Tk, device=dev))
    ops.rnn_attn_step_bwd(mode, g["dctx"], w, g["h"], g["Wq"], g["mem"], g["v"], g["enc"], lens_t, d_h2, d_q2, d_mem2, dv2, ws, **kw2)
    torch.cuda.synchronize()
    assert torch.equal(d_h2, d_h) and torch.equal(d_q2, d_q)
    added = lambda out, base, first: bool(((out - (base + first)).abs() <= 2.0 ** -22 * torch.maximum(base.abs(), (base + first).abs())).all())  # noqa: E731
    assert torch.equal(d_mem2[dead], d_mem0[dead]) and added(d_mem2[~dead], d_mem0[~dead], d_mem[~dead]) and added(dv2, dv0, dv)
    if mode == 1:
        assert added(kw2["ddense_part"], dd0, kw["ddense_part"]) and added(kw2["dconv_part"], dc0, kw["dconv_part"])
        assert torch.equal(kw2["d_prev"], kw["d_prev"]) and added(kw2["d_cum"], kw["d_cum"], torch.where(dead, torch.zeros_like(g["dwb"]), g["dwb"]))


def test_three_chained_lsa_positions_pin_the_prev_cum_carry():
    from unast_amd import ops
    dev = _dev()
    B, Tk, A, lens = 3, 70, 32, [70, 1, 65]
    d, live = _case(1, B, Tk, A, lens, seed=5)
    r = np.random.RandomState(9)
    hs = [torch.from_numpy(r.standard_normal((B, 256)) * 0.5) for _ in range(3)]
    dctxs = [torch.from_numpy(r.standard_normal((B, 512))) for _ in range(3)]

    def chain(dtype):
        lf = lambda x: x.to(dtype).clone().requires_grad_(True)                                  # noqa: E731
        h3, mem = [lf(h) for h in hs], lf(d["mem"])
        Wq, enc = d["Wq"].to(dtype), d["enc"].to(dtype)
        v, cw, dw = (d[k].to(dtype)[None].expand(B, *d[k].shape) for k in ("v", "conv_w", "dense_w"))
        prev, cum = torch.zeros(B, Tk, dtype=dtype), torch.zeros(B, Tk, dtype=dtype)
        L = 0
        for i in range(3):
            ctx, w, _ = attn_ref(1, h3[i], Wq, mem, v, enc, lens, prev, cum, cw, dw)
            prev, cum = w, cum + w
            L = L + (ctx * dctxs[i].to(dtype)).sum()
        L.backward()
        return [h.grad for h in h3] + [mem.grad]

    r64, r32 = chain(torch.float64), chain(torch.float32)
    e32 = max(EPS32, max(_nerr(a, b) for a, b in zip(r32, r64)))
    bound = min(CAP, MARGIN * e32)
    g = {k: _g(v) for k, v in d.items()}
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    W, CUM = torch.zeros(B, 4, Tk, device=dev), torch.zeros(B, 4, Tk, device=dev)
    ctx = torch.empty(B, 512, device=dev)
    hq = [_g(h) for h in hs]
    for i in range(3):
        ops.rnn_attn_step_train(1, hq[i], g["Wq"], g["mem"], g["v"], g["enc"], lens_t, ctx, W[:, i + 1], prev_in=W[:, i], cum_in=CUM[:, i],
                                cum_out=CUM[:, i + 1], conv_w=g["conv_w"], dense_w=g["dense_w"])
    z = lambda *s: torch.zeros(*s, device=dev)                                                   # noqa: E731
    d_mem, dv, dd, dc = z(B, Tk, A), z(B, A), z(B, A, 32), z(B, 32, 2, 31)
    dprev, dcum = [z(B, Tk), z(B, Tk)], [z(B, Tk), z(B, Tk)]
    ws = ops.rnn_attn_step_bwd_ws(B, Tk, A, dev)
    d_hs = [None] * 3
    for i in (2, 1, 0):
        cur, nxt = (2 - i) & 1, (3 - i) & 1
        d_hs[i], d_q = torch.empty(B, 256, device=dev), torch.empty(B, A, device=dev)
        ops.rnn_attn_step_bwd(1, _g(dctxs[i]), W[:, i + 1], hq[i], g["Wq"], g["mem"], g["v"], g["enc"], lens_t, d_hs[i], d_q, d_mem, dv, ws,
                              prev=W[:, i], cum=CUM[:, i], conv_w=g["conv_w"], dense_w=g["dense_w"], d_w_a=dprev[cur], d_w_b=dcum[cur], carry=True,
                              ddense_part=dd, dconv_part=dc, d_prev=dprev[nxt], d_cum=dcum[nxt])
    torch.cuda.synchronize()
    errs = [_nerr(a, b) for a, b in zip(d_hs + [d_mem], r64)]
    print("three chained LSA positions: e32 %.2e, errors d_h0..2, d_mem %s = %.2f x e32 at worst" % (e32, ["%.2e" % e for e in errs], max(errs) / e32))
    assert max(errs) <= bound


@pytest.mark.parametrize("mode", [0, 1])
def test_train_forward_carries_the_eval_kernels_bits(mode):
    from unast_amd import ops
    dev = _dev()
    B, Tk, A, lens = 3, 300, 32, [300, 1, 257]
    d, _ = _case(mode, B, Tk, A, lens, seed=3)
    g = {k: _g(v) for k, v in d.items()}
    lens_t = torch.tensor(lens, dtype=torch.int32, device=dev)
    prev, cum = torch.zeros(B, Tk, device=dev), torch.zeros(B, Tk, device=dev)
    Tkp = 304
    W, CUM = torch.zeros(B, 3, Tkp, device=dev), torch.zeros(B, 3, Tkp, device=dev)
    slab = torch.empty(B, 2, 768, device=dev)
    r = np.random.RandomState(1)
    for i in range(2):
        h = _g(torch.from_numpy(r.standard_normal((B, 256)) * 0.5))
        ctx = torch.empty(B, 512, device=dev)
        ops.rnn_attn_step(mode, h, g["Wq"], g["mem"], g["v"], g["enc"], lens_t, ctx, prev=prev, cum=cum if mode == 1 else None, conv_w=g.get("conv_w"),
                          dense_w=g.get("dense_w"))
        ops.rnn_attn_step_train(mode, h, g["Wq"], g["mem"], g["v"], g["enc"], lens_t, slab[:, i, 256:], W[:, i + 1, :Tk], prev_in=W[:, i, :Tk],
                                cum_in=CUM[:, i, :Tk], cum_out=CUM[:, i + 1, :Tk], conv_w=g.get("conv_w"), dense_w=g.get("dense_w"))
        assert torch.equal(ctx, slab[:, i, 256:]) and torch.equal(prev, W[:, i + 1, :Tk])
        if mode == 1:
            assert torch.equal(cum, CUM[:, i + 1, :Tk])
    assert W[:, :, Tk:].abs().sum().item() == 0.0                                                # the row padding is never written
    if mode == 1:                                                                                # in place is unast_rnn_attn_step's form
        with pytest.raises(Exception):
            ops.rnn_attn_step_train(1, h, g["Wq"], g["mem"], g["v"], g["enc"], lens_t, ctx, prev, prev_in=prev, cum_in=cum, cum_out=cum,
                                    conv_w=g["conv_w"], dense_w=g["dense_w"])


@pytest.mark.parametrize("B", [1, 3])
def test_lstm_cell_train_and_bwd(B):
    from unast_amd import ops
    dev = _dev()
    r = np.random.RandomState(B)
    gates, c_prev = torch.from_numpy(r.standard_normal((B, 1024)) * 1.5), torch.from_numpy(r.standard_normal((B, 256)))
    mask = torch.from_numpy((r.rand(B, 256) > 0.3) / 0.7)
    dh, dh2, dc_in = (torch.from_numpy(r.standard_normal((B, 256))) for _ in range(3))
    gg, cg = _g(gates), _g(c_prev)
    c_eval, h_eval = cg.clone(), torch.empty(B, 256, device=dev)
    ops.lstm_cell(gg, c_eval, h_eval)
    slab = torch.empty(B, 2, 5, 256, device=dev)                                                 # row-strided operands, as the loop passes them
    hs, hd = torch.empty(B, 2, 256, device=dev), torch.empty(B, 256, device=dev)
    ops.lstm_cell_train(gg, cg, slab[:, 1], hs[:, 1], mask=_g(mask), hd=hd)
    assert torch.equal(hs[:, 1], h_eval) and torch.equal(slab[:, 1, 4], c_eval), "the train cell must carry the eval cell's bits"
    assert torch.equal(hd, h_eval * _g(mask))

    def ref(dtype):
        g_, c_, d2 = (t.to(dtype).clone().requires_grad_(True) for t in (gates, c_prev, dh2))
        i, f, g, o = g_.chunk(4, -1)
        c = torch.sigmoid(f) * c_ + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        ((h * (dh.to(dtype) + dh2.to(dtype) * mask.to(dtype))).sum() + (c * dc_in.to(dtype)).sum()).backward()
        return g_.grad, c_.grad

    r64, r32 = ref(torch.float64), ref(torch.float32)
    e32 = max(EPS32, max(_nerr(a, b) for a, b in zip(r32, r64)))
    dG, dc_out = torch.empty(B, 2, 1024, device=dev), _g(dc_in)
    ops.lstm_cell_bwd(slab[:, 1], cg, dG[:, 0], dc_out, dh=_g(dh), dh2=_g(dh2), mask=_g(mask), dc_in=dc_out)            # dc_out in place of dc_in
    torch.cuda.synchronize()
    errs = (_nerr(dG[:, 0], r64[0]), _nerr(dc_out, r64[1]))
    print("lstm_cell_bwd B %d: e32 %.2e, dG %.2e, dc %.2e = %.2f x e32 at worst" % (B, e32, errs[0], errs[1], max(errs) / e32))
    assert max(errs) <= min(CAP, MARGIN * e32)
    # None operands are zeros
    dG2, dc2 = torch.empty(B, 1024, device=dev), torch.empty(B, 256, device=dev)
    ops.lstm_cell_bwd(slab[:, 1], cg, dG2, dc2)
    assert dG2.abs().sum().item() == 0.0 and dc2.abs().sum().item() == 0.0
    # tanh_bwd
    y, dy = torch.tanh(_g(dh)), _g(dh2)
    want = dy.double() * (1 - y.double() ** 2)
    ops.tanh_bwd(dy, y)
    assert _nerr(dy, want.cpu()) <= 4 * EPS32
