"""The kernels of the prefix prenet (csrc/prefix.hip: unast_prefix_bn_fwd, unast_prefix_bn_bwd, unast_prefix_embed_fwd, unast_prefix_embed_bwd)
against fp64 torch on random, non-identical rows in the slab layout of unast_amd.train_rnn.prefix_layout.

Shapes: (B, T) = (2,1) one segment of 2 rows; (2,2); (3,9) the fixtures' shape; (7,40) segments on either side of 64 and 256 live rows (7 x 9 = 63,
7 x 10 = 70, 7 x 36 = 252, 7 x 37 = 259) and of 64-row chunk edges; (2,130) segments of 256 and 258 live rows and the longest prefixes.  C = 256.
Gap rows of every input a kernel is documented not to read hold NaN; its outputs at gap rows must be exact zeros.
Bounds: forward 1e-3 x max|ref|; gradients min(1e-3, 16 x e32) in relative L2 norm, e32 = a torch fp32 run of the same math against
the fp64 run."""
import functools

import numpy as np
import pytest
import torch

from tests import dropout_mirror as DM
from tests import rnn_train_mirror as TM

pytestmark = pytest.mark.gpu

C = 256
SHAPES = [(2, 1), (2, 2), (3, 9), (7, 40), (2, 130)]
PS = [0.0, 0.5]
SEED, STREAM = 31, 17
EPS, MOM = 1e-5, 0.1
FWD_TOL, GRAD_CAP, GRAD_MARGIN = 1e-3, 1e-3, 16.0


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _geom(B, T):
    from unast_amd.train_rnn import prefix_layout, GAP
    lay = prefix_layout(B, T)
    seg = []                                                   # per segment: live rows [B, L]
    live = np.zeros(lay.total, bool)
    for s in range(T):
        L = lay.lens[s]
        rows = lay.off[s] + np.arange(B)[:, None] * (L + GAP) + np.arange(L)[None, :]
        seg.append(torch.from_numpy(rows))
        live[rows.reshape(-1)] = True
    return lay, seg, torch.from_numpy(live)


def _bn_math(x, gamma, beta, seg, mask, dtype, rm, rv):
    """Per-segment train-mode BatchNorm + ReLU + dropout over the live rows of x [R,C]; returns y [R,C] (zeros on gap rows), mean, rstd [T,C]
    and updates rm, rv in segment order."""
    y = torch.zeros_like(x)
    means, rstds = [], []
    for rows in seg:
        flat = x[rows.reshape(-1)]
        n = flat.shape[0]
        mean, var = flat.mean(0), flat.var(0, unbiased=False)
        rstd = 1.0 / torch.sqrt(var + EPS)
        v = torch.relu((flat - mean) * rstd * gamma + beta)
        if mask is not None:
            v = v * mask[rows.reshape(-1)].to(dtype)
        y = y.index_put((rows.reshape(-1),), v)
        means.append(mean.detach())
        rstds.append(rstd.detach())
        rm.mul_(1 - MOM).add_(MOM * mean.detach().to(rm.dtype))
        rv.mul_(1 - MOM).add_(MOM * (var.detach() * n / (n - 1)).to(rv.dtype))
    return y, torch.stack(means), torch.stack(rstds)


@functools.lru_cache(maxsize=None)
def _case(B, T, p):
    """Inputs and the fp64 / fp32 references of one (B, T, p), computed once and left unchanged."""
    lay, seg, live = _geom(B, T)
    R = lay.total
    r = np.random.RandomState(1000 * B + T)
    x = torch.from_numpy(r.standard_normal((R, C)) * 1.5 + 0.3).float()
    gamma, beta = torch.from_numpy(r.uniform(0.5, 1.5, C)).float(), torch.from_numpy(r.standard_normal(C) * 0.3).float()
    dy, dP = torch.from_numpy(r.standard_normal((R, C))).float(), torch.from_numpy(r.standard_normal((B, T, C))).float()
    rm0, rv0 = torch.from_numpy(r.standard_normal(C)).float(), torch.from_numpy(r.uniform(0.5, 2.0, C)).float()
    mask = torch.from_numpy(DM.drop_factor(SEED, STREAM, R, C, p)) if p > 0 else None
    last = torch.stack([seg[s][:, -1] for s in range(T)], 1)                                         # [B,T] slab row of each prefix's last row
    out = dict(x=x, gamma=gamma, beta=beta, dy=dy, dP=dP, rm0=rm0, rv0=rv0, live=live, last=last, lay=lay, seg=seg, mask=mask)
    for dtype, tag in ((torch.float64, "64"), (torch.float32, "32")):
        xl, gl, bl = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
        rm, rv = rm0.clone(), rv0.clone()                                                            # fp32 running statistics, as torch keeps them
        y, mean, rstd = _bn_math(xl, gl, bl, seg, mask, dtype, rm, rv)
        gx, gg, gb = torch.autograd.grad((y * dy.to(dtype)).sum(), (xl, gl, bl), retain_graph=True)
        hx, hg, hb = torch.autograd.grad((y[last] * dP.to(dtype)).sum(), (xl, gl, bl))
        out["r" + tag] = dict(y=y.detach(), mean=mean, rstd=rstd, rm=rm, rv=rv, slab=(gx, gg, gb), last=(hx, hg, hb))
    return out


def _tabs(B, T):
    from unast_amd.train_rnn import prefix_tables
    return prefix_tables(B, T, _dev())


def _nan_gaps(t, live):
    t = t.clone()
    t[~live] = float("nan")
    return t.to(_dev())


def _run_fwd(cs, B, T, p, last_only):
    from unast_amd import ops
    tabs, dev = _tabs(B, T), _dev()
    R = cs["lay"].total
    x = _nan_gaps(cs["x"], cs["live"])
    mean, rstd, varu = (torch.empty(T, C, device=dev) for _ in range(3))
    rm, rv, nbt = cs["rm0"].to(dev), cs["rv0"].to(dev), torch.zeros((), dtype=torch.int64, device=dev)
    y = None if last_only else torch.full((R, C), 7.0, device=dev)
    P = torch.full((B, T, C), 7.0, device=dev) if last_only else None
    ops.prefix_bn_fwd(x, tabs, cs["gamma"].to(dev), cs["beta"].to(dev), mean, rstd, varu, ops.prefix_bn_ws(tabs, C, dev), y=y, p_last=P, running_mean=rm,
                      running_var=rv, num_batches_tracked=nbt, eps=EPS, momentum=MOM, drop_p=p, seed=SEED, stream_id=STREAM)
    torch.cuda.synchronize()
    return dict(y=y, P=P, mean=mean, rstd=rstd, rm=rm, rv=rv, nbt=nbt)


def _close(name, got, ref, tol=FWD_TOL):
    got, ref = got.detach().cpu().double(), ref.double()
    err, mx = (got - ref).abs().max().item(), ref.abs().max().item()
    print("%-28s err %.3g = %.3g of max|ref|" % (name, err, err / mx))
    assert err <= tol * mx, (name, err, mx)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("B,T", SHAPES)
def test_segmented_batchnorm_forward(B, T, p):
    cs = _case(B, T, p)
    r64 = cs["r64"]
    a = _run_fwd(cs, B, T, p, False)
    live = cs["live"]
    assert a["y"][~live.to(_dev())].abs().max().item() == 0.0, "gap rows must be exact zeros"
    assert torch.isfinite(a["y"]).all()
    _close("y", a["y"], r64["y"])
    _close("mean", a["mean"], r64["mean"])
    _close("rstd", a["rstd"], r64["rstd"])
    # the running statistics after T sequential momentum updates, against the fp32 torch loop (its own fp32 statistics: 1e-6 of their scale per update)
    _close("running_mean", a["rm"], cs["r32"]["rm"], 2e-5)
    _close("running_var", a["rv"], cs["r32"]["rv"], 2e-5)
    _close("running_mean vs fp64", a["rm"], r64["rm"], 2e-5)
    assert int(a["nbt"]) == T
    # stage 3's form: each prefix's last row straight into [B,T,C]; the same statistics; two runs agree to the bit
    b = _run_fwd(cs, B, T, p, True)
    assert torch.equal(b["P"], a["y"][cs["last"].to(_dev())]), "p_last must carry the slab form's bits"
    for k in ("mean", "rstd", "rm", "rv"):
        assert torch.equal(a[k], b[k]), k
    a2 = _run_fwd(cs, B, T, p, False)
    assert all(torch.equal(a[k], a2[k]) for k in ("y", "mean", "rstd", "rm", "rv"))


def _check_grad(name, got, r64, r32):
    # (two-row segments under a mask leave sums of at most two terms, which torch's fp32 run forms exactly: e32 = 0.  An fp32 result cannot be
    #  held below its own rounding, so e32 is floored at the fp32 unit roundoff 2^-24.)
    e32 = max(TM.normerr(r32, r64), 2.0 ** -24)
    err = TM.normerr(got.detach().cpu(), r64)
    bound = min(GRAD_CAP, GRAD_MARGIN * e32)
    print("%-28s err %.3g, e32 %.3g, %.2f of its bound" % (name, err, e32, err / bound))
    assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("last_only", [False, True])
@pytest.mark.parametrize("B,T", SHAPES)
def test_segmented_batchnorm_backward(B, T, p, last_only):
    from unast_amd import ops
    cs = _case(B, T, p)
    tabs, dev, live = _tabs(B, T), _dev(), cs["live"]
    fwd = _run_fwd(cs, B, T, p, False)
    x = _nan_gaps(cs["x"], live)
    dy = cs["dP"].to(dev) if last_only else _nan_gaps(cs["dy"], live)
    key = "last" if last_only else "slab"

    def run():
        dz = torch.full((cs["lay"].total, C), 7.0, device=dev)
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)                               # accumulated into (a non-zero base would add its own rounding)
        ops.prefix_bn_bwd(dy, x, tabs, fwd["mean"], fwd["rstd"], cs["gamma"].to(dev), cs["beta"].to(dev), dz, dg, db, ops.prefix_bn_ws(tabs, C, dev),
                          last_only=last_only, drop_p=p, seed=SEED, stream_id=STREAM)
        torch.cuda.synchronize()
        return dz, dg, db

    dz, dg, db = run()
    assert dz[~live.to(dev)].abs().max().item() == 0.0, "gap rows must be exact zeros"
    assert torch.isfinite(dz).all()
    (gx64, gg64, gb64), (gx32, gg32, gb32) = cs["r64"][key], cs["r32"][key]
    _check_grad("dz", dz, gx64, gx32)
    _check_grad("dgamma", dg, gg64, gg32)
    _check_grad("dbeta", db, gb64, gb32)
    dz2, dg2, db2 = run()
    assert torch.equal(dz, dz2) and torch.equal(dg, dg2) and torch.equal(db, db2), "two runs must agree to the bit"


@pytest.mark.parametrize("p", PS)
def test_degenerate_segment_of_identical_rows(p):
    """Identical rows (position 0: [SOS] in every sequence): zero variance, x_hat = 0, the forward is relu(beta) times the mask factor."""
    from unast_amd import ops
    B, T = 3, 3
    lay, seg, live = _geom(B, T)
    cs = _case(3, 9, p)
    dev, tabs = _dev(), _tabs(B, T)
    x = torch.from_numpy(np.random.RandomState(4).standard_normal((lay.total, C))).float()
    x[seg[0].reshape(-1)] = x[seg[0][0, 0]].clone()                                                   # segment 0: B identical rows
    x[seg[2].reshape(-1)] = x[seg[2][0, 0]].clone()                                                   # segment 2: B x 2 identical rows
    mean, rstd, varu = (torch.empty(T, C, device=dev) for _ in range(3))
    y = torch.empty(lay.total, C, device=dev)
    beta = cs["beta"].to(dev)
    ops.prefix_bn_fwd(_nan_gaps(x, live), tabs, cs["gamma"].to(dev), beta, mean, rstd, varu, ops.prefix_bn_ws(tabs, C, dev), y=y, eps=EPS, drop_p=p, seed=SEED,
                      stream_id=STREAM)
    torch.cuda.synchronize()
    f = torch.from_numpy(DM.drop_factor(SEED, STREAM, lay.total, C, p)).float().to(dev) if p > 0 else torch.ones(lay.total, C, device=dev)
    for s in (0, 2):
        rows = seg[s].reshape(-1).to(dev)
        want = torch.relu(beta)[None, :] * f[rows]
        # x - mean is at most one fp32 rounding of |x| <= 5 (3e-7), times rstd = eps^-1/2 = 316 and gamma <= 1.5: 1.5e-4 at the very most; an exact
        # mean (fp64 sums of identical values) leaves 0
        assert (y[rows] - want).abs().max().item() <= 1.5e-4 * float(f.max()), s
        assert abs(rstd[s].mean().item() - EPS ** -0.5) <= 1e-2 and varu[s].abs().max().item() <= 1e-10


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("B,T", SHAPES)
def test_embedded_slab_gather_and_scatter(B, T, p):
    from unast_amd import ops
    from unast_amd.utils import SOS_IDX
    lay, seg, live = _geom(B, T)
    dev, tabs = _dev(), _tabs(B, T)
    V, D = 46, 256
    r = np.random.RandomState(7 * B + T)
    E = torch.from_numpy(r.standard_normal((V, D))).float()                                           # row 0 (PAD) is NOT zero: gaps must not lean on it
    tgt = torch.from_numpy(r.randint(0, V, size=(B, T)).astype(np.int64))
    ids = torch.zeros(lay.total, dtype=torch.int64)
    for s in range(T):
        ids[seg[s].reshape(-1)] = (torch.full((B, 1), SOS_IDX, dtype=torch.int64) if s == 0 else tgt[:, :s]).reshape(-1)
    f = torch.from_numpy(DM.drop_factor(SEED, STREAM, lay.total, D, p)) if p > 0 else torch.ones(lay.total, D, dtype=torch.float64)
    out = torch.full((lay.total, D), 7.0, device=dev)
    ops.prefix_embed_fwd(tgt.to(dev), E.to(dev), tabs, out, SOS_IDX, drop_p=p, seed=SEED, stream_id=STREAM)
    torch.cuda.synchronize()
    want = (E.double()[ids] * f) * live[:, None]
    assert out[~live.to(dev)].abs().max().item() == 0.0, "gap rows must be exact zeros"
    _close("embedded slab", out, want, 1e-6)
    # the scatter: dE[v] = sum of the masked gradient rows whose token is v, PAD excluded
    dx = torch.from_numpy(r.standard_normal((lay.total, D))).float()

    def ref(dtype):
        g = (dx.to(dtype) * f.to(dtype))[live]
        dE = torch.zeros(V, D, dtype=dtype).index_add_(0, ids[live], g)
        dE[0] = 0.0
        return dE

    def run():
        G = torch.empty(B, T + 1, D, device=dev)
        dE = torch.zeros(V, D, device=dev)
        ops.prefix_embed_bwd(_nan_gaps(dx, live), tabs, G, drop_p=p, seed=SEED, stream_id=STREAM)
        ids_ext = torch.cat([torch.full((B, 1), SOS_IDX, dtype=torch.int64), tgt], 1).contiguous().to(dev)
        ops.embed_bwd(ids_ext, G.view(B * (T + 1), D), dE, T + 1, padding_idx=0)
        torch.cuda.synchronize()
        return G, dE

    G, dE = run()
    assert torch.isfinite(G).all() and G[:, T].abs().max().item() == 0.0                              # target[:, T-1] is in no prefix
    assert dE[0].abs().max().item() == 0.0, "the PAD row gets no gradient"
    _check_grad("dE", dE, ref(torch.float64), ref(torch.float32))
    G2, _ = run()
    assert torch.equal(G, G2), "two runs must agree to the bit"
