"""The fp32-level contractions and the version-keyed operand cache, written once for the RNN family (unast_amd.rnn, unast_amd.train_rnn) and
the CBHG vocoder (unast_amd.vocoder, unast_amd.train_vocoder).  No kernel of its own: every function is a fixed sequence of unast_amd.ops calls.

The scheme.  One split-bf16 launch forms a_hi b_hi + a_hi b_lo + a_lo b_hi: it drops a_lo b_lo and whatever lies below 2^-17 of
either operand.  The main model accepts that floor.  Greedy trajectories held to the reference's own fp32 error and gradients
behind a 16-deep conv + BatchNorm + ReLU chain do not, so their contractions are formed as

    x = hi + rest  (hi = RNE_bf16(x), exactly a bf16),   W = W_hi + W_lo + wr  (wr = `resid(W)[1]`):      hi W + rest W + x wr

Why three launches: the first has no a_lo to drop; the second one's a_hi is the first one's missing a_lo and its a_lo the part of x below both;
the third brings in what W's two bf16 parts leave out.  The partial sums chain through the GEMM's residual operand in fp32.  What is dropped
is rest_lo W_lo, x_lo wr_lo and what lies below wr's own two parts: products of order 2^-26.  ops.split_parts (one element-wise kernel) writes
the parts.  The gradient forms (dgrad_rows, wgrad_rows, conv_grads) split dy the same way and take the other operand with its residual; the
vocoder's backward does NOT use them (one launch per gradient contraction on purpose).

Operand names throughout: Wp = resid(W) is a weight pair (W, wr); dyp = parts(dy) is (dy, hi, rest); xres = resid_of(x).
"""
import torch

from . import ops

_F32 = torch.float32


def buf(*shape, dev):
    return torch.empty(*shape, dtype=_F32, device=dev)


def detached(t):
    return t.detach().contiguous()


def relu_(x):
    ops.leaky_dropout(x, None, x, 0.0)
    return x


# ---- operand parts -------------------------------------------------------------------------------------------------------------------------
def resid(w):
    """(w, what the GEMM's split-bf16 operand preparation drops of w): a weight pair."""
    w = detached(w)
    wr = torch.empty_like(w)
    ops.split_parts(w, resid=wr)
    return w, wr


def resid_of(x):
    """What the operand preparation drops of x (contiguous): the activation-side partner of a gradient contraction."""
    r = torch.empty_like(x)
    ops.split_parts(x, resid=r)
    return r


def parts(x):
    """(x contiguous, hi, rest)."""
    x = x.contiguous()
    hi, rest = torch.empty_like(x), torch.empty_like(x)
    ops.split_parts(x, hi=hi, rest=rest)
    return x, hi, rest


def tap_major(conv):
    """A Conv1d's weight as the tap kernels read it ([Cout, taps, Cin]) with its residual, and its bias."""
    return resid(conv.weight.detach().permute(0, 2, 1)), detached(conv.bias)


def fold_bn(conv, bn):
    """Tap-major weights and bias of conv followed by eval BatchNorm: BN(Wx + b) = (s W) x + (b - mean) s + beta, s = gamma / sqrt(var + eps).
    Formed in fp64 and rounded once."""
    s = bn.weight.double() * torch.rsqrt(bn.running_var.double() + bn.eps)
    w = (conv.weight.double() * s[:, None, None]).permute(0, 2, 1).contiguous().to(_F32)
    b = ((conv.bias.double() - bn.running_mean.double()) * s + bn.bias.double()).to(_F32)
    return w, b


# ---- forward -------------------------------------------------------------------------------------------------------------------------------
def _scratch(what, x, out, work, shape):
    """Checks a caller's `out` and `work` = (x's two parts, two partial sums) before anything is launched; `shape`: the partial sums' (and a
    dense out's)."""
    def ok(t, shp, dense=True):
        return torch.is_tensor(t) and t.dtype is _F32 and t.device == x.device and tuple(t.shape) == tuple(shp) and (t.is_contiguous() or not dense)
    if out is not None and not ok(out, shape, dense=len(shape) == 2):
        raise ValueError("%s: out must be a float32 %s tensor on x's device" % (what, tuple(shape)))
    if work is not None and not (len(work) == 4 and all(ok(t, x.shape) for t in work[:2]) and all(ok(t, shape) for t in work[2:])):
        raise ValueError("%s: work must be four dense float32 tensors on x's device: x's parts %s twice, the partial sums %s twice"
                         % (what, tuple(x.shape), tuple(shape)))


def linear_rows(x2d, Wp, b, act=0, out=None, work=None):
    """y = act(x W^T + b) for many rows (act 1: ReLU).  out: a dense [M, ld] buffer, ld >= N; its first N columns are written, the pad columns
    never.  work: x's two parts [M,K] and two partial sums [M, ld] of a caller that keeps them across a step.  Returns out[:, :N] (out itself
    when ld == N).  The ReLU kernel reads dense rows, so act with ld > N (no caller on a hot path) stages the last launch in a dense [M,N]
    buffer and copies it in."""
    W, Wr = Wp
    M, K = x2d.shape
    N = W.shape[0]
    dev = x2d.device
    if out is not None and not (torch.is_tensor(out) and out.dim() == 2 and out.shape[1] >= N):
        raise ValueError("linear_rows: out must be a dense [%d, ld >= %d] tensor" % (M, N))
    ld = out.shape[1] if out is not None else N
    _scratch("linear_rows", x2d, out, work, (M, ld))
    x = x2d.contiguous()
    xh, xr = work[:2] if work is not None else (torch.empty_like(x), torch.empty_like(x))
    ops.split_parts(x, hi=xh, rest=xr)
    t1, t2 = work[2:] if work is not None else (buf(M, ld, dev=dev), buf(M, ld, dev=dev))
    y = out if out is not None and not (act and ld > N) else buf(M, N, dev=dev)
    ops.gemm(ops.OP_KC, ops.OP_KC, xh, K, W, K, t1, ld, M, N, K, bias=b)
    ops.gemm(ops.OP_KC, ops.OP_KC, xr, K, W, K, t2, ld, M, N, K, R=t1, ldr=ld)
    ops.gemm(ops.OP_KC, ops.OP_KC, x, K, Wr, K, y, y.stride(0), M, N, K, R=t2, ldr=ld)
    if act:
        relu_(y)
    if out is None or ld == N:
        return y
    if y is not out:
        out[:, :N].copy_(y)
    return out[:, :N]


def conv(x3d, Wp, b, pad_left, out=None, work=None):
    """out = conv(x, W) + b (no activation), Wp = a tap-major pair (tap_major, or resid of a folded weight).  out: [B,T,Cout], any strides the
    tap kernels take.  work: x's two parts [B,T,Cin] and two partial sums [B,T,Cout] of a caller that runs the same shape every step."""
    W, Wr = Wp
    B, T, _ = x3d.shape
    dev = x3d.device
    _scratch("conv", x3d, out, work, (B, T, W.shape[0]))
    x = x3d.contiguous()
    xh, xr, za, zb = work if work is not None else (torch.empty_like(x), torch.empty_like(x), buf(B, T, W.shape[0], dev=dev), buf(B, T, W.shape[0], dev=dev))
    ops.split_parts(x, hi=xh, rest=xr)
    out = out if out is not None else buf(B, T, W.shape[0], dev=dev)
    ops.conv_taps_fwd(xh, W, b, za, pad_left)
    ops.conv_taps_fwd(xr, W, None, zb, pad_left, R=za)
    ops.conv_taps_fwd(x, Wr, None, out, pad_left, R=zb)
    return out


# ---- gradients (the RNN family's; module docstring) -------------------------------------------------------------------------------------------
ALL = slice(None)


def dgrad_rows(dyp, Wp, dx):
    """dx[M,K] = dy[M,N] W[N,K]."""
    dy, dyh, dyr = dyp
    W, Wr = Wp
    t1, t2 = torch.empty_like(dx), torch.empty_like(dx)
    ops.linear_dgrad(dyh, W, t1)
    ops.linear_dgrad(dyr, W, t2, R=t1)
    ops.linear_dgrad(dy, Wr, dx, R=t2)
    return dx


def wgrad_rows(dyp, cols, x2d, xres, dW, dbs=()):
    """dW[N,K] += dy[:, cols]^T x, every db += column sums of dy[:, cols]."""
    dy, dyh, dyr = (t[:, cols] for t in dyp)
    M, N = dy.shape
    K = x2d.shape[1]
    sk = ops._splitk_for(N, K, M)
    for a, b in ((dyh, x2d), (dyr, x2d), (dy, xres)):
        ops.gemm(ops.OP_RC, ops.OP_RC, a, a.stride(0), b, b.stride(0), dW, dW.stride(0), N, K, M, beta=1, splitk=sk)
    for db in dbs:
        ops.colsum(dy, db)


def conv_grads(dz2d, x2d, B, T, wpair, conv, pad_left):
    """Weight, bias and input gradient of one tap-major conv (the text prenets' and the post-net's backward): conv.weight.grad and
    conv.bias.grad are added to, dx [B*T, Cin] is returned."""
    wp, wr = wpair
    C, Cin = dz2d.shape[1], x2d.shape[1]
    dz, dzh, dzr = (t.view(B, T, C) for t in parts(dz2d))
    gw = torch.zeros_like(wp)
    x3, x3res = x2d.view(B, T, Cin), resid_of(x2d).view(B, T, Cin)
    ops.conv_taps_wgrad(dzh, x3, gw, pad_left)
    ops.conv_taps_wgrad(dzr, x3, gw, pad_left)
    ops.conv_taps_wgrad(dz, x3res, gw, pad_left)
    conv.weight.grad.add_(gw.permute(0, 2, 1))
    ops.colsum(dz.view(B * T, C), conv.bias.grad)
    dx = buf(B, T, Cin, dev=dz2d.device)
    ops.conv_taps_dgrad(dzh, wp, dx, pad_left)
    ops.conv_taps_dgrad(dzr, wp, dx, pad_left, beta=1)
    ops.conv_taps_dgrad(dz, wr, dx, pad_left, beta=1)
    return dx.view(B * T, Cin)


# ---- what every train step does before its first launch ------------------------------------------------------------------------------------
def prepare_grads(params, accumulate):
    """Dense .grad of every parameter in its own shape, zeroed unless `accumulate` (a .grad that already is one is kept: the flat optimizers'
    views stay in place)."""
    gs = []
    for p in params:
        g = p.grad
        if g is None or not g.is_contiguous() or g.dtype is not _F32 or g.device != p.device or g.data_ptr() % 16:
            new = torch.zeros_like(p, memory_format=torch.contiguous_format)
            if accumulate and g is not None:
                new.copy_(g)
            g = p.grad = new
        gs.append(g)
    if not accumulate:
        torch._foreach_zero_(gs)


def check_bn(bn, what):
    if bn.momentum is None or not bn.track_running_stats or not bn.affine:
        raise NotImplementedError("%s: BatchNorm1d with affine parameters, running statistics and a fixed momentum (the reference's)" % what)


# ---- the version-keyed cache of derived operands: one slot in a module's __dict__ per pack ------------------------------------------------
def cached_operands(m, slot, tensors, build):
    """m's pack in `slot`, built by build() and rebuilt when the version counter of one of `tensors` has moved (or the device changed).
    Kernel writes behind the counters (BatchNorm running statistics, the flat optimizers) do not move the key: whoever makes them pops the slot."""
    key = (sum(t._version for t in tensors), tensors[-1].device if tensors else None)
    cached = m.__dict__.get(slot)
    if cached is None or cached[0] != key:
        cached = (key, build())
        m.__dict__[slot] = cached
    return cached[1]
