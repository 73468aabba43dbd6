"""Forward + hand-written backward of every block on the UNAST train-step hot path, as sequences of HIP kernel
launches (unast_amd.ops).  Each function runs the forward immediately and, when a Tape is given, records one closure
that consumes the gradient of its output Var(s) and produces the gradients of its inputs / parameters.

Reference semantics per block are cited next to each function (file:line in /root/reference).
Activations are fp32 [B*T, C] row-major (token-major); `lens` are int32 device tensors.
"""
import math

import torch

from . import config, ops
from .engine import Var, acc
from .utils import is_deterministic, lens_i32

LN_EPS = 1e-5


class Ctx:
    """Per-call context: parameter store, dropout configuration, RNG stream allocation."""

    def __init__(self, store, training, seed):
        self.st = store
        store.sync_split()
        self.P = store.phys
        self.training = training
        self.stochastic = training and not is_deterministic()      # dropout sites active
        self.noisy = not is_deterministic()                         # noise_fn ignores model.training (src/utils.py:40-49)
        self.seed = seed & 0xFFFFFFFF
        self._stream = 0

    def stream(self):
        self._stream += 1
        return self._stream

    def p(self, rate):
        return float(rate) if self.stochastic else 0.0


def _empty(*shape, like=None, device=None):
    return torch.empty(*shape, dtype=torch.float32, device=(like.device if like is not None else device))


def _bias_grad(cx, dy2d, name_or_view):
    g = cx.st.g(name_or_view) if isinstance(name_or_view, str) else name_or_view
    if g is not None:
        ops.colsum(dy2d, g)


# ---------------------------------------------------------------------------------------------------------------
# Transformer sub-layers (torch.nn.TransformerEncoderLayer / DecoderLayer, post-LN, ReLU; src/module.py:273-274,
# 286-287; exact math SURVEY.md Appendix A)
# ---------------------------------------------------------------------------------------------------------------
def _ln_backward(cx, out, z, mean, rstd, pre_norm, p, seed, stream_id):
    """(dz, dz_dropped-or-dz) of the LayerNorm that produced `out`: already there when the consuming sub-layer's last GEMM ran it in its
    epilogue (out.pre, _input_grad below), otherwise the stand-alone kernel on out.g."""
    if out.pre is not None:
        dz, dzd = out.pre
        out.pre = None
        return dz, (dzd if p > 0 else dz)
    st = cx.st
    dz = _empty(*z.shape, like=z)
    dzd = _empty(*z.shape, like=z) if p > 0 else None
    ops.layernorm_bwd(out.g, z, cx.P[pre_norm + "weight"], mean, rstd, dz, dzd, st.g(pre_norm + "weight"), st.g(pre_norm + "bias"),
                      drop_p=p, seed=seed, stream_id=stream_id)
    return dz, (dzd if p > 0 else dz)


def _input_grad(cx, x, dy2d, W, dz_res):
    """The last GEMM of a sub-layer's backward: dx = dz_res + dy2d @ W, accumulated into x -- or, when x is the output of a LayerNorm
    inside the stack whose only consumer this sub-layer is (x.ln, set by the stack loops) and nothing else has contributed to x.g, that
    LayerNorm's backward in the same launch (ops.linear_dgrad_lnbwd), its result left in x.pre for the producing sub-layer's closure."""
    ln = x.ln
    if ln is not None and x.g is None and x.pre is None:
        z, mean, rstd, pre_norm, p, seed, sid = ln
        st = cx.st
        dz = _empty(*z.shape, like=z)
        dzd = _empty(*z.shape, like=z) if p > 0 else None
        if ops.linear_dgrad_lnbwd(dy2d, W, dz_res, z, mean, rstd, cx.P[pre_norm + "weight"], dz, dzd, st.g(pre_norm + "weight"), st.g(pre_norm + "bias"),
                                  drop_p=p, seed=seed, stream_id=sid):
            x.pre = (dz, dzd)
            return
    dx = _empty(dy2d.shape[0], W.shape[1], like=dy2d)
    ops.linear_dgrad(dy2d, W, dx, R=dz_res)
    acc(x, dx)


def attn_sublayer(cx, tape, x, lens, causal, pre_attn, pre_norm, B, T, H, drop, pad_free_grads=False):
    """y = LN(x + dropout(MHA(x, x)))  with attention-probability dropout `drop` as well (self-attention; cross_attn_sublayer is the
    decoder's other one).  x: Var [B*T, E]."""
    E = x.v.shape[1]
    N = B * T
    W, bias = cx.P[pre_attn + "in_proj_weight"], cx.P[pre_attn + "in_proj_bias"]
    Wo, bo = cx.P[pre_attn + "out_proj.weight"], cx.P[pre_attn + "out_proj.bias"]
    p = cx.p(drop)
    s_attn, s_out = cx.stream(), cx.stream()
    # Q / K / V (and dO below) are read by the attention kernels only: the projections store them pre-split (hi/lo bf16 chunks), so
    # the K/V tiles every query block stages -- and Q / dO in the backward -- need no fp32 -> hi/lo conversion there
    qkv = _empty(N, 3 * E, like=x.v)
    ops.linear_fwd(x.v, W, bias, qkv, out_split=True)
    Q, K, V = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
    O = _empty(N, E, like=x.v)
    LSE = _empty(B, H, T, like=x.v)
    ops.attn_fwd(Q, K, V, O, LSE, lens, B, H, T, T, causal, drop_p=p, seed=cx.seed, stream_id=s_attn, qkv_split=True)
    z = _empty(N, E, like=x.v)
    y, mean, rstd = _empty(N, E, like=x.v), _empty(N, like=x.v), _empty(N, like=x.v)
    # z = x + drop(O Wo^T + bo), y = LayerNorm(z): one launch where the row-panel GEMM serves the shape, GEMM + LayerNorm otherwise
    ops.linear_fwd(O, Wo, bo, z, drop_p=p, seed=cx.seed, stream_id=s_out, R=x.v, ln=(cx.P[pre_norm + "weight"], cx.P[pre_norm + "bias"], y, mean, rstd, LN_EPS))
    out = Var(y)
    if tape is not None:
        seed = cx.seed

        out.ln = (z, mean, rstd, pre_norm, p, seed, s_out)      # (used only while the next sub-layer is its sole consumer: the stack loops clear it on their output)

        def bwd():
            if out.g is None and out.pre is None:
                return
            with ops.wgrad_batch():            # out-proj + in-proj weight gradients: one grouped launch at the end
                st = cx.st
                dz, da = _ln_backward(cx, out, z, mean, rstd, pre_norm, p, seed, s_out)
                gWo = st.g(pre_attn + "out_proj.weight")
                if gWo is not None:
                    ops.linear_wgrad(da, O, gWo, db=st.g(pre_attn + "out_proj.bias"))
                dO = _empty(N, E, like=z)
                ops.linear_dgrad(da, Wo, dO, out_split=True)
                delta = _empty(B, H, T, like=z)
                gW, gb = st.g(pre_attn + "in_proj_weight"), st.g(pre_attn + "in_proj_bias")
                dqkv = _empty(N, 3 * E, like=z)
                ops.attn_bwd(Q, K, V, O, dO, LSE, delta, dqkv[:, :E], dqkv[:, E:2 * E], dqkv[:, 2 * E:], lens, B, H, T, T, causal,
                             drop_p=p, seed=seed, stream_id=s_attn, qkv_split=True, lens_q=lens if (pad_free_grads and config.ENC_SKIP_PAD_GRADS) else None)
                if gW is not None:
                    ops.linear_wgrad(dqkv, x.v, gW, db=gb)
                _input_grad(cx, x, dqkv, W, dz)
        tape.record(bwd)
    return out


def cross_attn_sublayer(cx, tape, x, mems, lens_ks, Tks, pre_attn, pre_norm, B, Tq, H, drop):
    """The cross-attention sub-layer of n decoder calls of one query shape and the same weights (one call, or the auto-encoder's and the
    supervised sub-step's decoder of one generator phase, /root/reference/src/train.py:609-628): y = LN(x + dropout(MHA(x, mem_h))) for
    the n row blocks of x [n B Tq, E] with their own memories mems[h] (Var [B Tk_h, E]).  Everything that does not see the memory runs
    once over all blocks -- the query projection, the out-projection + LayerNorm, their backward GEMMs and weight gradients; the K/V
    projections and the attention core run per block."""
    n = len(mems)
    E = x.v.shape[1]
    N = B * Tq
    blk = lambda t, h: t[h * N:(h + 1) * N]
    W, bias = cx.P[pre_attn + "in_proj_weight"], cx.P[pre_attn + "in_proj_bias"]
    Wo, bo = cx.P[pre_attn + "out_proj.weight"], cx.P[pre_attn + "out_proj.bias"]
    p = cx.p(drop)
    s_attn, s_out = [cx.stream() for _ in range(n)], cx.stream()
    # Q / K / V (and dO below) pre-split for the attention kernels, as in attn_sublayer
    q = _empty(n * N, E, like=x.v)
    ops.linear_fwd(x.v, W[:E], bias[:E], q, out_split=True)
    kvs = []
    for h in range(n):
        kv = _empty(B * Tks[h], 2 * E, like=x.v)
        ops.linear_fwd(mems[h].v, W[E:], bias[E:], kv, out_split=True)
        kvs.append(kv)
    O = _empty(n * N, E, like=x.v)
    LSE = _empty(n, B, H, Tq, like=x.v)
    for h in range(n):
        ops.attn_fwd(blk(q, h), kvs[h][:, :E], kvs[h][:, E:], blk(O, h), LSE[h], lens_ks[h], B, H, Tq, Tks[h], False,
                     drop_p=p, seed=cx.seed, stream_id=s_attn[h], qkv_split=True)
    z = _empty(n * N, E, like=x.v)
    y, mean, rstd = _empty(n * N, E, like=x.v), _empty(n * N, like=x.v), _empty(n * N, like=x.v)
    ops.linear_fwd(O, Wo, bo, z, drop_p=p, seed=cx.seed, stream_id=s_out, R=x.v, ln=(cx.P[pre_norm + "weight"], cx.P[pre_norm + "bias"], y, mean, rstd, LN_EPS))
    out = Var(y)
    if tape is not None:
        seed = cx.seed

        out.ln = (z, mean, rstd, pre_norm, p, seed, s_out)

        def bwd():
            if out.g is None and out.pre is None:
                return
            st = cx.st
            gW, gb = st.g(pre_attn + "in_proj_weight"), st.g(pre_attn + "in_proj_bias")
            dkvs = []
            with ops.wgrad_batch():
                dz, da = _ln_backward(cx, out, z, mean, rstd, pre_norm, p, seed, s_out)
                gWo = st.g(pre_attn + "out_proj.weight")
                if gWo is not None:
                    ops.linear_wgrad(da, O, gWo, db=st.g(pre_attn + "out_proj.bias"))
                dO = _empty(n * N, E, like=z)
                ops.linear_dgrad(da, Wo, dO, out_split=True)
                dq = _empty(n * N, E, like=z)
                for h in range(n):
                    delta = _empty(B, H, Tq, like=z)
                    dkv = _empty(B * Tks[h], 2 * E, like=z)
                    ops.attn_bwd(blk(q, h), kvs[h][:, :E], kvs[h][:, E:], blk(O, h), blk(dO, h), LSE[h], delta,
                                 blk(dq, h), dkv[:, :E], dkv[:, E:], lens_ks[h], B, H, Tq, Tks[h], False,
                                 drop_p=p, seed=seed, stream_id=s_attn[h], qkv_split=True)
                    dkvs.append(dkv)
                    dmem = _empty(B * Tks[h], E, like=z)
                    ops.linear_dgrad(dkv, W[E:], dmem)
                    acc(mems[h], dmem)
                if gW is not None:
                    ops.linear_wgrad(dkvs[0], mems[0].v, gW[E:], db=gb[E:])
                    ops.linear_wgrad(dq, x.v, gW[:E], db=gb[:E])
                _input_grad(cx, x, dq, W[:E], dz)           # (contraction over 256: the K-streamed kernel does not serve it; plain path)
            # the later memories' K/V weight gradients accumulate into the SAME rows of in_proj_weight as the first's: the problems of a
            # grouped launch run side by side, so they go out on their own, behind the group (same stream: ops keeps a gradient buffer's stream)
            if gW is not None:
                for h in range(1, n):
                    ops.linear_wgrad(dkvs[h], mems[h].v, gW[E:], db=gb[E:])
        tape.record(bwd)
    return out


def ffn_sublayer(cx, tape, x, pre, pre_norm, drop):
    """y = LN(x + dropout(W2 dropout(relu(W1 x + b1)) + b2))."""
    N, E = x.v.shape
    W1, b1, W2, b2 = cx.P[pre + "linear1.weight"], cx.P[pre + "linear1.bias"], cx.P[pre + "linear2.weight"], cx.P[pre + "linear2.bias"]
    F = W1.shape[0]
    p = cx.p(drop)
    s1, s2 = cx.stream(), cx.stream()
    h = _empty(N, F, like=x.v)
    # keep bits of h (relu > 0 and not dropped) for the backward's gate, when both GEMMs that touch them run on the row-panel kernel
    bits = None
    if tape is not None and F % 64 == 0 and F <= 1024 and ops.panel_serves(N, E, W1) and ops.panel_serves(N, E, W2, transposed=True):
        bits = torch.empty(ops.gate_bits_bytes(N, F), dtype=torch.uint8, device=x.v.device)
    ops.linear_fwd(x.v, W1, b1, h, act=1, drop_p=p, seed=cx.seed, stream_id=s1, gate_bits=bits)
    z = _empty(N, E, like=x.v)
    y, mean, rstd = _empty(N, E, like=x.v), _empty(N, like=x.v), _empty(N, like=x.v)
    ops.linear_fwd(h, W2, b2, z, drop_p=p, seed=cx.seed, stream_id=s2, R=x.v, ln=(cx.P[pre_norm + "weight"], cx.P[pre_norm + "bias"], y, mean, rstd, LN_EPS))
    out = Var(y)
    if tape is not None:
        seed = cx.seed

        out.ln = (z, mean, rstd, pre_norm, p, seed, s2)

        def bwd():
            if out.g is None and out.pre is None:
                return
            with ops.wgrad_batch():            # linear2 + linear1 weight gradients: one grouped launch at the end
                bwd_body()

        def bwd_body():
            st = cx.st
            dz, da = _ln_backward(cx, out, z, mean, rstd, pre_norm, p, seed, s2)
            g2 = st.g(pre + "linear2.weight")
            if g2 is not None:
                ops.linear_wgrad(da, h, g2, db=st.g(pre + "linear2.bias"))
            du = _empty(N, F, like=z)
            gsc = 1.0 / (1.0 - p) if p > 0 else 1.0
            if bits is not None:
                ops.linear_dgrad(da, W2, du, gate_bits=bits, gate_scale=gsc)                      # relu' and dropout mask from the keep bits
            else:
                ops.linear_dgrad(da, W2, du, G=h, gate_scale=gsc)                                 # ... from h > 0
            g1 = st.g(pre + "linear1.weight")
            if g1 is not None:
                ops.linear_wgrad(du, x.v, g1, db=st.g(pre + "linear1.bias"))
            _input_grad(cx, x, du, W1, dz)
        tape.record(bwd)
    return out


def encoder_stack(cx, tape, x, lens, pre, L, B, T, H, drop):
    """src/module.py:270-280 (TransformerEncoder): all-False attn mask + key padding mask."""
    for i in range(L):
        lp = "%s%d." % (pre, i)
        x = attn_sublayer(cx, tape, x, lens, False, lp + "self_attn.", lp + "norm1.", B, T, H, drop, pad_free_grads=True)
        x = ffn_sublayer(cx, tape, x, lp, lp + "norm2.", drop)
    x.ln = None                 # the stack's output has consumers outside it (decoder memory, discriminator): plain LayerNorm backward
    return x


def decoder_stack(cx, tape, x, lens_q, mems, lens_ks, Tks, pre, L, B, Tq, H, drop):
    """src/module.py:283-293 (TransformerDecoder) over the n = len(mems) calls of one query shape whose rows x holds [n B Tq, E]: causal +
    tgt padding self-attention and the feed-forward block over n B sequences, memory-padding cross-attention per call on its own memory."""
    n = len(mems)
    for i in range(L):
        lp = "%s%d." % (pre, i)
        x = attn_sublayer(cx, tape, x, lens_q, True, lp + "self_attn.", lp + "norm1.", n * B, Tq, H, drop)
        x = cross_attn_sublayer(cx, tape, x, mems, lens_ks, Tks, lp + "multihead_attn.", lp + "norm2.", B, Tq, H, drop)
        x = ffn_sublayer(cx, tape, x, lp, lp + "norm3.", drop)
    x.ln = None                 # the stack's output has consumers outside it: its LayerNorm backward stays a launch of its own
    return x


def _row_block_tails(tape, y, n, tail):
    """[tail(h, x_h, dx_out_h)] for the n row blocks x_h of a decoder stack's output y (Var [n N, E]).  The tails write their input gradient
    into row blocks of ONE buffer (dx_out_h() hands out block h), which goes to the stack as it is: with one block the tail's gradient is
    the buffer, and nothing is launched here."""
    N, E = y.v.shape[0] // n, y.v.shape[1]
    gbuf = {}
    xs = [Var(y.v[h * N:(h + 1) * N]) for h in range(n)]
    if tape is not None:
        def join():                                   # recorded before the tails => runs after them: hand the buffer to the stack
            if "g" in gbuf:
                for h in range(n):
                    blk = gbuf["g"][h * N:(h + 1) * N]
                    if xs[h].g is None:
                        blk.zero_()
                    elif xs[h].g.data_ptr() != blk.data_ptr():
                        ops.sum2(blk, xs[h].g.contiguous())
                acc(y, gbuf["g"])
        tape.record(join)

    def dx_block(h):
        def get():
            if "g" not in gbuf:
                gbuf["g"] = _empty(n * N, E, like=y.v)
            return gbuf["g"][h * N:(h + 1) * N]
        return get
    return [tail(h, xs[h], dx_block(h)) for h in range(n)]


# ---------------------------------------------------------------------------------------------------------------
# Positional encoding (src/module.py:249-267; dropout fixed at 0.1)
# ---------------------------------------------------------------------------------------------------------------
def posenc(cx, tape, x, pe, T, gate=None, out=None):
    """out: an [N, Dm] row block of a larger buffer that receives the result (the blocks of an n-ary encoder / decoder call)."""
    N, Dm = x.v.shape
    p = cx.p(0.1)
    s = cx.stream()
    y = out if out is not None else _empty(N, Dm, like=x.v)
    scale = math.sqrt(Dm)
    ops.posenc_fwd(x.v, pe, y, T, scale, drop_p=p, seed=cx.seed, stream_id=s)
    out = Var(y)
    if tape is not None:
        seed = cx.seed

        def bwd():
            if out.g is None:
                return
            dx = _empty(N, Dm, like=y)
            ops.posenc_bwd(out.g, gate, dx, scale, drop_p=p, seed=seed, stream_id=s)
            acc(x, dx)
        tape.record(bwd)
    return out


# ---------------------------------------------------------------------------------------------------------------
# Text side
# ---------------------------------------------------------------------------------------------------------------
class ZeroPool:
    """fp64 scratch of a whole conv + BatchNorm stack, zeroed by ONE fill launch: per stage 2C doubles for the conv GEMM's column
    sums (forward) and 2C for the backward's reduction -- instead of a fill per stage and pass (17 + 14 launches per step)."""

    def __init__(self, stages, C, device):
        self.buf = torch.zeros(stages * 4 * C, dtype=torch.float64, device=device)
        self.C, self.i = C, 0

    def take(self, Cout):
        if Cout != self.C or (self.i + 1) * 4 * self.C > self.buf.numel():
            return torch.zeros(4 * Cout, dtype=torch.float64, device=self.buf.device)
        w = self.buf[self.i * 4 * self.C:(self.i + 1) * 4 * self.C]
        self.i += 1
        return w


def conv_bn_act(cx, tape, x, B, T, conv_pre, bn_pre, pad_left, act, drop, bn_buffers, pool=None):
    """dropout(act(BN_train(conv1d_k5(x)))) — one stage of TextPrenet.forward_fcn / SpeechPostnet.forward
    (src/module.py:162-165, 223-230).  x: Var [B*T, Cin]."""
    Wp, b = cx.P[conv_pre + "conv.weight"], cx.P[conv_pre + "conv.bias"]
    Cout, _, Cin = Wp.shape
    x3 = x.v.view(B, T, -1)[..., :Cin] if x.v.shape[1] != Cin else x.v.view(B, T, Cin)
    c = _empty(B, T, Cout, like=x.v)
    # [0, 2C): sum / sum of squares per channel out of the conv GEMM's epilogue; [2C, 4C): the backward's column sums (both pre-zeroed)
    ws4 = pool.take(Cout) if (pool is not None and cx.training) else torch.zeros(4 * Cout, dtype=torch.float64, device=x.v.device)
    ws, ws_b = ws4[:2 * Cout], ws4[2 * Cout:]
    ops.conv_fwd(x3, Wp, b, c, pad_left, colstats=ws if cx.training else None)
    p = cx.p(drop)
    s = cx.stream()
    N = B * T
    y = _empty(N, Cout, like=x.v)
    mean, rstd = _empty(Cout, like=x.v), _empty(Cout, like=x.v)
    rm, rv = bn_buffers[bn_pre + "running_mean"], bn_buffers[bn_pre + "running_var"]
    gamma, beta = cx.P[bn_pre + "weight"], cx.P[bn_pre + "bias"]
    if cx.training:
        ops.bn_fwd(c.view(N, Cout), gamma, beta, y, mean, rstd, rm, rv, ws, act, drop_p=p, seed=cx.seed, stream_id=s, have_sums=True,
                   num_batches_tracked=bn_buffers[bn_pre + "num_batches_tracked"])
    else:
        if tape is not None:
            raise NotImplementedError("eval-mode BatchNorm has no backward on this path; evaluate() runs under torch.no_grad()")
        ops.bn_eval_fwd(c.view(N, Cout), gamma, beta, rm, rv, y, mean, rstd, act)
    out = Var(y)
    if tape is not None:
        seed = cx.seed

        def bwd():
            if out.g is None:
                return
            st = cx.st
            dy = out.g if out.g.is_contiguous() else out.g.contiguous()
            dc = _empty(N, Cout, like=y)
            ops.bn_bwd(dy, c.view(N, Cout), mean, rstd, gamma, beta, dc, st.g(bn_pre + "weight"), st.g(bn_pre + "bias"), ws_b, act,
                       drop_p=p, seed=seed, stream_id=s, ws_zeroed=True)
            gW = st.g(conv_pre + "conv.weight")
            dc3 = dc.view(B, T, Cout)
            if gW is not None:
                ops.conv_wgrad(dc3, x3, gW, pad_left, db=st.g(conv_pre + "conv.bias"))
            dx = _empty(B, T, Cin, like=y)
            ops.conv_dgrad(dc3, Wp, dx, pad_left)
            acc(x, dx.view(N, Cin))
        tape.record(bwd)
    return out


def text_embed(cx, tape, ids, T, drop, noise, shift_sos):
    """prenet.emb_dropout(prenet.embed(ids)) [+ noise_fn]  (src/network.py:427-438); shift_sos builds [SOS, ids[:-1]]."""
    E = cx.P["text_m.prenet.embed.weight"]
    N = ids.numel()
    p = cx.p(drop)
    pn = 0.3 if (noise and cx.noisy) else 0.0
    s, sn = cx.stream(), cx.stream()
    y = _empty(N, E.shape[1], device=E.device)
    ops.embed_fwd(ids, E, y, T, shift_sos=shift_sos, drop_p=p, seed=cx.seed, stream_id=s, noise_p=pn, noise_stream=sn)
    out = Var(y)
    if tape is not None:
        seed = cx.seed

        def bwd():
            gE = cx.st.g("text_m.prenet.embed.weight")
            if out.g is None or gE is None:
                return
            ops.embed_bwd(ids, out.g, gE, T, shift_sos=shift_sos, drop_p=p, seed=seed, stream_id=s, noise_p=pn, noise_stream=sn)
        tape.record(bwd)
    return out


def text_frontend(cx, tape, m, ids, noise, out=None):
    """Embedding (+ noise_fn), the three conv + BatchNorm + ReLU stages and the positional encoding in front of the text encoder stack
    (src/network.py:427-434): everything of TextTransformer.encode that sees the batch as a whole (BatchNorm statistics)."""
    B, T = ids.shape
    a = m.args
    x = text_embed(cx, tape, ids, T, a.t_pre_drop, noise, -1)
    pool = ZeroPool(3, cx.P["text_m.prenet.conv1.conv.weight"].shape[0], ids.device) if cx.training else None
    for i in (1, 2, 3):
        x = conv_bn_act(cx, tape, x, B, T, "text_m.prenet.conv%d." % i, "text_m.prenet.batch_norm%d." % i, 2, 1, a.t_pre_drop, m.buffers_dict, pool=pool)
    return posenc(cx, tape, x, m.pe, T, out=out)


def _stack_rows(cx, tape, blocks, buf):
    """Var over `buf` [n N, E], whose n row blocks the front ends of an n-ary encoder / decoder call have just written (posenc out=): the
    gradient that comes back for the whole buffer is handed to the blocks as row-block views (no copy either way)."""
    x = Var(buf)
    if tape is not None:
        N = blocks[0].v.shape[0]

        def bwd():
            if x.g is None:
                return
            for i, h in enumerate(blocks):
                acc(h, x.g[i * N:(i + 1) * N])
        tape.record(bwd)                                # recorded after the blocks' own closures => runs before them
    return x


def text_encode(cx, tape, m, ids, noises, lens):
    """TextTransformer.encode (src/network.py:427-444) of the n batches `ids` of one shape (one call; or the auto-encoder's and the
    supervised sub-step's of one generator phase, same weights: /root/reference/src/train.py:609-628) with the encoder stack run ONCE over
    n B sequences (`lens`: their n B lengths).  What the reference keeps per call stays per block: the conv front end with its BatchNorm
    batch statistics and running-stat updates (in call order), the dropout / noise streams.  Returns the stack's output Var [n B T, E]."""
    n = len(ids)
    B, T = ids[0].shape
    a = m.args
    E = cx.P["text_m.prenet.embed.weight"].shape[1]
    buf = _empty(n * B * T, E, device=ids[0].device)
    blocks = [text_frontend(cx, tape, m, ids[h], noises[h], out=buf[h * B * T:(h + 1) * B * T]) for h in range(n)]
    x = _stack_rows(cx, tape, blocks, buf)
    return encoder_stack(cx, tape, x, lens, "text_m.encoder.transformer_encoder.layers.", a.num_layers, n * B, T, a.nhead, a.e_drop)


FUSED_STATS = {"text_head": 0, "text_grad_direct": 0, "text_grad_general": 0, "speech_head": 0, "speech_grad_direct": 0, "speech_grad_general": 0}      # launches so far (tests)


def _hint_conforms(dev, eos_w, gscale, *tensors):
    """Whether a loss_hint holds what the fused head + loss kernels read through raw pointers: every (tensor, dtype, elements) contiguous on
    `dev` with that dtype and element count, eos_weight and gscale finite."""
    return math.isfinite(float(eos_w)) and math.isfinite(float(gscale)) and all(
        torch.is_tensor(t) and t.dtype == dt and t.device == dev and t.numel() == n and t.is_contiguous() for t, dt, n in tensors)


def text_decode(cx, tape, m, ids, lens_q, mems, lens_ks, Tks, shift=True, loss_hints=None):
    """TextTransformer.decode_sequence (src/network.py:483-493) incl. TextPostnet (src/module.py:233-246) of the n calls `ids` of one
    target shape (one call; or the auto-encoder's text decoder and the ASR decoder of one generator phase): embeddings + positional
    encoding per call into one buffer, the decoder stack once over all, TextPostnet head + loss per call.
    Returns the n Var logits buffers [B*T, 48] (46 valid columns).  shift=False: `ids` are the decoder inputs as they are
    (TextTransformer.decode, src/network.py:446-450)."""
    n = len(ids)
    B, T = ids[0].shape
    a = m.args
    N = B * T
    E = cx.P["text_m.prenet.embed.weight"].shape[1]
    buf = _empty(n * N, E, device=ids[0].device)
    blocks = [posenc(cx, tape, text_embed(cx, tape, ids[h], T, a.t_pre_drop, False, 1 if shift else -1), m.pe, T, out=buf[h * N:(h + 1) * N])
              for h in range(n)]                                                        # SOS_IDX = 1
    x = _stack_rows(cx, tape, blocks, buf)
    y = decoder_stack(cx, tape, x, lens_q, mems, lens_ks, Tks, "text_m.decoder.transformer_decoder.layers.", a.num_layers, B, T, a.nhead, a.d_drop)
    hints = loss_hints or [None] * n
    return _row_block_tails(tape, y, n, lambda h, xh, dx_out: text_decode_tail(cx, tape, m, xh, loss_hint=hints[h], dx_out=dx_out))


def text_decode_tail(cx, tape, m, x, loss_hint=None, dx_out=None):
    """TextPostnet (dropout + fc1, src/module.py:233-246) on decoder states x (Var [B*T, E]), with the loss in the head's launch when the
    step announced it.  dx_out: where the backward puts d(loss)/dx (_row_block_tails)."""
    a = m.args
    N, E = x.v.shape
    p = cx.p(a.t_post_drop)
    s = cx.stream()
    if p > 0:
        xd = _empty(N, E, like=x.v)
        ops.leaky_dropout(x.v, None, xd, 1.0, drop_p=p, seed=cx.seed, stream_id=s)
    else:
        xd = x.v
    W, b = cx.P["text_m.postnet.fc1.weight"], cx.P["text_m.postnet.fc1.bias"]
    V = W.shape[0]
    ldl = (V + 3) // 4 * 4
    logits = None
    if loss_hint is not None and tape is not None and E == 256 and V <= 48:
        # loss_hint = (gold [B, T] int64, eos_weight, gscale, loss workspace): head GEMM, cross-entropy and its gradient in one launch, unless
        # the kernel could misread the hint.  The record rides on the logits buffer: train.text_loss takes it off through its input's view
        # base, and it is freed with the buffer
        gold, eos_w, gscale, ws = loss_hint
        goldc = gold.contiguous().view(-1)
        if _hint_conforms(x.v.device, eos_w, gscale, (goldc, torch.int64, N), (ws, torch.float64, 8)):
            logits = torch.empty(N, ldl, dtype=torch.float32, device=x.v.device)
            dlogits = torch.empty(N, ldl, dtype=torch.float32, device=x.v.device)
            loss = torch.empty(1, dtype=torch.float32, device=x.v.device)
            ops.text_head_loss(xd, W, b, goldc, V, eos_w, gscale, logits, dlogits, ws, loss)
            FUSED_STATS["text_head"] += 1
            logits.fused_loss = dict(kind="text", loss=loss, dlogits=dlogits, gold=goldc, eos_weight=float(eos_w), gscale=float(gscale), ws=ws)
    if logits is None:
        logits = torch.zeros(N, ldl, dtype=torch.float32, device=x.v.device)
        ops.linear_fwd(xd, W, b, logits[:, :V])
    out = Var(logits)
    if tape is not None:
        seed = cx.seed

        def bwd():
            if out.g is None:
                return
            st = cx.st
            dl = out.g
            gW = st.g("text_m.postnet.fc1.weight")
            if gW is not None:
                ops.linear_wgrad(dl[:, :V], xd, gW, db=st.g("text_m.postnet.fc1.bias"))
            last = dx_out() if dx_out is not None else None
            dxd = last if (last is not None and p <= 0) else _empty(N, E, like=xd)
            ops.linear_dgrad(dl[:, :V], W, dxd)
            if p > 0:
                dx = last if last is not None else _empty(N, E, like=xd)
                ops.leaky_dropout(x.v, dxd, dx, 1.0, drop_p=p, seed=seed, stream_id=s)
            else:
                dx = dxd
            acc(x, dx)
        tape.record(bwd)
    return out


# ---------------------------------------------------------------------------------------------------------------
# Speech side
# ---------------------------------------------------------------------------------------------------------------
def speech_prenet(cx, tape, m, mel2d, T, out=None):
    """SpeechPrenet (src/module.py:76-110; ONE dropout) followed by PositionalEncoding."""
    a = m.args
    N = mel2d.shape[0]
    W1, b1 = cx.P["speech_m.prenet.layer.fc1.linear_layer.weight"], cx.P["speech_m.prenet.layer.fc1.linear_layer.bias"]
    W2, b2 = cx.P["speech_m.prenet.layer.fc2.linear_layer.weight"], cx.P["speech_m.prenet.layer.fc2.linear_layer.bias"]
    p = cx.p(a.s_pre_drop)
    s = cx.stream()
    h1 = _empty(N, W1.shape[0], like=mel2d)
    ops.linear_fwd(mel2d, W1, b1, h1, act=1, drop_p=p, seed=cx.seed, stream_id=s)
    h2 = _empty(N, W2.shape[0], like=mel2d)
    ops.linear_fwd(h1, W2, b2, h2, act=1)
    h2v = Var(h2)
    if tape is not None:
        def bwd():
            st = cx.st
            d2 = h2v.g                                  # already gated by relu'(h2) in posenc's backward
            g2 = st.g("speech_m.prenet.layer.fc2.linear_layer.weight")
            if d2 is None or g2 is None:
                return
            ops.linear_wgrad(d2, h1, g2, db=st.g("speech_m.prenet.layer.fc2.linear_layer.bias"))
            du = _empty(N, W1.shape[0], like=h1)
            ops.linear_dgrad(d2, W2, du, G=h1, gate_scale=(1.0 / (1.0 - p) if p > 0 else 1.0))
            ops.linear_wgrad(du, mel2d, st.g("speech_m.prenet.layer.fc1.linear_layer.weight"), db=st.g("speech_m.prenet.layer.fc1.linear_layer.bias"))
        tape.record(bwd)                                # recorded before posenc's closure => runs after it
    y = posenc(cx, tape, h2v, m.pe, T, gate=h2, out=out)
    return y


def speech_frontend(cx, tape, m, mel, noise, out=None):
    """noise_fn on the raw mel, SpeechPrenet and the positional encoding in front of the speech encoder stack (src/network.py:203-206)."""
    B, T, M = mel.shape
    mel2d = mel.reshape(B * T, M)
    if noise and cx.noisy:
        noised = _empty(B * T, M, like=mel2d)
        ops.rowmask(mel2d, noised, 0.3, cx.seed, cx.stream())
        mel2d = noised
    return speech_prenet(cx, tape, m, mel2d, T, out=out)


def speech_encode(cx, tape, m, mels, noises, lens):
    """SpeechTransformer.encode (src/network.py:203-208) of the n batches `mels` of one shape with the encoder stack run once over n B
    sequences (see text_encode; the speech front end has no batch statistics, its dropout / noise streams stay per call)."""
    n = len(mels)
    B, T, M = mels[0].shape
    a = m.args
    E = cx.P["speech_m.prenet.layer.fc2.linear_layer.weight"].shape[0]
    buf = _empty(n * B * T, E, like=mels[0])
    blocks = [speech_frontend(cx, tape, m, mels[h], noises[h], out=buf[h * B * T:(h + 1) * B * T]) for h in range(n)]
    x = _stack_rows(cx, tape, blocks, buf)
    return encoder_stack(cx, tape, x, lens, "speech_m.encoder.transformer_encoder.layers.", a.num_layers, n * B, T, a.nhead, a.e_drop)


def speech_decode_front(cx, tape, m, mel, shift=True, out=None):
    """The decoder input of SpeechTransformer.decode_sequence: go-frame shift (src/network.py:254-262), SpeechPrenet, positional encoding."""
    B, T, M = mel.shape
    N = B * T
    if shift:
        if M % 4 == 0 and mel.is_contiguous() and mel.data_ptr() % 16 == 0:
            tgt = ops.shift_frames(mel, torch.empty_like(mel))      # [zero frame, mel[:-1]] in one launch
        else:
            tgt = torch.zeros_like(mel)
            tgt[:, 1:] = mel[:, :-1]
    else:
        tgt = mel.contiguous()
    return speech_prenet(cx, tape, m, tgt.view(N, M), T, out=out)


def speech_decode(cx, tape, m, mels, lens_q, mems, lens_ks, Tks, shift=True, postnet=True, loss_hints=None):
    """SpeechTransformer.decode_sequence (src/network.py:254-269) + SpeechPostnet (src/module.py:155-171) of the n calls `mels` of one
    target shape (one call; or the auto-encoder's and the TTS decoder of one generator phase): front ends per call into one buffer, the
    decoder stack once over all, heads + post-net + loss terms per call (the post-net's BatchNorm statistics stay per call, in call order).
    Returns per call (head Var [B*T, 84]: cols 0..79 pre-net mel, col 80 stop logit; post Var [B*T, 80]).
    shift=False feeds `mels` as the decoder input as they are, postnet=False stops at the heads (SpeechTransformer.decode,
    src/network.py:210-214; no tape)."""
    n = len(mels)
    B, T, M = mels[0].shape
    a = m.args
    N = B * T
    E = cx.P["speech_m.prenet.layer.fc2.linear_layer.weight"].shape[0]
    buf = _empty(n * N, E, like=mels[0])
    blocks = [speech_decode_front(cx, tape, m, mels[h], shift, out=buf[h * N:(h + 1) * N]) for h in range(n)]
    x = _stack_rows(cx, tape, blocks, buf)
    y = decoder_stack(cx, tape, x, lens_q, mems, lens_ks, Tks, "speech_m.decoder.transformer_decoder.layers.", a.num_layers, B, T, a.nhead, a.d_drop)
    hints = loss_hints or [None] * n
    return _row_block_tails(tape, y, n, lambda h, xh, dx_out: speech_decode_tail(cx, tape, m, xh, mels[h], postnet=postnet, loss_hint=hints[h], dx_out=dx_out))


def _postnet_convs(cx, tape, m, x, B, T, pool=None):
    """The four conv + BatchNorm + tanh stages of SpeechPostnet (src/module.py:155-171) on x (Var [B*T, >= num_mels]); `pool`: their fp64
    scratch where the caller keeps one (ZeroPool)."""
    y = conv_bn_act(cx, tape, x, B, T, "speech_m.postnet.conv1.", "speech_m.postnet.pre_batchnorm.", 4, 2, m.args.s_post_drop, m.buffers_dict, pool=pool)
    for i in range(3):
        y = conv_bn_act(cx, tape, y, B, T, "speech_m.postnet.conv_list.%d." % i, "speech_m.postnet.batch_norm_list.%d." % i, 4, 2,
                        m.args.s_post_drop, m.buffers_dict, pool=pool)
    return y


def speech_decode_tail(cx, tape, m, x, mel, postnet=True, loss_hint=None, dx_out=None):
    """The heads ([linear_project | stop_linear]) and the SpeechPostnet on decoder states x (Var [B*T, E]); mel only gives shapes / device.
    dx_out: where the backward puts d(loss)/dx (_row_block_tails) instead of a buffer of its own."""
    B, T, M = mel.shape
    N = B * T
    E = x.v.shape[1]
    st = cx.st
    Wh = st.span("speech_m.postnet.linear_project.weight", "speech_m.postnet.stop_linear.weight", (M + 1, E))
    bh = st.span("speech_m.postnet.linear_project.bias", "speech_m.postnet.stop_linear.bias", (M + 1,))
    ldh = (M + 1 + 3) // 4 * 4
    fused = None
    if loss_hint is not None and tape is not None and postnet and E == 256 and M % 4 == 0 and M + 1 <= 96 and \
            Wh.data_ptr() % 16 == 0 and bh.data_ptr() % 16 == 0:
        # loss_hint = (gold mel [B, T, M] float32, lengths [B], eos_weight, gscale, loss workspace): the heads, the pre-net MSE, the stop BCE and
        # their gradient in one launch, unless the kernel could misread the hint; the post-net term and the scalar follow behind the post-net
        # (speech_post_loss below)
        gold, glens, eos_w, gscale, ws = loss_hint
        goldc, glens = gold.contiguous(), lens_i32(glens, mel.device)
        if _hint_conforms(mel.device, eos_w, gscale, (goldc, torch.float32, N * M), (glens, torch.int32, B), (ws, torch.float64, 8)):
            head = torch.empty(N, ldh, dtype=torch.float32, device=mel.device)
            d_head = torch.empty(N, ldh, dtype=torch.float32, device=mel.device)
            ops.speech_head_loss(x.v, Wh, bh, goldc.view(N, M), glens, B, T, M, eos_w, gscale, head, d_head, ws)
            FUSED_STATS["speech_head"] += 1
            fused = dict(kind="speech", gold=goldc, lens=glens, eos_weight=float(eos_w), gscale=float(gscale), ws=ws, d_head=d_head)
    if fused is None:
        head = torch.zeros(N, ldh, dtype=torch.float32, device=mel.device)
        ops.linear_fwd(x.v, Wh, bh, head[:, :M + 1])
    headv = Var(head)
    pre = Var(head)                                                 # postnet input = columns [0,M) of head (row stride ldh)
    postv = Var(None)
    if tape is not None:
        def bwd_head():
            # d(head) = loss part (headv.g) + postnet-input part (pre.g, [N,M]) + residual part of post = pre + postnet(pre)
            dh = headv.g
            if dh is None:
                dh = torch.zeros(N, ldh, dtype=torch.float32, device=mel.device)
            if pre.g is not None:
                ops.add_strided(dh, pre.g, M)
            if postv.g is not None:
                ops.add_strided(dh, postv.g, M)
            gW = st.gspan("speech_m.postnet.linear_project.weight", "speech_m.postnet.stop_linear.weight", (M + 1, E))
            if gW is not None:
                ops.linear_wgrad(dh[:, :M + 1], x.v, gW, db=st.gspan("speech_m.postnet.linear_project.bias", "speech_m.postnet.stop_linear.bias", (M + 1,)))
            dx = dx_out() if dx_out is not None else _empty(N, E, like=x.v)
            ops.linear_dgrad(dh[:, :M + 1], Wh, dx)
            acc(x, dx)
        tape.record(bwd_head)                                       # runs after every postnet closure
    if not postnet:
        return headv, None
    pool = ZeroPool(4, cx.P["speech_m.postnet.conv1.conv.weight"].shape[0], mel.device) if cx.training else None
    y = _postnet_convs(cx, tape, m, pre, B, T, pool=pool)
    Wp2, b2 = cx.P["speech_m.postnet.conv2.conv.weight"], cx.P["speech_m.postnet.conv2.conv.bias"]
    post = _empty(B, T, M, like=mel)
    C = y.v.shape[1]
    ops.gemm(ops.OP_KC_CONV, ops.OP_KC, y.v, C, Wp2, 5 * C, post, M, N, M, 5 * C, conv=(T, C, 0, 4), bias=b2, R=head, ldr=ldh)   # + residual pre
    postv.v = post.view(N, M)
    if fused is not None:
        fused["d_post"] = torch.empty(B, T, M, dtype=torch.float32, device=mel.device)
        fused["loss"] = torch.empty(1, dtype=torch.float32, device=mel.device)
        ops.speech_post_loss(fused["gold"].view(N, M), postv.v, fused["lens"], B, T, M, fused["gscale"], fused["d_post"], fused["ws"], fused["loss"])
        head.fused_loss = fused                                     # for train.speech_loss, through its pred_mel's view base (see text_decode_tail)
    if tape is not None:
        def bwd_conv2():
            if postv.g is None:
                return
            dp = postv.g if postv.g.is_contiguous() else postv.g.contiguous()
            postv.g = dp
            gW = st.g("speech_m.postnet.conv2.conv.weight")
            dp3 = dp.view(B, T, M)
            if gW is not None:
                ops.conv_wgrad(dp3, y.v.view(B, T, C), gW, 4, db=st.g("speech_m.postnet.conv2.conv.bias"))
            dy = _empty(B, T, C, like=dp)
            ops.conv_dgrad(dp3, Wp2, dy, 4)
            acc(y, dy.view(N, C))
        tape.record(bwd_conv2)                                      # recorded last => runs first
    return headv, postv


# ---------------------------------------------------------------------------------------------------------------
# LSTM discriminator (src/network.py:172-186, src/module.py:297-336)
# ---------------------------------------------------------------------------------------------------------------
def lstm_discriminator(cx, tape, m, x, lens, Bd, T, need_input_grad=True):
    """x: Var [Bd*T, d_in] (zero padded), lens int32 [Bd].  Returns Var logits buffer [Bd, 4] (column 0 valid)."""
    st = cx.st
    Hh, L, ndir = m.hidden, m.num_layers, m.num_dir
    G4 = 4 * Hh
    dev = x.v.device
    p_inter = cx.p(m.dropout_p) if L > 1 else 0.0
    saved = []
    inp = x
    hfin = None
    for l in range(L):
        names = ["discriminator.rnn.rnn.%s_l%d" % (k, l) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        last = [n + ("_reverse" if ndir == 2 else "") for n in names]
        din = inp.v.shape[1]
        Wih = st.span(names[0], last[0], (ndir * G4, din))
        Whh = st.span(names[1], last[1], (ndir * G4, Hh))
        bih = st.span(names[2], last[2], (ndir * G4,))
        bhh = st.span(names[3], last[3], (ndir * G4,))
        xproj = _empty(Bd * T, ndir * G4, device=dev)
        ops.linear_fwd(inp.v, Wih, None, xproj)
        y = _empty(Bd, T, ndir * Hh, device=dev)                          # (the recurrence kernels write zeros at the padded steps themselves)
        gates = _empty(Bd, T, ndir, G4, device=dev)
        cs = _empty(Bd, T, ndir, Hh, device=dev)
        hprev = _empty(Bd, T, ndir, Hh, device=dev)
        hfin = _empty(Bd, ndir * Hh, device=dev)
        ops.lstm_fwd(xproj.view(Bd, T, ndir * G4), Whh, bih, bhh, lens, y, gates, cs, hprev, hfin, ndir, G4 * Hh, G4)
        yv = Var(y.view(Bd * T, ndir * Hh))
        rec = dict(l=l, names=names, last=last, Wih=Wih, Whh=Whh, inp=inp, y=yv, gates=gates, cs=cs, hprev=hprev, din=din, drop=None)
        saved.append(rec)
        if l + 1 < L:
            if p_inter > 0:
                s = cx.stream()
                yd = _empty(Bd * T, ndir * Hh, device=dev)
                ops.leaky_dropout(yv.v, None, yd, 1.0, drop_p=p_inter, seed=cx.seed, stream_id=s)
                rec["drop"] = s
                inp = Var(yd)
                rec["next_in"] = inp
            else:
                inp = yv
                rec["next_in"] = inp
    # head: reduce_h_W on [h_fwd | h_bwd] of the top layer -> LeakyReLU -> Dropout -> fc2
    p_head = cx.p(m.dropout_p)
    if ndir == 2:
        Wr, br = cx.P["discriminator.rnn.reduce_h_W.weight"], cx.P["discriminator.rnn.reduce_h_W.bias"]
        r = _empty(Bd, Hh, device=dev)
        ops.linear_fwd(hfin, Wr, br, r)
    else:
        r = hfin
    s_head = cx.stream()
    a = _empty(Bd, Hh, device=dev)
    ops.leaky_dropout(r, None, a, m.relu_slope, drop_p=p_head, seed=cx.seed, stream_id=s_head)
    W2, b2 = cx.P["discriminator.fc2.weight"], cx.P["discriminator.fc2.bias"]
    logit = torch.zeros(Bd, 4, dtype=torch.float32, device=dev)
    ops.linear_fwd(a, W2, b2, logit[:, :1])
    out = Var(logit)
    if tape is not None:
        seed = cx.seed

        def bwd():
            if out.g is None:
                return
            with ops.wgrad_batch():            # the input-projection gradients of both LSTM layers: one grouped launch
                bwd_body()

        def bwd_body():
            dl = out.g                                             # [Bd,4], column 0 valid
            g2 = st.g("discriminator.fc2.weight")
            if g2 is not None:
                ops.linear_wgrad(dl[:, :1], a, g2, db=st.g("discriminator.fc2.bias"))
            da = _empty(Bd, Hh, device=dev)
            ops.linear_dgrad(dl[:, :1], W2, da)
            dr = _empty(Bd, Hh, device=dev)
            ops.leaky_dropout(r, da, dr, m.relu_slope, drop_p=p_head, seed=seed, stream_id=s_head)
            if ndir == 2:
                gr = st.g("discriminator.rnn.reduce_h_W.weight")
                if gr is not None:
                    ops.linear_wgrad(dr, hfin, gr, db=st.g("discriminator.rnn.reduce_h_W.bias"))
                dhf = _empty(Bd, ndir * Hh, device=dev)
                ops.linear_dgrad(dr, Wr, dhf)
            else:
                dhf = dr
            dy = None
            for rec in reversed(saved):
                dg = _empty(Bd, T, ndir, G4, device=dev)
                ops.lstm_bwd(dy, dhf, rec["Whh"], rec["gates"], rec["cs"], lens, dg, ndir, G4 * Hh)
                dhf = None                                          # only the top layer's final state feeds the head
                dg2 = dg.view(Bd * T, ndir * G4)
                names, last = rec["names"], rec["last"]
                gWih = st.gspan(names[0], last[0], (ndir * G4, rec["din"]))
                if gWih is not None:
                    ops.linear_wgrad(dg2, rec["inp"].v, gWih, db=st.gspan(names[2], last[2], (ndir * G4,)))
                    gWhh = st.gspan(names[1], last[1], (ndir * G4, Hh))
                    hp = rec["hprev"].view(Bd * T, ndir * Hh)
                    for d in range(ndir):
                        ops.linear_wgrad(dg2[:, d * G4:(d + 1) * G4], hp[:, d * Hh:(d + 1) * Hh], gWhh[d * G4:(d + 1) * G4])
                    ops.colsum(dg2, st.gspan(names[3], last[3], (ndir * G4,)))
                need_dx = rec["l"] > 0 or need_input_grad
                if not need_dx:
                    break
                dxin = _empty(Bd * T, rec["din"], device=dev)
                ops.linear_dgrad(dg2, rec["Wih"], dxin)
                if rec["l"] > 0:
                    prev = saved[rec["l"] - 1]
                    if prev["drop"] is not None:
                        dyp = _empty(Bd * T, ndir * Hh, device=dev)
                        ops.leaky_dropout(prev["y"].v, dxin, dyp, 1.0, drop_p=p_inter, seed=seed, stream_id=prev["drop"])
                        dy = dyp.view(Bd, T, ndir * Hh)
                    else:
                        dy = dxin.view(Bd, T, ndir * Hh)
                else:
                    acc(x, dxin)
        tape.record(bwd)
    return out


# ---------------------------------------------------------------------------------------------------------------
# Inference-only helpers used by unast_amd.inference (no tape)
# ---------------------------------------------------------------------------------------------------------------
def speech_prenet_step(cx, m, frames, pos_t):
    """SpeechPrenet on the frames [B, T, num_mels] at the device-resident position pos_t (one decoder input per sequence)."""
    a = m.args
    N = frames.shape[0]
    W1, b1 = cx.P["speech_m.prenet.layer.fc1.linear_layer.weight"], cx.P["speech_m.prenet.layer.fc1.linear_layer.bias"]
    W2, b2 = cx.P["speech_m.prenet.layer.fc2.linear_layer.weight"], cx.P["speech_m.prenet.layer.fc2.linear_layer.bias"]
    h1 = _empty(N, W1.shape[0], like=frames)
    ops.decode_linear(None, W1, b1, h1, act=1, drop_p=cx.p(a.s_pre_drop), seed=cx.seed, stream_id=cx.stream(), x_frames=frames, pos=pos_t)
    h2 = _empty(N, W2.shape[0], like=frames)
    ops.decode_linear(h1, W2, b2, h2, act=1)
    return h2


def text_postnet(cx, m, hid3d):
    """TextPostnet (src/module.py:233-246) on a [B,T,E] tensor: fc1(dropout(x)) -> [B,T,V]; no tape."""
    B, T, E = hid3d.shape
    N = B * T
    x = hid3d.reshape(N, E)
    p = cx.p(m.args.t_post_drop)
    if p > 0:
        xd = _empty(N, E, like=x)
        ops.leaky_dropout(x, None, xd, 1.0, drop_p=p, seed=cx.seed, stream_id=cx.stream())
        x = xd
    W, b = cx.P["text_m.postnet.fc1.weight"], cx.P["text_m.postnet.fc1.bias"]
    V = W.shape[0]
    ldl = (V + 3) // 4 * 4
    logits = torch.zeros(N, ldl, dtype=torch.float32, device=x.device)
    ops.linear_fwd(x, W, b, logits[:, :V])
    return logits.view(B, T, ldl)[..., :V]


def speech_postnet_residual(cx, m, mel3d, residual=True):
    """mel + SpeechPostnet(mel) for a [B,T,M] tensor (src/network.py:246; BN in the model's current mode); residual=False:
    SpeechPostnet(mel) alone (SpeechTransformer.postprocess, src/network.py:216-217).  No tape."""
    B, T, M = mel3d.shape
    N = B * T
    x = Var(mel3d.reshape(N, M))
    y = _postnet_convs(cx, None, m, x, B, T)
    Wp2, b2 = cx.P["speech_m.postnet.conv2.conv.weight"], cx.P["speech_m.postnet.conv2.conv.bias"]
    post = _empty(B, T, M, like=mel3d)
    C = y.v.shape[1]
    ops.gemm(ops.OP_KC_CONV, ops.OP_KC, y.v, C, Wp2, 5 * C, post, M, N, M, 5 * C, conv=(T, C, 0, 4), bias=b2, R=x.v if residual else None, ldr=M)
    return post
