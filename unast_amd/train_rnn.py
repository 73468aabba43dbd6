"""Training the RNN family's encoders on the HIP path: the train-mode `encode` of TextRNN / SpeechRNN (src/network.py:295-310, 514-537;
src/module.py:95-110, 217-230, 313-336) and its backward, as two explicit entry points.  `model.encode()` stays the eval forward and keeps
refusing train mode, autograd and noise_in (unast_amd.network._RNNModel._check_call).

    tape = encoder_forward(model, x, lens, noise_in=False, seed=0)      # tape.hidden = (h, c), tape.enc_output, tape.pad_mask
    d_mel = encoder_backward(tape, d_enc_output, d_h, d_c)                  # writes p.grad of model.prenet and model.encoder

Arithmetic as the reference's train mode: dropout at every nn.Dropout of the prenets (SpeechPrenet has ONE, after fc1: its second
'dropout2' key replaces the first in the OrderedDict, src/module.py:95-102), nn.LSTM's inter-layer dropout on layer 0's output, noise_fn on
the embedded text / the mel, and BatchNorm on batch statistics over all B*T positions with the running statistics updated.  Masks come
from the package's counter-based RNG; the tape lists every site (name, p, seed, stream, epoch, rows, cols, kind) so that a test can rebuild
them (tests/dropout_mirror.py).  Contractions keep fp32-level products in both directions (unast_amd.rnn._linear_rows and its gradient
forms below).  The recurrence and its backward are unast_lstm_seq_fwd_train / unast_lstm_seq_bwd (csrc/rnn.hip); dW_ih, dW_hh, dx and the
bias gradients are GEMMs and column sums over the kernel's dxproj.  Everything runs under torch.no_grad() on the current stream.  DESIGN 5i.
"""
import collections

import torch

from . import ops
from .rnn import _buf, _c, _conv, _linear_rows, _resid
from .utils import PAD_IDX

_F32 = torch.float32
NOISE_P = 0.3                     # noise_fn's mask_p (src/utils.py:40)
# stream ids of the mask sites (one seed per call, one stream per site)
S_EMB, S_NOISE, S_PRE1, S_PRE2, S_PRE3, S_EDROP = 1, 2, 3, 4, 5, 6

Site = collections.namedtuple("Site", "name p seed stream epoch rows cols kind")      # kind: 'element' (dropout, 1/(1-p) rescale) or 'row' (noise_fn)


class TrainPack:
    """The operands the train kernels read, derived from the parameters of model.prenet and model.encoder (batch-statistics BatchNorm cannot
    use rnn.Pack's folded conv weights)."""

    def __init__(self, m, side):
        enc = m.encoder
        self.layers = []
        for l in range(enc.num_layers):
            sfx = ("_l%d" % l, "_l%d_reverse" % l)
            g = lambda n: [getattr(enc.rnn, n + s) for s in sfx]                        # noqa: E731
            whh = torch.stack(g("weight_hh"))
            self.layers.append(dict(w_ih=_resid(torch.cat(g("weight_ih"))), wfrag=ops.lstm_whh_fragments(whh), wfrag_t=ops.lstm_whh_fragments_bwd(whh),
                                    b_ih=torch.cat(g("bias_ih")).detach().contiguous(), b_hh=torch.cat(g("bias_hh")).detach().contiguous(),
                                    params=[tuple(getattr(enc.rnn, n + s) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) for s in sfx]))
        self.reduce = [(_c(lin.weight), _c(lin.bias), lin.weight.detach().t().contiguous(), lin) for lin in (enc.reduce_h_W, enc.reduce_c_W)]
        if side == "text":
            pn = m.prenet
            self.emb = _c(pn.embed.weight)
            self.convs = [(_resid(getattr(pn, "conv%d" % i).conv.weight.detach().permute(0, 2, 1)), _c(getattr(pn, "conv%d" % i).conv.bias),
                           getattr(pn, "conv%d" % i).conv, getattr(pn, "batch_norm%d" % i)) for i in (1, 2, 3)]
        else:
            pn = m.prenet.layer
            self.fcs = [(_resid(fc.linear_layer.weight), _c(fc.linear_layer.bias), fc.linear_layer) for fc in (pn.fc1, pn.fc2)]


def train_pack_of(m, side):
    ver, dev = 0, None
    for t in list(m.prenet.parameters()) + list(m.encoder.parameters()):
        ver += t._version
        dev = t.device
    key = (ver, dev)
    cached = m.__dict__.get("_rnn_train_pack")
    if cached is None or cached[0] != key:
        cached = (key, TrainPack(m, side))
        m.__dict__["_rnn_train_pack"] = cached
    return cached[1]


class Tape:
    """What encoder_forward returns and encoder_backward consumes (once)."""

    def __init__(self):
        self.sites = []
        self.used = False

    def site(self, name, p, stream, rows, cols, kind="element"):
        if p > 0.0:
            self.sites.append(Site(name, float(p), self.seed, stream, self.epoch, rows, cols, kind))


def _encoder_params(model):
    return list(model.prenet.parameters()) + list(model.encoder.parameters())


def _check_model(model, what):
    from .network import TextRNN, SpeechRNN
    if not isinstance(model, (TextRNN, SpeechRNN)):
        raise TypeError("%s: model must be a unast_amd.network.TextRNN or SpeechRNN" % what)
    if not model.training:
        raise RuntimeError("%s is the train-mode entry point: call model.train() first (model.encode() is the eval forward)" % what)


# ---- fp32-level gradient contractions (the forward's three-launch form, unast_amd.rnn._linear_rows) ------------------------------------
def _parts(x2d):
    x = x2d.contiguous()
    hi, rest = torch.empty_like(x), torch.empty_like(x)
    ops.split_parts(x, hi=hi, rest=rest)
    return x, hi, rest


def _dgrad_rows(dyp, Wp, dx):
    """dx[M,K] = dy[M,N] W[N,K]; dyp = _parts(dy), Wp = _resid(W)."""
    dy, dyh, dyr = dyp
    W, Wr = Wp
    t1, t2 = torch.empty_like(dx), torch.empty_like(dx)
    ops.linear_dgrad(dyh, W, t1)
    ops.linear_dgrad(dyr, W, t2, R=t1)
    ops.linear_dgrad(dy, Wr, dx, R=t2)
    return dx


def _wgrad_rows(dyp, cols, x2d, xres, dW, dbs=()):
    """dW[N,K] += dy[:, cols]^T x, every db += column sums of dy[:, cols]; dyp = _parts(dy), xres = what the operand preparation drops of x."""
    dy, dyh, dyr = (t[:, cols] for t in dyp)
    M, N = dy.shape
    K = x2d.shape[1]
    sk = ops._splitk_for(N, K, M)
    for a, b in ((dyh, x2d), (dyr, x2d), (dy, xres)):
        ops.gemm(ops.OP_RC, ops.OP_RC, a, a.stride(0), b, b.stride(0), dW, dW.stride(0), N, K, M, beta=1, splitk=sk)
    for db in dbs:
        ops.colsum(dy, db)


def _resid_of(x2d):
    r = torch.empty_like(x2d)
    ops.split_parts(x2d, resid=r)
    return r


ALL = slice(None)


# ---- forward -------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def encoder_forward(model, x, lens, noise_in=False, seed=0):
    """Train-mode `encode`: x = token ids [B,T] int64 (TextRNN) or mel [B,T,num_mels] (SpeechRNN) on the GPU, lens as encode takes them
    (max(lens) == T).  Returns a Tape: .hidden = (h, c) [2,B,256], .enc_output [B,T,512] (zero rows at t >= lens[b]), .pad_mask bool [B,T].
    Updates the BatchNorm running statistics (text)."""
    _check_model(model, "encoder_forward")
    if not torch.is_tensor(x) or x.dim() < 2:
        raise ValueError("encoder_forward: x must be a tensor [B,T] (text) or [B,T,num_mels] (speech)")
    side = model._side
    lens_i32 = model._enc_lens(x, lens)
    if not x.is_cuda:
        raise ValueError("encoder_forward: x must be a CUDA tensor")
    if next(model.parameters()).device.type != "cuda":
        raise RuntimeError("unast_amd runs on the GPU only: move the model to a CUDA (ROCm) device first; there is no CPU path")
    P = train_pack_of(model, side)
    tape = Tape()
    tape.model, tape.side, tape.P, tape.lens, tape.noise_in = model, side, P, lens_i32, bool(noise_in)
    tape.seed, tape.epoch = int(seed), ops.rng_epoch_counter().clone()
    dev = x.device
    noise_p = NOISE_P if noise_in else 0.0
    if side == "text":
        ids = model._ids(x)
        B, T = ids.shape
        N = B * T
        p = float(model.prenet.p)
        x0 = _buf(N, P.emb.shape[1], dev=dev)
        ops.embed_fwd(ids, P.emb, x0, T, drop_p=p, seed=seed, stream_id=S_EMB, noise_p=noise_p, noise_stream=S_NOISE)
        tape.site("emb_dropout", p, S_EMB, N, x0.shape[1])
        tape.site("noise", noise_p, S_NOISE, N, 1, "row")
        tape.ids = ids
        tape.pad_mask = ids.eq(PAD_IDX)
        C = 256
        tape.xs, tape.zs = [x0], []
        tape.mean, tape.rstd = _buf(3, C, dev=dev), _buf(3, C, dev=dev)
        bn_ws = torch.empty(2 * C, dtype=torch.float64, device=dev)
        cur = x0.view(B, T, -1)
        for i, (wp, bias, _, bn) in enumerate(P.convs):
            if bn.momentum is None or not bn.track_running_stats or not bn.affine:
                raise NotImplementedError("encoder_forward: BatchNorm1d with affine parameters, running statistics and a fixed momentum (the reference's)")
            z = _conv(cur, wp, bias, 2)
            y = _buf(N, C, dev=dev)
            ops.bn_fwd(z.view(N, C), bn.weight, bn.bias, y, tape.mean[i], tape.rstd[i], bn.running_mean, bn.running_var, bn_ws, 1, drop_p=p, seed=seed,
                       stream_id=S_PRE1 + i, eps=bn.eps, momentum=bn.momentum, num_batches_tracked=bn.num_batches_tracked)
            tape.site("dropout%d" % (i + 1), p, S_PRE1 + i, N, C)
            tape.zs.append(z.view(N, C))
            tape.xs.append(y)
            cur = y.view(B, T, C)
        model.__dict__.pop("_rnn_pack", None)              # the running statistics moved under the cached eval operands (kernel writes)
        front = tape.xs[3]
    else:
        mel = model._mel(x)
        B, T, M = mel.shape
        N = B * T
        p = float(model.prenet.p)
        m2 = mel.view(N, M)
        if noise_in:
            mn = torch.empty_like(m2)
            ops.rowmask(m2, mn, noise_p, seed, S_NOISE)
            m2 = mn
        tape.site("noise", noise_p, S_NOISE, N, 1, "row")
        (w1, b1, _), (w2, b2, _) = P.fcs
        a1 = _linear_rows(m2, w1, b1)
        h1 = torch.empty_like(a1)
        ops.leaky_dropout(a1, None, h1, 0.0, p, seed, S_PRE1)
        tape.site("dropout2", p, S_PRE1, N, a1.shape[1])
        h2 = _linear_rows(h1, w2, b2, act=1)
        tape.m2, tape.a1, tape.h1, tape.h2 = m2, a1, h1, h2
        tape.pad_mask = torch.arange(T, device=dev)[None, :] >= lens_i32[:, None]
        front = h2
    # ---- RNNEncoder.forward: packed bidirectional LSTM stack, inter-layer dropout, reduce_h_W / reduce_c_W ------------------------------------
    e_drop = float(model.encoder.rnn.dropout)
    L = len(P.layers)
    h, c = _buf(L, B, 256, dev=dev), _buf(L, B, 256, dev=dev)
    tape.B, tape.T, tape.e_drop = B, T, e_drop
    tape.lstm = []
    x2 = front
    for l, lay in enumerate(P.layers):
        xproj = _linear_rows(x2, lay["w_ih"], None).view(B, T, -1)
        y, hn, cn = _buf(B, T, 512, dev=dev), _buf(B, 512, dev=dev), _buf(B, 512, dev=dev)
        saved, hprev = _buf(B, T, 2, 5, 256, dev=dev), _buf(B, T, 512, dev=dev)
        ops.lstm_seq_fwd_train(xproj, lay["wfrag"], lay["b_ih"], lay["b_hh"], lens_i32, y, hn, cn, saved, hprev)
        ops.rnn_linear(hn, P.reduce[0][0], P.reduce[0][1], h[l])
        ops.rnn_linear(cn, P.reduce[1][0], P.reduce[1][1], c[l])
        tape.lstm.append(dict(x=x2, hn=hn, cn=cn, saved=saved, hprev=hprev))
        x2 = y.view(N, 512)
        if l + 1 < L and e_drop > 0.0:
            yd = torch.empty_like(x2)
            ops.leaky_dropout(x2, None, yd, 1.0, e_drop, seed, S_EDROP + l)
            tape.site("e_drop%d" % l, e_drop, S_EDROP + l, N, 512)
            x2 = yd
    tape.hidden, tape.enc_output = (h, c), y
    return tape


# ---- backward ------------------------------------------------------------------------------------------------------------------------------
def _prepare_grads(params, accumulate):
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


def _cot(t, shape, name, dev):
    if t is None:
        return None
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype is _F32 and tuple(t.shape) == tuple(shape)):
        raise ValueError("encoder_backward: %s must be a float32 CUDA tensor %s" % (name, tuple(shape)))
    return t.detach().contiguous()


@torch.no_grad()
def encoder_backward(tape, d_enc_output=None, d_h=None, d_c=None, accumulate=False):
    """Backward of encoder_forward for the scalar whose gradients with respect to enc_output [B,T,512], h and c [2,B,256] are given (None =
    zero).  Writes p.grad of exactly the parameters under model.prenet and model.encoder, in the reference's shapes: overwritten
    (accumulate=False; an existing dense fp32 .grad is kept in place) or added to (accumulate=True).  Returns d_mel [B,T,num_mels] (speech)
    or None (text).  A tape is used once."""
    if not isinstance(tape, Tape):
        raise TypeError("encoder_backward: tape must come from encoder_forward")
    if tape.used:
        raise RuntimeError("encoder_backward: this tape has been used; run encoder_forward again")
    model, P, B, T, seed = tape.model, tape.P, tape.B, tape.T, tape.seed
    N = B * T
    dev = tape.enc_output.device
    L = len(P.layers)
    d_enc_output = _cot(d_enc_output, (B, T, 512), "d_enc_output", dev)
    d_h, d_c = _cot(d_h, (L, B, 256), "d_h", dev), _cot(d_c, (L, B, 256), "d_c", dev)
    tape.used = True
    _prepare_grads(_encoder_params(model), accumulate)

    dy = d_enc_output.view(N, 512) if d_enc_output is not None else torch.zeros(N, 512, dtype=_F32, device=dev)
    for l in range(L - 1, -1, -1):
        lay, st = P.layers[l], tape.lstm[l]
        dfin = []
        for d_state, (W, _, Wt, lin), fin in ((d_h, P.reduce[0], st["hn"]), (d_c, P.reduce[1], st["cn"])):
            if d_state is None:
                dfin.append(None)
                continue
            g = d_state[l]                                                                 # [B,256]: the gradient of reduce_*_W's output
            dfin.append(ops.rnn_linear(g, Wt, None, _buf(B, 512, dev=dev)))                # g W [256,512]
            _wgrad_rows(_parts(g), ALL, fin, _resid_of(fin), lin.weight.grad, (lin.bias.grad,))
        if l + 1 < L and tape.e_drop > 0.0:
            dyd = torch.empty_like(dy)
            ops.leaky_dropout(dy, dy, dyd, 1.0, tape.e_drop, seed, S_EDROP + l)            # slope 1: the mask and its 1/(1-p) only
            dy = dyd
        dxproj = _buf(B, T, 2048, dev=dev)
        ops.lstm_seq_bwd(dy.view(B, T, 512), lay["wfrag_t"], st["saved"], tape.lens, dxproj, dhfinal=dfin[0], dcfinal=dfin[1])
        dxp = _parts(dxproj.view(N, 2048))
        xin, hprev = st["x"], st["hprev"].view(N, 512)
        xin_res, hprev_res = _resid_of(xin), _resid_of(hprev)
        for d, (w_ih, w_hh, b_ih, b_hh) in enumerate(lay["params"]):
            cols = slice(1024 * d, 1024 * (d + 1))
            _wgrad_rows(dxp, cols, xin, xin_res, w_ih.grad, (b_ih.grad, b_hh.grad))
            _wgrad_rows(dxp, cols, hprev[:, 256 * d:256 * (d + 1)], hprev_res[:, 256 * d:256 * (d + 1)], w_hh.grad)
        dy = _dgrad_rows(dxp, lay["w_ih"], _buf(N, xin.shape[1], dev=dev))

    if tape.side == "text":
        C = 256
        p = float(model.prenet.p)
        bn_ws = torch.empty(2 * C, dtype=torch.float64, device=dev)
        for i in (2, 1, 0):
            (wp, wr), _, conv, bn = P.convs[i]
            dz = _buf(N, C, dev=dev)
            ops.bn_bwd(dy, tape.zs[i], tape.mean[i], tape.rstd[i], bn.weight, bn.bias, dz, bn.weight.grad, bn.bias.grad, bn_ws, 1, drop_p=p, seed=seed,
                       stream_id=S_PRE1 + i)
            xin = tape.xs[i]
            Cin = xin.shape[1]
            dz, dzh, dzr = (t.view(B, T, C) for t in _parts(dz))
            gw = torch.zeros_like(wp)
            x3, x3res = xin.view(B, T, Cin), _resid_of(xin).view(B, T, Cin)
            ops.conv_taps_wgrad(dzh, x3, gw, 2)
            ops.conv_taps_wgrad(dzr, x3, gw, 2)
            ops.conv_taps_wgrad(dz, x3res, gw, 2)
            conv.weight.grad.add_(gw.permute(0, 2, 1))
            ops.colsum(dz.view(N, C), conv.bias.grad)
            dx = _buf(B, T, Cin, dev=dev)
            ops.conv_taps_dgrad(dzh, wp, dx, 2)
            ops.conv_taps_dgrad(dzr, wp, dx, 2, beta=1)
            ops.conv_taps_dgrad(dz, wr, dx, 2, beta=1)
            dy = dx.view(N, Cin)
        noise_p = NOISE_P if tape.noise_in else 0.0
        ops.embed_bwd(tape.ids, dy, model.prenet.embed.weight.grad, T, drop_p=p, seed=seed, stream_id=S_EMB, noise_p=noise_p, noise_stream=S_NOISE,
                      padding_idx=model.prenet.embed.padding_idx)
        return None

    p = float(model.prenet.p)
    (w1, _, fc1), (w2, _, fc2) = P.fcs
    ops.relu_bwd(dy, tape.h2)
    dyp = _parts(dy)
    _wgrad_rows(dyp, ALL, tape.h1, _resid_of(tape.h1), fc2.weight.grad, (fc2.bias.grad,))
    dh1 = _dgrad_rows(dyp, w2, _buf(N, tape.h1.shape[1], dev=dev))
    da1 = torch.empty_like(dh1)
    ops.leaky_dropout(tape.a1, dh1, da1, 0.0, p, seed, S_PRE1)
    dap = _parts(da1)
    _wgrad_rows(dap, ALL, tape.m2, _resid_of(tape.m2), fc1.weight.grad, (fc1.bias.grad,))
    M = tape.m2.shape[1]
    d_mel = _dgrad_rows(dap, w1, _buf(N, M, dev=dev))
    if tape.noise_in:
        out = torch.empty_like(d_mel)
        ops.rowmask(d_mel, out, NOISE_P, seed, S_NOISE)
        d_mel = out
    return d_mel.view(B, T, M)
