"""Training the CBHG vocoder on the HIP path: the loop body of src/train_vocoder.py (85-100: train-mode forward, L1 / L2 sum loss,
backward, clip, Adam(W), schedule) without its dataset, TensorBoard and file handling.

`vocoder_step` is the explicit entry point of the train-mode forward and backward; `Vocoder.forward` stays the eval forward.  BatchNorm
runs on batch statistics over all B*T rows (padded rows included: the reference does not mask) and updates its running statistics as
nn.BatchNorm1d does.  The backward's discrete decisions -- ReLU gates, the max pool's choice, the L1 sign -- are read from what the
forward stored, never recomputed.  Everything is enqueued on the current stream; the loss stays on the device.  DESIGN 5g.
"""
import torch

from . import flat_adam, ops
from .vocoder import Vocoder

_F32 = torch.float32


def _check_batch(model, mel, mag, what):
    if not isinstance(model, Vocoder):
        raise TypeError("%s: model must be a unast_amd.vocoder.Vocoder" % what)
    ok = (torch.is_tensor(mel) and torch.is_tensor(mag) and mel.dim() == 3 and mag.dim() == 3 and mel.shape[2] == model.num_mels
          and mag.shape[2] == model.num_bins and mel.shape[:2] == mag.shape[:2] and mel.shape[0] > 0 and mel.shape[1] > 0
          and mel.dtype is _F32 and mag.dtype is _F32 and mel.is_cuda and mag.is_cuda and mel.device == mag.device)
    if not ok:
        raise ValueError("%s: mel [B, T, %d] and mag [B, T, %d] must be float32 CUDA tensors of one batch" % (what, model.num_mels, model.num_bins))


def _loss_flag(loss_type):
    if loss_type not in ("l1", "l2"):
        raise ValueError("loss_type must be 'l1' or 'l2' (src/train_vocoder.py:58-61), got %r" % (loss_type,))
    return loss_type == "l2"


def _grads(model):
    """Dense zeroed .grad of every parameter, in the reference's shapes (kept when they already are: FlatAdamW's views stay in place)."""
    gs = []
    for p in model.parameters():
        g = p.grad
        if g is None or not g.is_contiguous() or g.dtype is not _F32 or g.device != p.device or g.data_ptr() % 16:
            g = p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
        gs.append(g)
    torch._foreach_zero_(gs)


def _gru_operands(gru, layer):
    """One layer's operands as vocoder._Pack lays them out: weight_ih of both directions [768,256], its bias with b_hr, b_hz added,
    weight_hh [2,384,128], b_hn [2,128]."""
    H = gru.hidden_size
    w_ih, b_x, w_hh, b_hn = [], [], [], []
    for sfx in ("_l%d" % layer, "_l%d_reverse" % layer):
        b_ih, b_hh = getattr(gru, "bias_ih" + sfx), getattr(gru, "bias_hh" + sfx)
        w_ih.append(getattr(gru, "weight_ih" + sfx))
        w_hh.append(getattr(gru, "weight_hh" + sfx))
        bx = b_ih.clone()
        bx[:2 * H] += b_hh[:2 * H]
        b_x.append(bx)
        b_hn.append(b_hh[2 * H:])
    return torch.cat(w_ih).contiguous(), torch.cat(b_x).contiguous(), torch.stack(w_hh).contiguous(), torch.stack(b_hn).contiguous()


def _wgrad(dy2d, x2d, dW, db):
    """dW[N,K] += dy2d[M,N]^T x2d[M,K], db[N] += column sums of dy2d, on the current stream (dy2d / x2d may be column slices)."""
    M, N = dy2d.shape
    K = x2d.shape[1]
    ops.gemm(ops.OP_RC, ops.OP_RC, dy2d, dy2d.stride(0), x2d, x2d.stride(0), dW, dW.stride(0), N, K, M, beta=1,
             splitk=ops._splitk_for(N, K, M), rowsum_a=db)


@torch.no_grad()
def vocoder_step(model, mel, mag, loss_type="l1", taps=None):
    """Train-mode forward, sum loss and backward of the vocoder (src/train_vocoder.py:90-94).  mel [B,T,num_mels], mag [B,T,num_bins], fp32
    on the GPU.  Returns (loss, mag_pred): loss a float64 device scalar (no host synchronisation here), mag_pred a [B,T,num_bins] view.
    Overwrites p.grad of every parameter in the reference's shapes and updates the BatchNorm running statistics.
    taps: a dict that receives bank [B,T,256 K] (post-ReLU concat), proj1 [B,T,256] (post-ReLU), highway_pre (four [N,512] blocks
    [linear | gate] before their activations) and mag_pred -- the stored values the backward takes its gates from."""
    if not isinstance(model, Vocoder):
        raise TypeError("vocoder_step: model must be a unast_amd.vocoder.Vocoder")
    if not model.training:
        raise RuntimeError("vocoder_step is the train-mode step: call model.train() first (Vocoder.forward is the eval forward)")
    _check_batch(model, mel, mag, "vocoder_step")
    l2 = _loss_flag(loss_type)
    c = model.cbhg
    B, T, M = mel.shape
    N, C, K, F_ = B * T, model.hidden_size, c.K, model.num_bins
    ld = (F_ + 3) // 4 * 4
    dev = mel.device
    bns = list(c.batchnorm_list) + [c.batchnorm_proj_1, c.batchnorm_proj_2]
    for bn in bns:
        if bn.momentum is None or not bn.track_running_stats or not bn.affine:
            raise NotImplementedError("vocoder_step: BatchNorm1d with affine parameters, running statistics and a fixed momentum (the reference's)")

    def buf(*shape):
        return torch.empty(*shape, dtype=_F32, device=dev)

    def bn_fwd(i, z2d, y2d, act):
        bn = bns[i]
        ops.bn_fwd(z2d, bn.weight, bn.bias, y2d, mean[i], rstd[i], bn.running_mean, bn.running_var, bn_ws, act, eps=bn.eps, momentum=bn.momentum,
                   num_batches_tracked=bn.num_batches_tracked)

    def bn_bwd(i, dy2d, z2d, dz2d):
        bn = bns[i]
        ops.bn_bwd(dy2d, z2d, mean[i], rstd[i], bn.weight, bn.bias, dz2d, bn.weight.grad, bn.bias.grad, bn_ws, 0)      # (act 0: dy arrives gated)

    def conv_fwd(x3d, wp, wr, bias, z3d, pad_left):
        """z = conv(x, W) + bias with fp32-level products: the three-term split-bf16 form drops x_lo W_lo and what lies below 2^-17 of
        either operand, and 16 chained stages of that put the deepest stages' gradients at 20 x an fp32 step's error.  With
        x = hi + rest (hi in bf16 exactly) and W = W_hi + W_lo + wr, conv(hi, W) + conv(rest, W) + conv(x, wr) holds every product but
        the ones of order 2^-26."""
        ops.split_parts(x3d if x3d.is_contiguous() else x3d.contiguous(), hi=xh[:x3d.numel()], rest=xr[:x3d.numel()])
        h3, r3 = xh[:x3d.numel()].view(x3d.shape), xr[:x3d.numel()].view(x3d.shape)
        ops.conv_taps_fwd(h3, wp, bias, za.view(z3d.shape), pad_left)
        ops.conv_taps_fwd(r3, wp, None, zb.view(z3d.shape), pad_left, R=za)
        ops.conv_taps_fwd(x3d, wr, None, z3d, pad_left, R=zb)

    def lin_fwd(x2d, w, bias, out, n_out):
        """out[:, :n_out] = x2d w^T + bias with the same three launches (the linear layers feed the same chains)."""
        k, ldc = x2d.shape[1], out.stride(0)
        wr = torch.empty_like(w)
        ops.split_parts(w, resid=wr)
        ops.split_parts(x2d, hi=xh[:x2d.numel()], rest=xr[:x2d.numel()])
        t1, t2 = torch.empty_like(out), torch.empty_like(out)
        ops.gemm(ops.OP_KC, ops.OP_KC, xh[:x2d.numel()].view(N, k), k, w, k, t1, ldc, N, n_out, k, bias=bias)
        ops.gemm(ops.OP_KC, ops.OP_KC, xr[:x2d.numel()].view(N, k), k, w, k, t2, ldc, N, n_out, k, R=t1, ldr=ldc)
        ops.gemm(ops.OP_KC, ops.OP_KC, x2d, k, wr, k, out, ldc, N, n_out, k, R=t2, ldr=ldc)

    def tap_major(conv):
        wp = conv.weight.permute(0, 2, 1).contiguous()      # tap-major [Cout,k,Cin]
        wr = torch.empty_like(wp)
        ops.split_parts(wp, resid=wr)
        return wp, wr

    _grads(model)
    model.__dict__.pop("_vocoder_pack", None)             # the running statistics move under the cached eval operands (kernel writes)
    mean, rstd = buf(K + 2, C), buf(K + 2, C)
    bn_ws = torch.empty(2 * C, dtype=torch.float64, device=dev)
    # ---- forward ---------------------------------------------------------------------------------------------------------------------
    x2 = mel.contiguous().view(N, M)
    mag2 = mag.contiguous().view(N, F_)
    pre = model.pre_projection.conv
    pre_w = pre.weight[:, :, 0].contiguous()
    x0 = buf(N, C)
    xh, xr, za, zb = buf(N * K * C), buf(N * K * C), buf(N, C), buf(N, C)       # operand parts and partial sums of conv_fwd / lin_fwd
    lin_fwd(x2, pre_w, pre.bias, x0, C)
    zs, ys = buf(K, N, C), buf(K, N, C)                    # bank: conv outputs (BatchNorm inputs) and post-ReLU stage outputs
    pooled = buf(B, T, K * C)
    bank_w = []
    src = x0.view(B, T, C)
    for k in range(1, K + 1):                               # a CHAIN: stage k reads stage k-1 (src/module.py:605-607)
        conv = c.convbank_list[k - 1]
        wp, wr = tap_major(conv)
        bank_w.append(wp)
        conv_fwd(src, wp, wr, conv.bias, zs[k - 1].view(B, T, C), k // 2)
        bn_fwd(k - 1, zs[k - 1], ys[k - 1], 1)
        src = ys[k - 1].view(B, T, C)
        ops.maxpool_prev(src, pooled[:, :, (k - 1) * C:k * C])
    (w1, w1r), (w2, w2r) = tap_major(c.conv_projection_1), tap_major(c.conv_projection_2)
    z1, p1, z2 = buf(N, C), buf(N, C), buf(N, C)
    conv_fwd(pooled, w1, w1r, c.conv_projection_1.bias, z1.view(B, T, C), 1)
    bn_fwd(K, z1, p1, 1)
    conv_fwd(p1.view(B, T, C), w2, w2r, c.conv_projection_2.bias, z2.view(B, T, C), 1)
    hx = buf(5, N, C)                                       # highway inputs; hx[4] is its output
    bn_fwd(K + 1, z2, hx[0], 0)
    ops.add_inplace(hx[0], x0)                              # residual (src/module.py:619)
    hts = buf(4, N, 2 * C)
    hw_w = []
    for i, (l, g) in enumerate(zip(c.highway.linears, c.highway.gates)):
        w = torch.cat([l.linear_layer.weight, g.linear_layer.weight]).contiguous()
        b = torch.cat([l.linear_layer.bias, g.linear_layer.bias]).contiguous()
        hw_w.append(w)
        lin_fwd(hx[i], w, b, hts[i], 2 * C)
        ops.highway_combine(hts[i], hx[i], hx[i + 1])
    gy = buf(2, B, T, C)                                    # GRU layer outputs
    saved = buf(2, B, T, 2, 2 * C)
    gru_w = []
    xproj = buf(B, T, 3 * C)
    gin = hx[4]
    for layer in range(2):
        w_ih, b_x, w_hh, b_hn = _gru_operands(c.gru, layer)
        gru_w.append((w_ih, w_hh))
        lin_fwd(gin, w_ih, b_x, xproj.view(N, 3 * C), 3 * C)
        ops.gru_fwd_train(xproj, w_hh, b_hn, gy[layer], saved[layer])
        gin = gy[layer].view(N, C)
    post = model.post_projection.conv
    post_w = post.weight[:, :, 0].contiguous()
    out = buf(N, ld)
    lin_fwd(gin, post_w, post.bias, out, F_)
    # ---- loss (src/train_vocoder.py:91) ----------------------------------------------------------------------------------------------
    loss = torch.zeros((), dtype=torch.float64, device=dev)
    dout = buf(N, ld)
    ops.sum_loss(out[:, :F_], mag2, dout[:, :F_], l2, loss)
    if taps is not None:
        taps.update(bank=ys.view(K, B, T, C).permute(1, 2, 0, 3).reshape(B, T, K * C), proj1=p1.view(B, T, C).clone(),
                    highway_pre=[hts[i].clone() for i in range(4)], mag_pred=out.view(B, T, ld)[:, :, :F_])
    # ---- backward (loss.backward(), src/train_vocoder.py:94) -------------------------------------------------------------------------
    _wgrad(dout[:, :F_], gin, post.weight.grad.view(F_, C), post.bias.grad)
    dg = buf(N, C)
    ops.linear_dgrad(dout[:, :F_], post_w, dg)
    dxg, dhn, hs = buf(B, T, 2, 3 * C // 2), buf(B, T, 2, C // 2), buf(B, T, C)
    H = C // 2
    for layer in (1, 0):
        w_ih, w_hh = gru_w[layer]
        y = gy[layer]
        ops.gru_bwd(dg.view(B, T, C), y, saved[layer], w_hh, dxg, dhn)
        hs.zero_()                                          # h of the previous step in each direction's own order (layout copies)
        if T > 1:
            hs[:, 1:, :H].copy_(y[:, :-1, :H])
            hs[:, :-1, H:].copy_(y[:, 1:, H:])
        xin = (gy[0] if layer == 1 else hx[4]).view(N, C)
        dx2, dh2, hs2 = dxg.view(N, 6 * H), dhn.view(N, 2 * H), hs.view(N, C)
        for d, sfx in enumerate(("_l%d" % layer, "_l%d_reverse" % layer)):
            g_wih, g_whh = getattr(c.gru, "weight_ih" + sfx).grad, getattr(c.gru, "weight_hh" + sfx).grad
            g_bih, g_bhh = getattr(c.gru, "bias_ih" + sfx).grad, getattr(c.gru, "bias_hh" + sfx).grad
            _wgrad(dx2[:, 3 * H * d:3 * H * (d + 1)], xin, g_wih, g_bih)
            _wgrad(dx2[:, 3 * H * d:3 * H * d + 2 * H], hs2[:, H * d:H * (d + 1)], g_whh[:2 * H], None)
            _wgrad(dh2[:, H * d:H * (d + 1)], hs2[:, H * d:H * (d + 1)], g_whh[2 * H:], g_bhh[2 * H:])
            g_bhh[:2 * H].copy_(g_bih[:2 * H])              # b_hr, b_hz only ever appear summed with b_ir, b_iz
        ops.linear_dgrad(dx2, w_ih, dg)
    dpre = buf(N, 2 * C)
    for i in (3, 2, 1, 0):
        ops.highway_combine_bwd(dg, hts[i], hx[i], dpre, dg)
        l, g = c.highway.linears[i].linear_layer, c.highway.gates[i].linear_layer
        _wgrad(dpre[:, :C], hx[i], l.weight.grad, l.bias.grad)
        _wgrad(dpre[:, C:], hx[i], g.weight.grad, g.bias.grad)
        ops.linear_dgrad(dpre, hw_w[i], dg, beta=1)
    # dg = gradient of (BN2(conv2(p1)) + x0): it flows into the projection chain and, as the residual, into x0
    dz, dz_next, dy = buf(N, C), buf(N, C), buf(N, C)
    bn_bwd(K + 1, dg, z2, dz)
    gw2 = torch.zeros_like(w2)
    ops.conv_taps_wgrad(dz.view(B, T, C), p1.view(B, T, C), gw2, 1, db=c.conv_projection_2.bias.grad)
    c.conv_projection_2.weight.grad.copy_(gw2.permute(0, 2, 1))
    ops.conv_taps_dgrad(dz.view(B, T, C), w2, dy.view(B, T, C), 1)
    ops.relu_bwd(dy, p1)
    bn_bwd(K, dy, z1, dz)
    gw1 = torch.zeros_like(w1)
    ops.conv_taps_wgrad(dz.view(B, T, C), pooled, gw1, 1, db=c.conv_projection_1.bias.grad)
    c.conv_projection_1.weight.grad.copy_(gw1.permute(0, 2, 1))
    dpooled = buf(B, T, K * C)
    ops.conv_taps_dgrad(dz.view(B, T, C), w1, dpooled, 1)
    for k in range(K, 0, -1):
        yk = ys[k - 1].view(B, T, C)
        if k < K:                                           # stage k also feeds conv k+1: its input gradient first, the pool's share on top
            ops.conv_taps_dgrad(dz_next.view(B, T, C), bank_w[k], dy.view(B, T, C), (k + 1) // 2)
        ops.maxpool_prev_bwd(dpooled[:, :, (k - 1) * C:k * C], yk, dy.view(B, T, C), accumulate=k < K, relu_gate=True)
        bn_bwd(k - 1, dy, zs[k - 1], dz)
        conv = c.convbank_list[k - 1]
        gw = torch.zeros_like(bank_w[k - 1])
        xin = ys[k - 2].view(B, T, C) if k > 1 else x0.view(B, T, C)
        ops.conv_taps_wgrad(dz.view(B, T, C), xin, gw, k // 2, db=conv.bias.grad)
        conv.weight.grad.copy_(gw.permute(0, 2, 1))
        dz, dz_next = dz_next, dz
    ops.conv_taps_dgrad(dz_next.view(B, T, C), bank_w[0], dg.view(B, T, C), 0, beta=1)      # + the residual's share already in dg
    _wgrad(dg, x2, pre.weight.grad.view(C, M), pre.bias.grad)
    return loss, out.view(B, T, ld)[:, :, :F_]


def valid_loss(model, mel, mag, loss_type="l1"):
    """src/train_vocoder.py:135-136: the eval forward (Vocoder.forward) and the same sum loss; a float64 device scalar."""
    _check_batch(model, mel, mag, "valid_loss")
    l2 = _loss_flag(loss_type)
    with torch.no_grad():
        pred = model.forward(mel)
        loss = torch.zeros((), dtype=torch.float64, device=mel.device)
        B, T, F_ = pred.shape
        ops.sum_loss(pred.as_strided((B * T, F_), (pred.stride(1), 1)), mag.contiguous().view(B * T, F_), None, l2, loss)
    return loss


class FlatAdamW(flat_adam.FlatAdam):
    """flat_adam.FlatAdam over the vocoder's parameters (src/train_vocoder.py:31-35): parameters and gradients are re-pointed to views of two
    flat fp32 buffers, one segment that is always stepped, so step(max_norm) is one ops.sumsq launch and one ops.adamw launch."""

    def __init__(self, model, lr, weight_decay=0.0, decoupled=True, betas=(0.9, 0.999), eps=1e-8):
        params = list(model.parameters())
        if not params or any(p.dtype is not _F32 or not p.is_cuda for p in params):
            raise ValueError("FlatAdamW: float32 CUDA parameters")
        self.model = model
        super().__init__(params, [flat_adam.adopt("vocoder", params)], lr, weight_decay, betas, eps, decoupled)
        self._touch()

    def _touch(self):
        """The kernels write the flat buffer behind torch's back: drop the model's derived eval operands (Vocoder._pack is keyed on
        version counters, which such writes do not move)."""
        self.model.__dict__.pop("_vocoder_pack", None)

    @torch.no_grad()
    def step(self, max_norm=0.0, closure=None):
        self._launch(self.segments, max_norm)
        self._touch()

    def zero_grad(self, set_to_none=False):
        self.segments[0].grad.zero_()


def initialize(args):
    """src/train_vocoder.py:20-63 without the dataset and the checkpoint lookup: (model, optimizer, scheduler, loss_type).  The linear
    schedule needs args.train_steps (the reference derives it from its dataset's size)."""
    from .train import get_linear_schedule_with_warmup, get_transformer_paper_schedule
    from .utils import set_seed
    set_seed(args.seed)
    model = Vocoder(args.num_mels, args.hidden_size, args.n_fft).to("cuda")
    if args.optim_type not in ("adam", "adamw"):
        raise ValueError("optim_type must be 'adam' or 'adamw' (src/train_vocoder.py:32-35)")
    optimizer = FlatAdamW(model, lr=args.lr, weight_decay=args.weight_decay, decoupled=args.optim_type == "adamw")
    last_step = int(getattr(args, "last_step", 0))
    if args.sched_type == "linear":
        scheduler = get_linear_schedule_with_warmup(optimizer, args.warmup_steps, args.train_steps, last_epoch=last_step - 1)
    elif args.sched_type == "transformer":
        scheduler = get_transformer_paper_schedule(optimizer, args.warmup_steps, last_epoch=last_step - 1)
    else:
        raise ValueError("sched_type must be 'linear' or 'transformer' (src/train_vocoder.py:50-54)")
    _loss_flag(args.loss_type)
    return model, optimizer, scheduler, args.loss_type


def train_step(model, optimizer, scheduler, mel, mag, args):
    """src/train_vocoder.py:90-100: step, clip by args.grad_clip, update, scheduler.step(); returns the loss as a float (the one host read)."""
    loss, _ = vocoder_step(model, mel, mag, getattr(args, "loss_type", "l1"))
    optimizer.step(max_norm=args.grad_clip if args.grad_clip > 0.0 else 0.0)
    if scheduler is not None:
        scheduler.step()
    return float(loss.item())
