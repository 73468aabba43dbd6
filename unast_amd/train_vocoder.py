"""Training the CBHG vocoder on the HIP path: the loop body of src/train_vocoder.py (85-100: train-mode forward, L1 / L2 sum loss,
backward, clip, Adam(W), schedule) without its dataset, TensorBoard and file handling.

`vocoder_step` is the explicit entry point of the train-mode forward and backward; `Vocoder.forward` stays the eval forward.  BatchNorm
runs on batch statistics over all B*T rows (padded rows included: the reference does not mask) and updates its running statistics as
nn.BatchNorm1d does.  The backward's discrete decisions -- ReLU gates, the max pool's choice, the L1 sign -- are read from what the
forward stored, never recomputed.  Every forward contraction is one of unast_amd.contract's three-launch forms (linear_rows, conv) over
weight pairs derived per call, just ahead of each stage; the backward keeps one launch per gradient contraction (_wgrad, ops.linear_dgrad,
ops.conv_taps_wgrad / _dgrad).  Everything is enqueued on the current stream; the loss stays on the device.  DESIGN 5g, 5t.
"""
import torch

from . import contract, flat_adam, ops
from .contract import buf
from .vocoder import Vocoder, gru_operands, highway_operands

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
        contract.check_bn(bn, "vocoder_step")

    def bn_fwd(i, z2d, y2d, act):
        bn = bns[i]
        ops.bn_fwd(z2d, bn.weight, bn.bias, y2d, mean[i], rstd[i], bn.running_mean, bn.running_var, bn_ws, act, eps=bn.eps, momentum=bn.momentum,
                   num_batches_tracked=bn.num_batches_tracked)

    def bn_bwd(i, dy2d, z2d, dz2d):
        bn = bns[i]
        ops.bn_bwd(dy2d, z2d, mean[i], rstd[i], bn.weight, bn.bias, dz2d, bn.weight.grad, bn.bias.grad, bn_ws, 0)      # (act 0: dy arrives gated)

    def work(x, z):
        """The step's scratch as the four temporaries of one forward contraction with input x and output z."""
        return tuple(t[:like.numel()].view(like.shape) for t, like in zip(scratch, (x, x, z, z)))

    contract.prepare_grads(model.parameters(), False)
    model.__dict__.pop("_vocoder_pack", None)             # the running statistics move under the cached eval operands (kernel writes)
    mean, rstd = buf(K + 2, C, dev=dev), buf(K + 2, C, dev=dev)
    bn_ws = torch.empty(2 * C, dtype=torch.float64, device=dev)
    # ---- forward: each contraction's weight pair (contract.resid / tap_major, the extractors of unast_amd.vocoder) is derived per call -- FlatAdamW
    # moves the parameters behind the version counters, a cache would go stale every step -- and just ahead of its stage: these small launches
    # then queue behind the stage before, where at the top of the step the GPU would wait for the host through all of them -----------------------
    x2 = mel.contiguous().view(N, M)
    mag2 = mag.contiguous().view(N, F_)
    pre, post = model.pre_projection.conv, model.post_projection.conv
    x0 = buf(N, C, dev=dev)
    scratch = [buf(N * K * C, dev=dev), buf(N * K * C, dev=dev), buf(N * max(ld, 3 * C), dev=dev), buf(N * max(ld, 3 * C), dev=dev)]  # operand parts and partial sums (work)
    contract.linear_rows(x2, contract.resid(pre.weight[:, :, 0]), pre.bias, out=x0, work=work(x2, x0))
    zs, ys = buf(K, N, C, dev=dev), buf(K, N, C, dev=dev)  # bank: conv outputs (BatchNorm inputs) and post-ReLU stage outputs
    pooled = buf(B, T, K * C, dev=dev)
    bank_w = []                                             # the weights alone: what the backward's single launches read
    src = x0.view(B, T, C)
    for k in range(1, K + 1):                               # a CHAIN: stage k reads stage k-1 (src/module.py:605-607)
        wp, bias = contract.tap_major(c.convbank_list[k - 1])
        bank_w.append(wp[0])
        z = zs[k - 1].view(B, T, C)
        contract.conv(src, wp, bias, k // 2, out=z, work=work(src, z))
        bn_fwd(k - 1, zs[k - 1], ys[k - 1], 1)
        src = ys[k - 1].view(B, T, C)
        ops.maxpool_prev(src, pooled[:, :, (k - 1) * C:k * C])
    (w1p, b1), (w2p, b2) = contract.tap_major(c.conv_projection_1), contract.tap_major(c.conv_projection_2)
    w1, w2 = w1p[0], w2p[0]
    z1, p1, z2 = buf(N, C, dev=dev), buf(N, C, dev=dev), buf(N, C, dev=dev)
    contract.conv(pooled, w1p, b1, 1, out=z1.view(B, T, C), work=work(pooled, z1.view(B, T, C)))
    bn_fwd(K, z1, p1, 1)
    contract.conv(p1.view(B, T, C), w2p, b2, 1, out=z2.view(B, T, C), work=work(p1.view(B, T, C), z2.view(B, T, C)))
    hx = buf(5, N, C, dev=dev)                              # highway inputs; hx[4] is its output
    bn_fwd(K + 1, z2, hx[0], 0)
    ops.add_inplace(hx[0], x0)                              # residual (src/module.py:619)
    hts = buf(4, N, 2 * C, dev=dev)
    hw_w = []
    for i, (w, b) in enumerate(highway_operands(c.highway)):
        hw_w.append(w)
        contract.linear_rows(hx[i], contract.resid(w), b, out=hts[i], work=work(hx[i], hts[i]))
        ops.highway_combine(hts[i], hx[i], hx[i + 1])
    gy = buf(2, B, T, C, dev=dev)                           # GRU layer outputs
    saved = buf(2, B, T, 2, 2 * C, dev=dev)
    xproj = buf(B, T, 3 * C, dev=dev)
    gin = hx[4]
    gru_w = []
    for layer in range(2):
        w_ih, b_x, w_hh, b_hn = gru_operands(c.gru, layer)
        gru_w.append((w_ih, w_hh))
        contract.linear_rows(gin, contract.resid(w_ih), b_x, out=xproj.view(N, 3 * C), work=work(gin, xproj.view(N, 3 * C)))
        ops.gru_fwd_train(xproj, w_hh, b_hn, gy[layer], saved[layer])
        gin = gy[layer].view(N, C)
    out = buf(N, ld, dev=dev)
    post_w = contract.resid(post.weight[:, :, 0])
    contract.linear_rows(gin, post_w, post.bias, out=out, work=work(gin, out))
    del scratch[:]                                          # (the partial sums are as wide as the prediction: not kept through the backward)
    # ---- loss (src/train_vocoder.py:91) ----------------------------------------------------------------------------------------------
    loss = torch.zeros((), dtype=torch.float64, device=dev)
    dout = buf(N, ld, dev=dev)
    ops.sum_loss(out[:, :F_], mag2, dout[:, :F_], l2, loss)
    if taps is not None:
        taps.update(bank=ys.view(K, B, T, C).permute(1, 2, 0, 3).reshape(B, T, K * C), proj1=p1.view(B, T, C).clone(),
                    highway_pre=[hts[i].clone() for i in range(4)], mag_pred=out.view(B, T, ld)[:, :, :F_])
    # ---- backward (loss.backward(), src/train_vocoder.py:94) -------------------------------------------------------------------------
    _wgrad(dout[:, :F_], gin, post.weight.grad.view(F_, C), post.bias.grad)
    dg = buf(N, C, dev=dev)
    ops.linear_dgrad(dout[:, :F_], post_w[0], dg)
    dxg, dhn, hs = buf(B, T, 2, 3 * C // 2, dev=dev), buf(B, T, 2, C // 2, dev=dev), buf(B, T, C, dev=dev)
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
    dpre = buf(N, 2 * C, dev=dev)
    for i in (3, 2, 1, 0):
        ops.highway_combine_bwd(dg, hts[i], hx[i], dpre, dg)
        l, g = c.highway.linears[i].linear_layer, c.highway.gates[i].linear_layer
        _wgrad(dpre[:, :C], hx[i], l.weight.grad, l.bias.grad)
        _wgrad(dpre[:, C:], hx[i], g.weight.grad, g.bias.grad)
        ops.linear_dgrad(dpre, hw_w[i], dg, beta=1)
    # dg = gradient of (BN2(conv2(p1)) + x0): it flows into the projection chain and, as the residual, into x0
    dz, dz_next, dy = buf(N, C, dev=dev), buf(N, C, dev=dev), buf(N, C, dev=dev)
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
    dpooled = buf(B, T, K * C, dev=dev)
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
