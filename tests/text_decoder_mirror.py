"""fp64 torch restatement of TextRNN's teacher-forced train-mode decoder (decode_sequence at teacher_ratio = 1, src/network.py:539-575;
TextPrenet, src/module.py:174-230; RNNDecoder.forward and both attention layers, src/module.py:362-497; TextPostnet, src/module.py:233-246)
with autograd, written from the description in DESIGN 5k:

  position 0 runs the prenet over [SOS] (length 1), position i >= 1 over target[:, 0:i] (length i, no SOS); every call is train-mode:
  BatchNorm on the batch statistics of the B * L_i rows of that prefix alone (PAD rows included), the running statistics updated once per
  position in order (T updates per BatchNorm, unbiased variance, num_batches_tracked += T); only the last row of each call feeds the decoder.

Dropout is an explicit factor tensor per site (0 or 1/(1-p)), so that a test can impose the kernels' own masks (tests/dropout_mirror.py).
Sites, as unast_amd.train_rnn.text_decoder_forward lists them: 't_emb_dropout' [slab rows, E], 't_dropout1..3' [slab rows, 256] in the slab
layout of unast_amd.train_rnn.prefix_layout (gap rows carry mask values nobody reads); 'd_drop0', 'd_dropout1', 't_post_dropout' [B*T, 256].

The scalar is L = <logits, R>.  enc_output, h and c are leaves: their gradients are what encoder_backward takes, so the text autoencoder is
the encoder mirror (tests/rnn_train_mirror.run), this mirror, then the encoder mirror again with those three as cotangents (`autoencoder`).

Planted faults (`fault=`):
  'sos_prefix'     position i >= 1 is fed [SOS, target[:, :i-1]] instead of target[:, :i]
  'slab_stats'     the batch statistics are taken over all live rows of all prefixes instead of per prefix
  'running_once'   the running statistics are updated once (with the last prefix's statistics) instead of T times (moves the buffers only)
"""
import numpy as np
import torch
from torch import nn

from tests import rnn_train_mirror as TM
from tests.rnn_decoder_mirror import _cell, memory  # noqa: F401  (memory: case a's random enc_output / h / c)
from unast_amd.train_rnn import prefix_layout, GAP
from unast_amd.utils import SOS_IDX

F = nn.functional
H = 256
FAULTS = ("sos_prefix", "slab_stats", "running_once")
BUFFERS = ("running_mean", "running_var", "num_batches_tracked")
PRE_BN = ["prenet.batch_norm%d" % i for i in (1, 2, 3)]
# conv biases in front of a train-mode BatchNorm: their gradients are mathematically zero (the batch mean absorbs them)
DEGENERATE = ["prenet.conv%d.conv.bias" % i for i in (1, 2, 3)]
# position 0's prefix is [SOS] for every sequence: identical rows, variance 0, rstd = eps^-1/2 = 316 at each stage.  The amplified gradients cancel
# over the batch in exact arithmetic; fp32 leaves a residue in these three (the reference's own fp32 run is 4e-4 .. 3e-3 off its fp64 run)
ILL_CONDITIONED = ["prenet.embed.weight", "prenet.conv1.conv.weight", "prenet.batch_norm1.bias"]


def trained_keys(sd):
    """The parameters text_decoder_backward writes: everything under prenet., decoder. and postnet. that is not a BatchNorm buffer."""
    return [k for k in sd if k.startswith(("prenet.", "decoder.", "postnet.")) and not k.endswith(BUFFERS)]


def cotangent(seed, B, T, V):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((B, T, V)))


def tokens(seed, B, T, lens=None, pad_rows=()):
    """Random non-special token ids [B,T] (3..45); PAD (0) from lens[b] on, and in the second half of the rows listed in pad_rows."""
    ids = np.random.RandomState(seed).randint(3, 46, size=(B, T)).astype(np.int64)
    if lens is not None:
        for b in range(B):
            ids[b, int(lens[b]):] = 0
    for b in pad_rows:
        ids[b, T // 2:] = 0
    return ids


def grad_bounds(e32, cap=1e-3, margin=16.0):
    """Per-tensor bounds from {name: e32}, e32 = the reference's fp32 run against its fp64 run.  The three ILL_CONDITIONED tensors are held to
    margin x their OWN e32, uncapped (the cap would sit below the reference's own fp32 error); every other tensor to
    min(cap, margin x max(common, own)) with the common figure taken as tests/rnn_decoder_mirror.grad_bounds takes it (the largest e32 that is
    not more than 10 x the median, over the well-conditioned tensors).  Returns ({name: bound}, common)."""
    well = {k: v for k, v in e32.items() if k not in ILL_CONDITIONED}
    med = float(np.median(list(well.values())))
    common = max(v for v in well.values() if v <= 10 * med)
    out = {k: min(cap, margin * max(common, v)) for k, v in well.items()}
    out.update({k: margin * e32[k] for k in ILL_CONDITIONED if k in e32})
    return out, common


def conditioned_bounds(e32, cap=1e-3, margin=16.0):
    """The conditioned case (eps = 0.1 on the three prenet BatchNorms): EVERY tensor meets min(cap, margin x common e32)."""
    med = float(np.median(list(e32.values())))
    common = max(v for v in e32.values() if v <= 10 * med)
    return {k: min(cap, margin * max(common, v)) for k, v in e32.items()}, common


def prefix_prenet(P, sd, target, masks, fault, dtype, momentum, eps):
    """TextPrenet over every prefix.  Returns pn [B,T,256] (the last row of every call) and {buffer name: value after the call}."""
    B, T = target.shape
    lay = prefix_layout(B, T)
    sos = torch.full((B, 1), SOS_IDX, dtype=torch.int64)

    def seg_mask(name, s, width):                                                               # the slab rows of segment s -> [B, L_s, width]
        if name not in masks:
            return None
        L = lay.lens[s]
        rows = lay.off[s] + torch.arange(B)[:, None] * (L + GAP) + torch.arange(L)[None, :]
        return masks[name].to(dtype).reshape(lay.total, width)[rows]

    cur = []
    for s in range(T):
        if s == 0:
            tok = sos
        elif fault == "sos_prefix":
            tok = torch.cat([sos, target[:, :s - 1]], 1)
        else:
            tok = target[:, :s]
        e = F.embedding(tok, P["prenet.embed.weight"], padding_idx=0)
        m = seg_mask("t_emb_dropout", s, e.shape[-1])
        cur.append((e if m is None else e * m).transpose(1, 2))                                  # [B, E, L_s]
    bufs = {}
    for i in (1, 2, 3):
        bn = "prenet.batch_norm%d" % i
        w, b = P[bn + ".weight"], P[bn + ".bias"]
        rm, rv = (sd[bn + "." + n].detach().to(dtype).clone() for n in ("running_mean", "running_var"))
        zs = [F.conv1d(x, P["prenet.conv%d.conv.weight" % i], P["prenet.conv%d.conv.bias" % i], padding=2) for x in cur]
        if fault == "slab_stats":
            allz = torch.cat([z.transpose(1, 2).reshape(-1, H) for z in zs], 0)
            g_mean, g_var = allz.mean(0), allz.var(0, unbiased=False)
        nxt = []
        for s, z in enumerate(zs):
            n = z.shape[0] * z.shape[2]
            flat = z.transpose(1, 2).reshape(n, H)
            mean, var = (g_mean, g_var) if fault == "slab_stats" else (flat.mean(0), flat.var(0, unbiased=False))
            if fault != "running_once" or s == T - 1:
                rm = (1 - momentum) * rm + momentum * mean.detach()
                rv = (1 - momentum) * rv + momentum * var.detach() * n / (n - 1)
            y = torch.relu((z - mean[None, :, None]) / torch.sqrt(var[None, :, None] + eps) * w[None, :, None] + b[None, :, None])
            m = seg_mask("t_dropout%d" % i, s, H)
            nxt.append(y if m is None else y * m.transpose(1, 2))
        cur = nxt
        bufs[bn + ".running_mean"], bufs[bn + ".running_var"] = rm, rv
        bufs[bn + ".num_batches_tracked"] = int(sd[bn + ".num_batches_tracked"]) + (1 if fault == "running_once" else T)
    return torch.stack([y[:, :, -1] for y in cur], 1), bufs


def run(sd, attn, target, enc_output, h, c, lens_k, cot, masks=None, fault=None, dtype=torch.float64, momentum=0.1, eps=1e-5):
    """One train-mode decode_sequence and backward.  sd: the model's state dict (CPU tensors); target int64 [B,T]; enc_output [B,Tk,512]; h, c
    [2,B,256]; cot [B,T,V]; masks: {site name: factor tensor [rows, cols]} (a missing site = no dropout); eps: the three prenet BatchNorms'.
    Returns logits, grads {key: tensor}, d_enc_output, d_h, d_c and the prenet BatchNorms' buffers after the call."""
    assert fault in (None,) + FAULTS and attn in ("luong", "lsa")
    masks = masks or {}
    target = torch.as_tensor(target, dtype=torch.int64)
    B, T = target.shape
    Tk = enc_output.shape[1]
    mk = lambda name, shape: masks[name].to(dtype).reshape(shape) if name in masks else None      # noqa: E731
    P = {k: nn.Parameter(sd[k].detach().to(dtype).clone()) for k in trained_keys(sd)}
    leaf = lambda t: torch.as_tensor(t).detach().to(dtype).clone().requires_grad_(True)              # noqa: E731
    enc, h_in, c_in = leaf(enc_output), leaf(h), leaf(c)
    pad = torch.arange(Tk)[None, :] >= torch.as_tensor(np.asarray(lens_k), dtype=torch.int64)[:, None]

    pn, out = prefix_prenet(P, sd, target, masks, fault, dtype, momentum, eps)

    A_ = "decoder.attention_layer."
    if attn == "lsa":
        Wq, Wm, vw = P[A_ + "query_layer.linear_layer.weight"], P[A_ + "memory_layer.linear_layer.weight"], P[A_ + "v.linear_layer.weight"]
        conv_w, dense_w = P[A_ + "location_layer.location_conv.conv.weight"], P[A_ + "location_layer.location_dense.linear_layer.weight"]
        prev, cum = torch.zeros(B, Tk, dtype=dtype), torch.zeros(B, Tk, dtype=dtype)
    else:
        Wq, Wm, vw = P[A_ + "project_hid.weight"], P[A_ + "project_eo.weight"], P[A_ + "fc2.weight"]
    mem = F.linear(enc, Wm)
    R = {n: P["decoder.rnn." + n] for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l1", "weight_hh_l1", "bias_ih_l1", "bias_hh_l1")}
    m_inter, m_out, m_post = mk("d_drop0", (B, T, H)), mk("d_dropout1", (B, T, H)), mk("t_post_dropout", (B, T, H))
    hs, cs = [h_in[0], h_in[1]], [c_in[0], c_in[1]]
    logits = []
    for i in range(T):
        q = hs[1]                                                                                # the top layer's h from BEFORE this position's LSTM
        x = F.linear(q, Wq)[:, None, :] + mem
        if attn == "lsa":
            loc = F.conv1d(torch.stack([prev, cum], 1), conv_w, padding=15).transpose(1, 2)
            x = x + F.linear(loc, dense_w)
        e = F.linear(torch.tanh(x), vw).squeeze(-1).masked_fill(pad, float("-inf"))
        w = torch.softmax(e, 1)
        if attn == "lsa":
            prev, cum = w, cum + w
        ctx = torch.bmm(w[:, None, :], enc)[:, 0]
        hs[0], cs[0] = _cell(torch.cat([pn[:, i], ctx], -1), hs[0], cs[0], R["weight_ih_l0"], R["weight_hh_l0"], R["bias_ih_l0"], R["bias_hh_l0"])
        x1 = hs[0] if m_inter is None else hs[0] * m_inter[:, i]
        hs[1], cs[1] = _cell(x1, hs[1], cs[1], R["weight_ih_l1"], R["weight_hh_l1"], R["bias_ih_l1"], R["bias_hh_l1"])
        o = torch.tanh(F.linear(torch.cat([hs[1], ctx], -1), P["decoder.linear_projection.linear_layer.weight"], P["decoder.linear_projection.linear_layer.bias"]))
        if m_out is not None:
            o = o * m_out[:, i]
        if m_post is not None:
            o = o * m_post[:, i]
        logits.append(F.linear(o, P["postnet.fc1.weight"], P["postnet.fc1.bias"]))
    logits = torch.stack(logits, 1)
    (logits * cot.to(dtype)).sum().backward()
    out.update(logits=logits.detach(), grads={k: (p.grad.detach() if p.grad is not None else torch.zeros_like(p)) for k, p in P.items()},
               d_enc_output=enc.grad.detach(), d_h=h_in.grad.detach(), d_c=c_in.grad.detach())
    return out


def autoencoder(sd, attn, text, lens, cot, enc_masks=None, dec_masks=None, dtype=torch.float64):
    """TextRNN.forward in train mode (encode + decode_sequence, src/network.py:495-500) and the backward of <logits, cot>: the encoder
    mirror's forward, this mirror on the state dict with the encoder's running-statistics update applied (the prenet is shared: the decoder's T
    updates follow the encoder's one), then the encoder mirror again with the decoder's three input gradients as its cotangents.  Returns
    this mirror's result with 'grads' summed over both halves, plus enc_grads, dec_grads, enc_output, h, c."""
    text = torch.as_tensor(text, dtype=torch.int64)
    B, T = text.shape
    zero = (torch.zeros(B, T, 2 * H), torch.zeros(2, B, H), torch.zeros(2, B, H))
    fwd = TM.run("text", sd, text, lens, zero, masks=enc_masks, dtype=dtype)
    sd2 = dict(sd)
    for bn in PRE_BN:
        for n in ("running_mean", "running_var"):
            sd2[bn + "." + n] = fwd[bn + "." + n]
        sd2[bn + ".num_batches_tracked"] = sd[bn + ".num_batches_tracked"] + 1
    dec = run(sd2, attn, text, fwd["enc_output"], fwd["h"], fwd["c"], lens, cot, masks=dec_masks, dtype=dtype)
    enc = TM.run("text", sd, text, lens, (dec["d_enc_output"], dec["d_h"], dec["d_c"]), masks=enc_masks, dtype=dtype)
    grads = dict(dec["grads"])
    for k, g in enc["grads"].items():
        grads[k] = grads[k] + g if k in grads else g
    res = dict(dec)
    res.update(grads=grads, enc_grads=enc["grads"], dec_grads=dec["grads"], enc_output=fwd["enc_output"], h=fwd["h"], c=fwd["c"])
    return res
