"""fp64 torch restatement of SpeechRNN's teacher-forced train-mode decoder (decode_sequence at teacher_ratio = 1, src/network.py:352-392;
RNNDecoder.forward and both attention layers, src/module.py:362-497; SpeechPostnet, src/module.py:155-171) with autograd.  Dropout is an
explicit factor tensor per site (0 or 1/(1-p)), so that a test can impose the kernels' own masks (tests/dropout_mirror.py); the two layers
of the decoder's nn.LSTM are written out as cells so that the inter-layer dropout takes a given mask.

Sites (rows in [B, T] order, as unast_amd.train_rnn lists them): 'd_prenet_dropout', 'd_drop0' (inter-layer), 'd_dropout1' [B*T, 256];
'post_dropout0..3' [B*(T+1), 256].

The scalar is L = <pre, R1> + <post, R2> + <stop, R3> with the cotangents of `cotangents(seed, ...)`.  enc_output, h and c are leaves:
their gradients are what encoder_backward takes, so the autoencoder (SpeechRNN.forward) is this mirror followed by
tests/rnn_train_mirror.run with those three as its cotangents (`autoencoder`).

Planted faults (`fault=`), both in the backward only (the forward values are unchanged):
  'query_after_lstm'   the attention query's gradient joins the top layer's carry one position off.  (The literal mistake -- the query taken
                       from h after the position's LSTM -- is a cycle, since that h depends on the context; in a hand-written backward loop it
                       shows as the query gradient being added to the carry of the wrong position, which is what is planted: position i's
                       query gradient goes to h1_{i-2} instead of h1_{i-1}: at i = 1 that is the encoder's h, so it lands in d_h; it is lost only at i = 0.)
  'lsa_cum_dropped'    location-sensitive attention's gradient through the cumulative weights is dropped (cum enters detached)
"""
import numpy as np
import torch
from torch import nn

from tests import rnn_train_mirror as TM

F = nn.functional
H = 256
FAULTS = ("query_after_lstm", "lsa_cum_dropped")
# conv biases in front of a train-mode BatchNorm: their gradients are mathematically zero (the batch mean absorbs them)
DEGENERATE = ["postnet.conv1.conv.bias"] + ["postnet.conv_list.%d.conv.bias" % i for i in range(3)]
BUFFERS = ("running_mean", "running_var", "num_batches_tracked")
POST_BN = ["postnet.pre_batchnorm"] + ["postnet.batch_norm_list.%d" % i for i in range(3)]
POST_CONV = ["postnet.conv1.conv"] + ["postnet.conv_list.%d.conv" % i for i in range(3)]


def trained_keys(sd):
    """The parameters decoder_backward writes: everything under prenet., decoder. and postnet. that is not a BatchNorm buffer."""
    return [k for k in sd if k.startswith(("prenet.", "decoder.", "postnet.")) and not k.endswith(BUFFERS)]


def cotangents(seed, B, T, M):
    r = np.random.RandomState(seed)
    return (torch.from_numpy(r.standard_normal((B, T, M))), torch.from_numpy(r.standard_normal((B, T, M))), torch.from_numpy(r.standard_normal((B, T))))


def memory(seed, B, Tk, lens_k):
    """Case (a)'s text-shaped memory: random enc_output [B,Tk,512] with zero rows past lens_k, random (h, c) [2,B,256]."""
    r = np.random.RandomState(seed)
    enc = r.standard_normal((B, Tk, 2 * H)) * 0.5
    for b in range(B):
        enc[b, int(lens_k[b]):] = 0.0
    return enc.astype(np.float32), (r.standard_normal((2, B, H)) * 0.5).astype(np.float32), (r.standard_normal((2, B, H)) * 0.5).astype(np.float32)


def grad_bounds(e32, cap=1e-3, margin=16.0):
    """Per-tensor bounds min(cap, margin x e32) from {name: e32}, e32 = a fp32 run's error against the fp64 run of the same case.  DESIGN 5i
    takes one e32 per case, the largest over the non-degenerate gradients; here a tensor whose own e32 stands out (more than 10 x the case's
    median: the autoencoder case's query projection, a gradient of norm 0.04 left by cancellation, 1e-4 in the reference's own fp32 run)
    would lift every other tensor's bound to the cap, so it is kept out of the common figure and held to its own e32.
    Returns ({name: bound}, the common e32)."""
    med = float(np.median(list(e32.values())))
    common = max(v for v in e32.values() if v <= 10 * med)
    return {k: min(cap, margin * max(common, v)) for k, v in e32.items()}, common


def _cell(x, h, c, w_ih, w_hh, b_ih, b_hh):
    i, f, g, o = (F.linear(x, w_ih, b_ih) + F.linear(h, w_hh, b_hh)).chunk(4, -1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


def run(sd, attn, target, enc_output, h, c, lens_k, cot, masks=None, fault=None, dtype=torch.float64, momentum=0.1, eps=1e-5):
    """One train-mode decode_sequence and backward.  sd: the model's state dict (CPU tensors); target [B,T,M]; enc_output [B,Tk,512]; h, c
    [2,B,256]; masks: {site name: factor tensor [rows, cols]} (a missing site = no dropout).  Returns pre, post, stop, grads {key: tensor},
    d_enc_output, d_h, d_c and the post-net's BatchNorm running statistics after the call."""
    assert fault in (None,) + FAULTS and attn in ("luong", "lsa")
    masks = masks or {}
    B, T, M = target.shape
    Tk = enc_output.shape[1]
    mk = lambda name, shape: masks[name].to(dtype).reshape(shape) if name in masks else None      # noqa: E731
    P = {k: nn.Parameter(sd[k].detach().to(dtype).clone()) for k in trained_keys(sd)}
    leaf = lambda t: torch.as_tensor(t).detach().to(dtype).clone().requires_grad_(True)              # noqa: E731
    enc, h_in, c_in = leaf(enc_output), leaf(h), leaf(c)
    tgt = torch.as_tensor(target).detach().to(dtype)
    lens_t = torch.as_tensor(np.asarray(lens_k), dtype=torch.int64)
    pad = torch.arange(Tk)[None, :] >= lens_t[:, None]

    feed = torch.cat([torch.zeros(B, 1, M, dtype=dtype), tgt[:, :-1]], 1)
    v = torch.relu(F.linear(feed, P["prenet.layer.fc1.linear_layer.weight"], P["prenet.layer.fc1.linear_layer.bias"]))
    m = mk("d_prenet_dropout", v.shape)
    if m is not None:
        v = v * m
    pn = torch.relu(F.linear(v, P["prenet.layer.fc2.linear_layer.weight"], P["prenet.layer.fc2.linear_layer.bias"]))

    A_ = "decoder.attention_layer."
    if attn == "lsa":
        Wq, Wm, vw = P[A_ + "query_layer.linear_layer.weight"], P[A_ + "memory_layer.linear_layer.weight"], P[A_ + "v.linear_layer.weight"]
        conv_w, dense_w = P[A_ + "location_layer.location_conv.conv.weight"], P[A_ + "location_layer.location_dense.linear_layer.weight"]
        prev, cum = torch.zeros(B, Tk, dtype=dtype), torch.zeros(B, Tk, dtype=dtype)
    else:
        Wq, Wm, vw = P[A_ + "project_hid.weight"], P[A_ + "project_eo.weight"], P[A_ + "fc2.weight"]
    mem = F.linear(enc, Wm)
    R = {n: P["decoder.rnn." + n] for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l1", "weight_hh_l1", "bias_ih_l1", "bias_hh_l1")}
    m_inter, m_out = mk("d_drop0", (B, T, H)), mk("d_dropout1", (B, T, H))
    hs, cs = [h_in[0], h_in[1]], [c_in[0], c_in[1]]
    h1_hist = [None, hs[1]]                                                                      # h1 before positions i-1 and i
    mels, stops = [], []
    for i in range(T):
        q = hs[1]                                                                                # the top layer's h from BEFORE this position's LSTM
        if fault == "query_after_lstm":
            wrong = h1_hist[-2]
            q = q.detach() if wrong is None else q.detach() + (wrong - wrong.detach())
        x = F.linear(q, Wq)[:, None, :] + mem
        if attn == "lsa":
            cum_in = cum.detach() if fault == "lsa_cum_dropped" else cum
            loc = F.conv1d(torch.stack([prev, cum_in], 1), conv_w, padding=15).transpose(1, 2)
            x = x + F.linear(loc, dense_w)
        e = F.linear(torch.tanh(x), vw).squeeze(-1).masked_fill(pad, float("-inf"))
        w = torch.softmax(e, 1)
        if attn == "lsa":
            prev, cum = w, cum + w
        ctx = torch.bmm(w[:, None, :], enc)[:, 0]
        hs[0], cs[0] = _cell(torch.cat([pn[:, i], ctx], -1), hs[0], cs[0], R["weight_ih_l0"], R["weight_hh_l0"], R["bias_ih_l0"], R["bias_hh_l0"])
        x1 = hs[0] if m_inter is None else hs[0] * m_inter[:, i]
        hs[1], cs[1] = _cell(x1, hs[1], cs[1], R["weight_ih_l1"], R["weight_hh_l1"], R["bias_ih_l1"], R["bias_hh_l1"])
        h1_hist.append(hs[1])
        o = torch.tanh(F.linear(torch.cat([hs[1], ctx], -1), P["decoder.linear_projection.linear_layer.weight"], P["decoder.linear_projection.linear_layer.bias"]))
        if m_out is not None:
            o = o * m_out[:, i]
        mels.append(F.linear(o, P["postnet.linear_project.weight"], P["postnet.linear_project.bias"]))
        stops.append(F.linear(o, P["postnet.stop_linear.weight"], P["postnet.stop_linear.bias"]))
    outs = torch.cat([torch.zeros(B, 1, M, dtype=dtype), torch.stack(mels, 1)], 1)
    stop = torch.cat(stops, 1)

    out = {}
    x = outs.transpose(1, 2)
    for k in range(4):
        x = F.conv1d(x, P[POST_CONV[k] + ".weight"], P[POST_CONV[k] + ".bias"], padding=4)[:, :, :-4]
        rm, rv = (sd[POST_BN[k] + "." + s].detach().to(dtype).clone() for s in ("running_mean", "running_var"))
        x = torch.tanh(F.batch_norm(x, rm, rv, P[POST_BN[k] + ".weight"], P[POST_BN[k] + ".bias"], True, momentum, eps))
        out[POST_BN[k] + ".running_mean"], out[POST_BN[k] + ".running_var"] = rm, rv
        m = mk("post_dropout%d" % k, (B, T + 1, H))
        if m is not None:
            x = x * m.transpose(1, 2)
    x = F.conv1d(x, P["postnet.conv2.conv.weight"], P["postnet.conv2.conv.bias"], padding=4)[:, :, :-4]
    post = outs + x.transpose(1, 2)
    pre, post = outs[:, 1:], post[:, 1:]
    r1, r2, r3 = (t.to(dtype) for t in cot)
    ((pre * r1).sum() + (post * r2).sum() + (stop * r3).sum()).backward()
    out.update(pre=pre.detach(), post=post.detach(), stop=stop.detach(), grads={k: p.grad.detach() for k, p in P.items()},
               d_enc_output=enc.grad.detach(), d_h=h_in.grad.detach(), d_c=c_in.grad.detach())
    return out


def autoencoder(sd, attn, mel, lens, cot, enc_masks=None, dec_masks=None, dtype=torch.float64):
    """SpeechRNN.forward in train mode (src/network.py:397-402) and the backward of the same scalar: the encoder mirror's forward, this
    decoder mirror, then the encoder mirror again with the decoder's three input gradients as its cotangents (the chain rule the entry points
    follow).  The teacher-forcing frames are constants (no gradient flows from them into d_mel).  Returns the decoder mirror's result with
    'grads' summed over both halves (the prenet is shared), plus enc_grads, dec_grads, d_mel, enc_output, h, c."""
    B, T = mel.shape[:2]
    zero = (torch.zeros(B, T, 2 * H), torch.zeros(2, B, H), torch.zeros(2, B, H))
    fwd = TM.run("speech", sd, mel, lens, zero, masks=enc_masks, dtype=dtype)
    dec = run(sd, attn, mel, fwd["enc_output"], fwd["h"], fwd["c"], lens, cot, masks=dec_masks, dtype=dtype)
    enc = TM.run("speech", sd, mel, lens, (dec["d_enc_output"], dec["d_h"], dec["d_c"]), masks=enc_masks, dtype=dtype)
    grads = dict(dec["grads"])
    for k, g in enc["grads"].items():
        grads[k] = grads[k] + g if k in grads else g
    res = dict(dec)
    res.update(grads=grads, enc_grads=enc["grads"], dec_grads=dec["grads"], d_mel=enc["d_mel"], enc_output=fwd["enc_output"], h=fwd["h"], c=fwd["c"])
    return res
