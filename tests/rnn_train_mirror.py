"""fp64 torch restatement of the RNN family's train-mode encoders (TextRNN.encode / SpeechRNN.encode, src/network.py:295-310, 514-537;
src/module.py:95-110, 217-230, 313-336) with autograd: nn.Embedding, nn.Conv1d, nn.BatchNorm1d (batch statistics) and nn.LSTM on packed
sequences.  Dropout and noise are explicit masks (factors 0 or 1/(1-p) per element; row keep flags for noise_fn), so that a test can impose
the kernels' own masks (tests/dropout_mirror.py).  The two layers of the encoder's nn.LSTM are two single-layer modules so that the
inter-layer dropout takes a given mask.

The scalar is L = <enc_output, R1> + <h, R2> + <c, R3> with the cotangents of `cotangents(seed, ...)`.

Planted faults (`fault=`), both in the backward only (the forward values are unchanged):
  'dhfinal_reverse_at_end'   the gradient of the reverse direction's final h enters at t = lens[b]-1 instead of t = 0
  'edrop_no_rescale'         the inter-layer dropout's backward multiplies by the keep flag without 1/(1-p)
"""
import numpy as np
import torch
from torch import nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

H = 256
NOISE_P = 0.3
SAMPLE_MAX = 2048            # (48 gradients of 4096 float64 samples would not fit one fixture file)
# conv biases in front of a train-mode BatchNorm: their gradients are mathematically zero (the batch mean absorbs them)
DEGENERATE = ["prenet.conv%d.conv.bias" % i for i in (1, 2, 3)]
FAULTS = ("dhfinal_reverse_at_end", "edrop_no_rescale")


def trained_keys(sd):
    """The parameters encoder_backward writes: everything under prenet. and encoder. that is not a BatchNorm buffer."""
    return [k for k in sd if (k.startswith("prenet.") or k.startswith("encoder.")) and not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]


def sample(v):
    """Strided sample of at most SAMPLE_MAX elements of a tensor / array, flat."""
    flat = np.asarray(v, dtype=np.float64).reshape(-1)
    return flat[::max(1, -(-flat.size // SAMPLE_MAX))]


def cotangents(seed, B, T, L=2):
    r = np.random.RandomState(seed)
    return (torch.from_numpy(r.standard_normal((B, T, 2 * H))), torch.from_numpy(r.standard_normal((L, B, H))), torch.from_numpy(r.standard_normal((L, B, H))))


def _p(sd, k, dtype):
    return nn.Parameter(sd[k].detach().to(dtype).clone())


def run(side, sd, x, lens, cot, masks=None, fault=None, dtype=torch.float64, momentum=0.1, eps=1e-5):
    """One train-mode encode and backward.  side 'text' (x int64 [B,T]) or 'speech' (x [B,T,M]); sd: the model's state dict (CPU tensors);
    masks: {site name: factor tensor [rows, cols] or, for 'noise', keep flags [rows]} (a missing site = no dropout).  Returns enc_output, h, c,
    grads {key: tensor}, d_mel (speech), and the BatchNorm running statistics after the call."""
    assert fault in (None,) + FAULTS
    masks = masks or {}
    B, T = x.shape[:2]
    N = B * T
    mk = lambda name, shape: masks[name].to(dtype).reshape(shape) if name in masks else None      # noqa: E731
    P = {k: _p(sd, k, dtype) for k in trained_keys(sd)}
    out = {}
    d_in = None
    if side == "text":
        e = nn.functional.embedding(x, P["prenet.embed.weight"], padding_idx=0)                    # the row is read; only its gradient is zero
        m = mk("emb_dropout", e.shape)
        if m is not None:
            e = e * m
        m = mk("noise", (B, T, 1))
        if m is not None:
            e = e * m
        cur = e.transpose(1, 2)
        for i in (1, 2, 3):
            cur = nn.functional.conv1d(cur, P["prenet.conv%d.conv.weight" % i], P["prenet.conv%d.conv.bias" % i], padding=2)
            rm, rv = (sd["prenet.batch_norm%d.%s" % (i, s)].detach().to(dtype).clone() for s in ("running_mean", "running_var"))
            cur = nn.functional.batch_norm(cur, rm, rv, P["prenet.batch_norm%d.weight" % i], P["prenet.batch_norm%d.bias" % i], True, momentum, eps)
            out["prenet.batch_norm%d.running_mean" % i], out["prenet.batch_norm%d.running_var" % i] = rm, rv
            cur = torch.relu(cur)
            m = mk("dropout%d" % i, (B, T, H))
            if m is not None:
                cur = cur * m.transpose(1, 2)
        feat = cur.transpose(1, 2)
    else:
        d_in = x.detach().to(dtype).clone().requires_grad_(True)
        v = d_in
        m = mk("noise", (B, T, 1))
        if m is not None:
            v = v * m
        v = torch.relu(nn.functional.linear(v, P["prenet.layer.fc1.linear_layer.weight"], P["prenet.layer.fc1.linear_layer.bias"]))
        m = mk("dropout2", v.shape)
        if m is not None:
            v = v * m
        feat = torch.relu(nn.functional.linear(v, P["prenet.layer.fc2.linear_layer.weight"], P["prenet.layer.fc2.linear_layer.bias"]))

    lens_t = torch.as_tensor(lens, dtype=torch.int64)
    hs, cs = [], []
    cur = feat
    for l in range(2):
        lstm = nn.LSTM(cur.shape[-1], H, num_layers=1, bidirectional=True, batch_first=True).to(dtype)
        for sfx in ("", "_reverse"):
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                delattr(lstm, n + "_l0" + sfx)
                setattr(lstm, n + "_l0" + sfx, P["encoder.rnn.%s_l%d%s" % (n, l, sfx)])
        lstm._flat_weights = [getattr(lstm, n) for n in lstm._flat_weights_names]
        po, (hn, cn) = lstm(pack_padded_sequence(cur, lens_t, batch_first=True, enforce_sorted=False))
        y, _ = pad_packed_sequence(po, batch_first=True, total_length=T)
        h_rev = hn[1]
        if fault == "dhfinal_reverse_at_end":
            wrong = y[torch.arange(B), lens_t - 1, H:]
            h_rev = h_rev.detach() + (wrong - wrong.detach())
        h_cat, c_cat = torch.cat([hn[0], h_rev], -1), torch.cat([cn[0], cn[1]], -1)
        hs.append(nn.functional.linear(h_cat, P["encoder.reduce_h_W.weight"], P["encoder.reduce_h_W.bias"]))
        cs.append(nn.functional.linear(c_cat, P["encoder.reduce_c_W.weight"], P["encoder.reduce_c_W.bias"]))
        cur = y
        if l == 0:
            m = mk("e_drop0", y.shape)
            if m is not None:
                if fault == "edrop_no_rescale":
                    keep = (m != 0).to(dtype)
                    cur = y * keep + (y * (m - keep)).detach()
                else:
                    cur = y * m
    enc, h, c = cur, torch.stack(hs), torch.stack(cs)
    r1, r2, r3 = (t.to(dtype) for t in cot)
    L = (enc * r1).sum() + (h * r2).sum() + (c * r3).sum()
    L.backward()
    out.update(enc_output=enc.detach(), h=h.detach(), c=c.detach(), grads={k: p.grad.detach() for k, p in P.items()},
               d_mel=None if d_in is None else d_in.grad.detach())
    return out


def normerr(got, ref):
    ref = ref.double()
    return ((got.double() - ref).norm() / ref.norm().clamp_min(1e-300)).item()
