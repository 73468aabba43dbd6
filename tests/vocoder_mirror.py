"""Host mirror, in plain torch, of the CBHG vocoder's eval forward (unast_amd.vocoder; reference src/network.py:627-655,
src/module.py:500-626): our own restatement of the semantics, token-major, runnable in fp64.  Tests compare the HIP forward with it at
sizes the fixtures under tests/golden/ do not reach, and compare IT with those fixtures so that the restatement is pinned by the reference.

    pre        x0 = mel W_pre^T + b                                       (k = 1 conv = linear)
    bank       a CHAIN: y_k = relu(BN_k(conv_k(y_{k-1}))), y_0 = x0, k = 1..16; conv_k has k taps and left pad k // 2:
               out[t] = sum_j W[:, :, j] x[t + j - k // 2], zero outside [0, T)   (an even kernel drops the last column)
    concat     [y_1 | ... | y_16] on channels, then p[t] = max(y[t - 1], y[t]), p[0] = y[0]
    proj       relu(BN(conv3(p))) -> BN(conv3(.)) + x0
    highway    4 x: h = relu(W1 x + b1), t = sigmoid(W2 x + b2), x = h t + x (1 - t)
    gru        2 layers, bidirectional, hidden 128, gates r, z, n, zero initial state, over all T positions:
               n = tanh(W_in x + b_in + r (W_hn h + b_hn)), h' = (1 - z) n + z h; layer 1 reads [fwd | bwd]
    post       mag = g W_post^T + b
"""
import torch

EPS = 1e-5


def conv_taps(x, W, b):
    """x [B,T,Cin], W [Cout,Cin,k] (the reference's shape), b [Cout] -> [B,T,Cout] with the padding rule above."""
    B, T, _ = x.shape
    k = W.shape[2]
    left = k // 2
    xp = torch.zeros(B, T + k - 1, x.shape[2], dtype=x.dtype)
    xp[:, left:left + T] = x
    out = b.expand(B, T, -1).clone()
    for j in range(k):
        out = out + xp[:, j:j + T] @ W[:, :, j].t()
    return out


def bn_eval(x, sd, pre):
    return (x - sd[pre + "running_mean"]) / torch.sqrt(sd[pre + "running_var"] + EPS) * sd[pre + "weight"] + sd[pre + "bias"]


def gru_layer(x, w_ih, w_hh, b_ih, b_hh, reverse):
    B, T, _ = x.shape
    H = w_hh.shape[1]
    h = torch.zeros(B, H, dtype=x.dtype)
    out = torch.zeros(B, T, H, dtype=x.dtype)
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        gi = x[:, t] @ w_ih.t() + b_ih
        gh = h @ w_hh.t() + b_hh
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        out[:, t] = h
    return out


def gru(x, sd, pre, layers=2):
    for l in range(layers):
        outs = []
        for sfx, rev in (("_l%d" % l, False), ("_l%d_reverse" % l, True)):
            outs.append(gru_layer(x, sd[pre + "weight_ih" + sfx], sd[pre + "weight_hh" + sfx], sd[pre + "bias_ih" + sfx],
                                  sd[pre + "bias_hh" + sfx], rev))
        x = torch.cat(outs, dim=2)
    return x


def forward(state_dict, mel, dtype=torch.float64, K=16):
    """state_dict: name -> tensor or array with the reference's keys; mel [B,T,80].  Returns (mag [B,T,F], dict of the stage outputs:
    pre, bank [B,T,256 K], pooled, proj, highway, gru), all on the CPU in `dtype`."""
    sd = {k: torch.as_tensor(v).to(dtype) for k, v in state_dict.items() if not k.endswith("num_batches_tracked")}
    x = torch.as_tensor(mel).to(dtype)
    x0 = x @ sd["pre_projection.conv.weight"][:, :, 0].t() + sd["pre_projection.conv.bias"]
    y, stages = x0, []
    for k in range(1, K + 1):
        y = conv_taps(y, sd["cbhg.convbank_list.%d.weight" % (k - 1)], sd["cbhg.convbank_list.%d.bias" % (k - 1)])
        y = torch.relu(bn_eval(y, sd, "cbhg.batchnorm_list.%d." % (k - 1)))
        stages.append(y)
    bank = torch.cat(stages, dim=2)
    pooled = bank.clone()
    pooled[:, 1:] = torch.maximum(bank[:, 1:], bank[:, :-1])
    p = conv_taps(pooled, sd["cbhg.conv_projection_1.weight"], sd["cbhg.conv_projection_1.bias"])
    p = torch.relu(bn_eval(p, sd, "cbhg.batchnorm_proj_1."))
    p = conv_taps(p, sd["cbhg.conv_projection_2.weight"], sd["cbhg.conv_projection_2.bias"])
    proj = bn_eval(p, sd, "cbhg.batchnorm_proj_2.") + x0
    h = proj
    for i in range(4):
        a = torch.relu(h @ sd["cbhg.highway.linears.%d.linear_layer.weight" % i].t() + sd["cbhg.highway.linears.%d.linear_layer.bias" % i])
        t = torch.sigmoid(h @ sd["cbhg.highway.gates.%d.linear_layer.weight" % i].t() + sd["cbhg.highway.gates.%d.linear_layer.bias" % i])
        h = a * t + h * (1 - t)
    g = gru(h, sd, "cbhg.gru.")
    mag = g @ sd["post_projection.conv.weight"][:, :, 0].t() + sd["post_projection.conv.bias"]
    return mag, dict(pre=x0, bank=bank, pooled=pooled, proj=proj, highway=h, gru=g)
