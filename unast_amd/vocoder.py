"""CBHG vocoder, eval forward: mel [B,T,80] -> magnitude spectrogram [B,T,1025] (src/network.py:627-655, src/module.py:500-626),
executed by HIP kernels on the token-major layout [B*T, C].

Parameters live in torch.nn containers with the reference's names, shapes, order and initialisation, so `state_dict()` /
`load_state_dict()` speak the reference's 162 keys and a reference-trained checkpoint loads unchanged.  What the kernels read is a
derived, cached copy (`_Pack`), rebuilt when any parameter's or buffer's version counter moves (load_state_dict, .to(), manual
edits): conv weights tap-major [Cout,k,Cin] with the eval BatchNorm folded in, each highway layer's [linears.i | gates.i] as one
[512,256] matrix, each GRU layer's weight_ih of both directions as one [768,256] matrix.

Supported: Vocoder(num_mels, 256, num_fft) with num_mels a multiple of 4 (the reference builds Vocoder(80, 256, 2048)); eval mode under
torch.no_grad() only.  Training has its own entry point, unast_amd.train_vocoder.vocoder_step (this forward keeps refusing train mode).
The magnitudes become waveforms in unast_amd.audio (spectrogram2wav_batch, mel2wav: Griffin-Lim on csrc/audio.hip), which reads this
forward's output as it is, padded rows included.
"""
import torch
import torch.nn as nn

from . import contract, ops
from .module import Linear, _no_forward

_F32 = torch.float32


class _Conv1(nn.Module):
    """src/module.py:42-73 at its default kernel_size=1 (the vocoder's pre / post projection)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size=1)
        nn.init.xavier_uniform_(self.conv.weight, gain=nn.init.calculate_gain('linear'))
    forward = _no_forward


class Highwaynet(nn.Module):
    """src/module.py:500-530 (gates registered before linears, as there)."""

    def __init__(self, num_units, num_layers=4):
        super().__init__()
        self.num_units, self.num_layers = num_units, num_layers
        self.gates = nn.ModuleList()
        self.linears = nn.ModuleList()
        for _ in range(num_layers):
            self.linears.append(Linear(num_units, num_units))
            self.gates.append(Linear(num_units, num_units))
    forward = _no_forward


class CBHG(nn.Module):
    """src/module.py:533-626."""

    def __init__(self, hidden_size, K=16, projection_size=256, num_gru_layers=2, max_pool_kernel_size=2):
        super().__init__()
        if hidden_size != 256 or projection_size != 256 or K < 1 or K > 16 or num_gru_layers != 2 or max_pool_kernel_size != 2:
            raise NotImplementedError("the HIP CBHG is built for hidden_size=256, projection_size=256, K<=16, 2 GRU layers of hidden 128, "
                                      "max pool 2 (src/network.py:642 builds CBHG(256))")
        self.hidden_size, self.projection_size, self.K = hidden_size, projection_size, K
        self.convbank_list = nn.ModuleList([nn.Conv1d(projection_size if k == 1 else hidden_size, hidden_size, kernel_size=k, padding=k // 2)
                                            for k in range(1, K + 1)])
        self.batchnorm_list = nn.ModuleList([nn.BatchNorm1d(hidden_size) for _ in range(K)])
        self.conv_projection_1 = nn.Conv1d(hidden_size * K, hidden_size, kernel_size=3, padding=1)
        self.conv_projection_2 = nn.Conv1d(hidden_size, projection_size, kernel_size=3, padding=1)
        self.batchnorm_proj_1 = nn.BatchNorm1d(hidden_size)
        self.batchnorm_proj_2 = nn.BatchNorm1d(projection_size)
        self.highway = Highwaynet(projection_size)
        self.gru = nn.GRU(projection_size, hidden_size // 2, num_layers=num_gru_layers, batch_first=True, bidirectional=True)
    forward = _no_forward


def highway_operands(highway):
    """Each highway layer's [linears.i | gates.i] as one (weight [2C, C], bias [2C])."""
    return [(torch.cat([l.linear_layer.weight, g.linear_layer.weight]).contiguous(),
             torch.cat([l.linear_layer.bias, g.linear_layer.bias]).contiguous()) for l, g in zip(highway.linears, highway.gates)]


def gru_operands(gru, layer):
    """One layer's operands as the GRU kernels read them: weight_ih of both directions [6H, In], its bias with b_hr, b_hz added, weight_hh
    [2, 3H, H], b_hn [2, H]."""
    H = gru.hidden_size
    w_ih, b_x, w_hh, b_hn = [], [], [], []
    for sfx in ("_l%d" % layer, "_l%d_reverse" % layer):
        b_ih, b_hh = getattr(gru, "bias_ih" + sfx), getattr(gru, "bias_hh" + sfx)
        w_ih.append(getattr(gru, "weight_ih" + sfx))
        w_hh.append(getattr(gru, "weight_hh" + sfx))
        bx = b_ih.clone()
        bx[:2 * H] += b_hh[:2 * H]              # b_hr, b_hz only ever appear summed with b_ir, b_iz; b_hn sits inside r * (.)
        b_x.append(bx)
        b_hn.append(b_hh[2 * H:])
    return torch.cat(w_ih).contiguous(), torch.cat(b_x).contiguous(), torch.stack(w_hh).contiguous(), torch.stack(b_hn).contiguous()


class _Pack:
    """The operands the kernels read, derived from the parameters (module docstring)."""

    def __init__(self, m):
        c = m.cbhg
        with torch.no_grad():
            self.pre_w = m.pre_projection.conv.weight[:, :, 0].contiguous()
            self.pre_b = m.pre_projection.conv.bias.detach()
            self.bank = [contract.fold_bn(conv, bn) for conv, bn in zip(c.convbank_list, c.batchnorm_list)]
            self.proj1 = contract.fold_bn(c.conv_projection_1, c.batchnorm_proj_1)
            self.proj2 = contract.fold_bn(c.conv_projection_2, c.batchnorm_proj_2)
            self.highway = highway_operands(c.highway)
            self.gru = [gru_operands(c.gru, layer) for layer in range(c.gru.num_layers)]
            self.post_w = m.post_projection.conv.weight[:, :, 0].contiguous()
            self.post_b = m.post_projection.conv.bias.detach()


class Vocoder(nn.Module):
    """src/network.py:627-655.  forward(mel [B,T,num_mels]) -> mag [B,T,num_fft//2+1] (a view of a buffer with a 16-byte row stride)."""

    def __init__(self, num_mels, hidden_size, num_fft):
        super().__init__()
        if num_mels % 4 != 0 or num_mels <= 0 or num_fft < 2:
            raise NotImplementedError("the HIP vocoder needs num_mels %% 4 == 0 (got %d; every reference config uses 80)" % num_mels)
        self.num_mels, self.hidden_size, self.num_bins = num_mels, hidden_size, num_fft // 2 + 1
        self.pre_projection = _Conv1(num_mels, hidden_size)
        self.cbhg = CBHG(hidden_size)
        self.post_projection = _Conv1(hidden_size, self.num_bins)

    def _pack(self):
        return contract.cached_operands(self, "_vocoder_pack", list(self.parameters()) + list(self.buffers()), lambda: _Pack(self))

    def forward(self, mel):
        return self._run(mel, None)

    def forward_with_intermediates(self, mel):
        """(mag, dict of the stage outputs as [B,T,C] tensors): pre, bank (the [B,T,4096] concat), pooled, proj, highway, gru."""
        taps = {}
        return self._run(mel, taps), taps

    def _run(self, mel, taps):
        if self.training:
            raise NotImplementedError("Vocoder.forward is the eval forward only (BatchNorm running statistics, no backward); call "
                                      "model.eval() and run under torch.no_grad() -- the train-mode step is unast_amd.train_vocoder.vocoder_step")
        if torch.is_grad_enabled():
            raise NotImplementedError("Vocoder.forward has no backward on this path; run it under torch.no_grad()")
        if mel.dim() != 3 or mel.shape[2] != self.num_mels or not mel.is_cuda or mel.dtype is not _F32:
            raise ValueError("Vocoder.forward: mel must be a float32 CUDA tensor [B, T, %d]" % self.num_mels)
        P = self._pack()
        B, T, M = mel.shape
        N, C, K = B * T, self.hidden_size, self.cbhg.K
        dev = mel.device

        def buf(*shape):
            return torch.empty(*shape, dtype=_F32, device=dev)
        x2 = mel.contiguous().view(N, M)
        x0 = buf(N, C)                                      # pre_projection: a k=1 conv is a linear
        ops.gemm(ops.OP_KC, ops.OP_KC, x2, M, P.pre_w, M, x0, C, N, C, M, bias=P.pre_b)
        # convolution bank: a CHAIN -- stage k reads stage k-1 (src/module.py:605-607) -- each stage written into its column slice
        cat = buf(B, T, K * C)
        src = x0.view(B, T, C)
        for k in range(1, K + 1):
            w, b = P.bank[k - 1]
            dst = cat[:, :, (k - 1) * C:k * C]
            ops.conv_taps_fwd(src, w, b, dst, k // 2, act=1)
            src = dst
        pooled = ops.maxpool_prev(cat, buf(B, T, K * C))
        p1 = ops.conv_taps_fwd(pooled, P.proj1[0], P.proj1[1], buf(B, T, C), 1, act=1)
        p2 = ops.conv_taps_fwd(p1, P.proj2[0], P.proj2[1], buf(B, T, C), 1, act=0, R=x0)
        h = p2.view(N, C)
        ht = buf(N, 2 * C)
        hw = buf(N, C)
        for w, b in P.highway:
            ops.gemm(ops.OP_KC, ops.OP_KC, h, C, w, C, ht, 2 * C, N, 2 * C, C, bias=b)
            ops.highway_combine(ht, h, hw)
            h = hw
        if taps is not None:
            hw_out = h.clone()
        g = h
        xproj = buf(B, T, 3 * C)
        for w_ih, b_x, w_hh, b_hn in P.gru:
            ops.gemm(ops.OP_KC, ops.OP_KC, g, C, w_ih, C, xproj, 3 * C, N, 3 * C, C, bias=b_x)
            y = ops.gru_fwd(xproj, w_hh, b_hn, buf(B, T, C))
            g = y.view(N, C)
        F_ = self.num_bins
        ld = (F_ + 3) // 4 * 4
        out = buf(N, ld)
        ops.gemm(ops.OP_KC, ops.OP_KC, g, C, P.post_w, C, out, ld, N, F_, C, bias=P.post_b)
        if taps is not None:
            taps.update(pre=x0.view(B, T, C), bank=cat, pooled=pooled, proj=p2, highway=hw_out.view(B, T, C), gru=g.view(B, T, C))
        return out.view(B, T, ld)[:, :, :F_]


def make_mags(model, mel, mel_lens):
    """src/inf_vocoder.py:56-64 without its file I/O: the magnitude frames of each utterance up to its length, a list of
    [mel_len_i, num_fft//2+1] tensors (views of the batch output)."""
    with torch.no_grad():
        mags = model.forward(mel)
    lens = mel_lens.tolist() if hasattr(mel_lens, "tolist") else list(mel_lens)
    return [mag[:int(n)] for mag, n in zip(mags, lens)]
