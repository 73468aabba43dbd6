"""GPU parity of the CBHG vocoder's eval forward (unast_amd.vocoder, csrc/vocoder.hip, unast_conv_fwd): the reference's fixtures, the
conv entry point over tap counts against fp64 conv1d, the GRU recurrence against fp64 torch.nn.GRU, the full-size forward against the
fp64 mirror (tests/vocoder_mirror.py, itself pinned by the fixtures in tests/test_cpu_vocoder.py), make_mags and the state_dict round trip.

Achieved errors (MI355X) are printed by every test and recorded in DESIGN.md section 3.
"""
import os

import numpy as np
import pytest
import torch

from tests import vocoder_mirror as VM

pytestmark = pytest.mark.gpu

FIXTURES = ["vocoder_b2_t37", "vocoder_b3_t64"]
BAR = 1e-3            # the project's standing bar on end-to-end tensors: 1e-3 of max |ref|
GEMM_TOL = 5e-5       # three-term split-bf16 contraction against fp64, relative to max |ref|
GRU_TOL = 2e-5        # fp32 VALU recurrence against fp64 (the bound of test_lstm_fwd_bwd_matches_torch_packed)


def dev():
    return torch.device("cuda:0")


def relerr(a, b):
    b = b.double()
    return ((a.double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def portable_sd(seed=1234):
    from unast_amd.network import Vocoder
    from unast_amd.portable import portable_tensor
    return {k: torch.from_numpy(portable_tensor(k, tuple(v.shape), seed)) for k, v in Vocoder(80, 256, 2048).state_dict().items()}


def make_model(sd):
    from unast_amd.network import Vocoder
    m = Vocoder(80, 256, 2048)
    m.load_state_dict(sd)
    return m.to(dev()).eval()


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_parity(golden_dir, name):
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    model = make_model(portable_sd(int(fx["meta"][2])))
    with torch.no_grad():
        mag, st = model.forward_with_intermediates(torch.from_numpy(fx["mel"]).to(dev()))
    assert tuple(mag.shape) == tuple(fx["out"].shape) and mag.stride(1) % 4 == 0
    cols, pcols = torch.from_numpy(fx["cols"]).to(dev()), torch.from_numpy(fx["pooled_cols"]).to(dev())
    got = {"out": mag, "pre": st["pre"][..., cols], "bank1": st["bank"][..., 0:256][..., cols], "bank2": st["bank"][..., 256:512][..., cols],
           "bank16": st["bank"][..., 3840:4096][..., cols], "pooled": st["pooled"][..., pcols], "proj": st["proj"][..., cols],
           "highway": st["highway"][..., cols], "gru": st["gru"][..., cols]}
    worst = {k: relerr(v, torch.from_numpy(fx[k])) for k, v in got.items()}
    print(name, {k: "%.2e" % e for k, e in worst.items()})
    assert max(worst.values()) < BAR, worst


def conv_ref(x, W, b, k):
    """fp64 conv1d with the vocoder's padding rule: left pad k // 2, output length T (an even kernel drops the last column)."""
    xp = torch.nn.functional.pad(x.transpose(1, 2), (k // 2, k - 1 - k // 2))
    return torch.nn.functional.conv1d(xp, W, b).transpose(1, 2)


@pytest.mark.parametrize("Cin", [80, 256, 4096])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 7, 8, 15, 16])
def test_conv_tap_sweep(k, Cin):
    from unast_amd import ops
    B, T, Cout = 3, 45, 256                                 # T odd, 135 rows: not a multiple of the 128-row tile
    g = torch.Generator().manual_seed(1000 * k + Cin)
    x = torch.randn(B, T, Cin, generator=g, dtype=torch.float64)
    W = torch.randn(Cout, Cin, k, generator=g, dtype=torch.float64) * 0.05
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    ref = conv_ref(x, W, b, k)
    Wp = W.permute(0, 2, 1).contiguous().float().to(dev())
    y = torch.empty(B, T, Cout, device=dev())
    ops.conv_taps_fwd(x.float().to(dev()), Wp, b.float().to(dev()), y, k // 2)
    e = relerr(y, ref)
    print("conv taps %d Cin %d: %.2e" % (k, Cin, e), end="; ")
    assert e < GEMM_TOL


def test_conv_epilogue_and_column_slices():
    """relu, residual, input read from / output written into a column slice of a wider buffer (how the bank chains through the concat)."""
    from unast_amd import ops
    B, T, C, k = 2, 37, 256, 6
    g = torch.Generator().manual_seed(5)
    wide = torch.randn(B, T, 4 * C, generator=g, dtype=torch.float64)
    W = torch.randn(C, C, k, generator=g, dtype=torch.float64) * 0.05
    b = torch.randn(C, generator=g, dtype=torch.float64)
    R = torch.randn(B, T, C, generator=g, dtype=torch.float64)
    ref = torch.relu(conv_ref(wide[..., C:2 * C], W, b, k)) + R
    buf = wide.float().to(dev())
    before = buf.clone()
    ops.conv_taps_fwd(buf[..., C:2 * C], W.permute(0, 2, 1).contiguous().float().to(dev()), b.float().to(dev()), buf[..., 2 * C:3 * C], k // 2,
                      act=1, R=R.float().to(dev()))
    assert relerr(buf[..., 2 * C:3 * C], ref) < GEMM_TOL
    keep = [0, 1, 3]
    assert all(torch.equal(buf[..., i * C:(i + 1) * C], before[..., i * C:(i + 1) * C]) for i in keep)


@pytest.mark.parametrize("B,T,Cin,Cout,pad", [(3, 37, 256, 256, 2), (2, 50, 80, 256, 4)])
def test_conv_five_taps_is_bit_identical_to_conv_fwd(B, T, Cin, Cout, pad):
    from unast_amd import ops
    g = torch.Generator().manual_seed(B * 100 + T)
    x = torch.randn(B, T, Cin, generator=g).to(dev())
    Wp = (torch.randn(Cout, 5, Cin, generator=g) * 0.05).to(dev())
    b = torch.randn(Cout, generator=g).to(dev())
    y0, y1 = torch.empty(B, T, Cout, device=dev()), torch.empty(B, T, Cout, device=dev())
    ops.conv_fwd(x, Wp, b, y0, pad)
    ops.conv_taps_fwd(x, Wp, b, y1, pad)
    assert torch.equal(y0, y1)


def gru_case(B, T, seed):
    """One bidirectional layer through ops.gru_fwd against fp64 torch.nn.GRU with the same weights; the input projections are formed in
    fp64 on the host (as the LSTM test does), so that the figure is the recurrence kernel's.  Returns (kernel error, error of fp32
    torch.nn.GRU on the CPU), both relative to max |fp64 output|."""
    from unast_amd import ops
    H = 128
    torch.manual_seed(seed)
    gru = torch.nn.GRU(256, H, num_layers=1, bidirectional=True, batch_first=True).double()
    x = torch.randn(B, T, 256, dtype=torch.float64)
    with torch.no_grad():
        ref, _ = gru(x)
        gru32 = torch.nn.GRU(256, H, num_layers=1, bidirectional=True, batch_first=True)
        gru32.load_state_dict({k: v.float() for k, v in gru.state_dict().items()})
        out32, _ = gru32(x.float())
        xp, whh, bhn = [], [], []
        for sfx in ("_l0", "_l0_reverse"):
            w_ih, w_hh = getattr(gru, "weight_ih" + sfx), getattr(gru, "weight_hh" + sfx)
            b_ih, b_hh = getattr(gru, "bias_ih" + sfx), getattr(gru, "bias_hh" + sfx)
            bx = b_ih.clone()
            bx[:2 * H] += b_hh[:2 * H]
            xp.append(x @ w_ih.t() + bx)
            whh.append(w_hh)
            bhn.append(b_hh[2 * H:])
    xproj = torch.cat(xp, dim=2).float().to(dev()).contiguous()
    y = torch.empty(B, T, 2 * H, device=dev())
    ops.gru_fwd(xproj, torch.stack(whh).float().to(dev()).contiguous(), torch.stack(bhn).float().to(dev()).contiguous(), y)
    return relerr(y, ref), relerr(out32, ref)


@pytest.mark.parametrize("B,T", [(5, 23), (1, 1)])
def test_gru_matches_fp64_torch_short(B, T):
    e, e32 = gru_case(B, T, seed=6)
    print("gru (%d,%d): kernel %.2e, fp32 torch on the CPU %.2e" % (B, T, e, e32))
    assert e < GRU_TOL


def test_gru_matches_fp64_torch_long():
    """800 steps: the bound is 4x what fp32 torch.nn.GRU on the CPU loses against fp64 on the same inputs (the kernel's sigmoid / tanh use the
    hardware exp2 and reciprocal instead of libm)."""
    e, e32 = gru_case(4, 800, seed=7)
    print("gru (4,800): kernel %.2e, fp32 torch on the CPU %.2e, bound %.2e" % (e, e32, 4 * e32))
    assert e < 4 * e32


def test_full_size_against_fp64_mirror_and_make_mags():
    from unast_amd.network import make_mags
    B, T = 8, 800
    sd = portable_sd()
    model = make_model(sd)
    mel = np.random.Generator(np.random.PCG64(99)).random((B, T, 80), dtype=np.float32)
    lens = [800, 771, 640, 555, 432, 301, 123, 37]
    for b in range(1, B):
        mel[b, lens[b]:] = 0.0
    torch.set_num_threads(16)
    ref, _ = VM.forward(sd, mel)
    mel_d = torch.from_numpy(mel).to(dev())
    with torch.no_grad():
        mag = model(mel_d)
        e = relerr(mag, ref)
        print("full size (8,800): %.2e of max |ref| = %.3f" % (e, ref.abs().max().item()))
        assert e < BAR
        # eval mode has no cross-batch coupling: row b of the batch is the same sequence run alone
        for b in (0, 3, 7):
            alone = model(mel_d[b:b + 1])
            eb = relerr(mag[b:b + 1], alone.double().cpu())
            print("row %d alone: %.2e" % (b, eb), end="; ")
            assert eb < GEMM_TOL
    mags = make_mags(model, mel_d, torch.tensor(lens))
    assert len(mags) == B
    for b in range(B):
        assert tuple(mags[b].shape) == (lens[b], 1025)
        assert torch.equal(mags[b], mag[b, :lens[b]])


def test_state_dict_round_trip_is_bit_equal():
    from unast_amd.network import Vocoder
    model = make_model(portable_sd(77))
    mel = torch.rand(2, 50, 80, generator=torch.Generator().manual_seed(3)).to(dev())
    with torch.no_grad():
        a = model(mel).clone()
        other = Vocoder(80, 256, 2048).to(dev()).eval()
        other.load_state_dict(model.state_dict())
        b = other(mel)
        model.load_state_dict(model.state_dict())
        c = model(mel)
    assert torch.equal(a, b) and torch.equal(a, c)


def test_pack_follows_parameter_updates():
    """The folded / packed operands are refreshed when a parameter or a BatchNorm buffer is written (version counters)."""
    sd = portable_sd(5)
    model = make_model(sd)
    mel = torch.rand(1, 20, 80, generator=torch.Generator().manual_seed(4)).to(dev())
    with torch.no_grad():
        a = model(mel).clone()
        model.cbhg.batchnorm_list[3].running_var.mul_(2.0)
        b = model(mel).clone()
        model.cbhg.batchnorm_list[3].running_var.mul_(0.5)
        c = model(mel)
    assert not torch.equal(a, b) and torch.equal(a, c)
    sd2 = {k: v.clone() for k, v in sd.items()}
    sd2["cbhg.batchnorm_list.3.running_var"] = sd2["cbhg.batchnorm_list.3.running_var"] * 2.0
    ref, _ = VM.forward(sd2, mel.cpu().numpy())
    assert relerr(b, ref) < BAR
