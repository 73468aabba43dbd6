"""unast_amd.contract on the GPU: the three-launch forms with a caller's `out` / `work` against their allocating selves (to the bit), and the
scheme's own accuracy against fp64 -- until now it was reached through whole-model fixtures only."""
import functools

import pytest
import torch

from tests.griffin_lim_mirror import K

pytestmark = pytest.mark.gpu

SENTINEL = -7.0                                             # negative: a ReLU that ran over the pad columns would show
LIN = (37, 80, 13, 16)                                      # rows, K, N, pitch of `out`: N odd, three pad columns, fewer rows than a tile
CONV = (2, 45, 256, 256)                                    # B, T (odd: 90 rows), Cin, Cout of tests/test_gpu_vocoder.py's tap sweep


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


def relerr(a, ref):
    return ((a.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def mixed(g, *shape):
    """float32 values of mixed magnitude (e^N(0, 1.5) around 1) with full mantissas: few are representable in bf16, or in two bf16 parts."""
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * torch.exp(1.5 * torch.randn(*shape, generator=g, dtype=torch.float64))).float()


@functools.lru_cache(maxsize=None)
def lin_case():
    M, Kd, N, _ = LIN
    g = torch.Generator().manual_seed(37)
    x, W, b = mixed(g, M, Kd), mixed(g, N, Kd) * 0.1, mixed(g, N)
    ref = x.double() @ W.double().t() + b.double()
    return x, W, b, ref, x @ W.t() + b


def conv_ref(x, W, b, taps, pad_left):
    """conv1d over [B,T,Cin] with tap-major W [Cout,taps,Cin], pad_left zeros in front, in x's dtype on the CPU."""
    xp = torch.nn.functional.pad(x.transpose(1, 2), (pad_left, taps - 1 - pad_left))
    return torch.nn.functional.conv1d(xp, W.permute(0, 2, 1).contiguous(), b).transpose(1, 2)


@functools.lru_cache(maxsize=None)
def conv_case(taps):
    B, T, Cin, Cout = CONV
    g = torch.Generator().manual_seed(100 + taps)
    x, W, b = mixed(g, B, T, Cin), mixed(g, Cout, taps, Cin) * 0.05, mixed(g, Cout)
    return x, W, b, conv_ref(x.double(), W.double(), b.double(), taps, taps // 2), conv_ref(x, W, b, taps, taps // 2)


@pytest.mark.parametrize("act", [0, 1])
def test_linear_rows_into_a_padded_out_with_work_equals_the_allocating_form(act):
    from unast_amd import contract
    M, Kd, N, ld = LIN
    x, W, b = (t.to(dev()) for t in lin_case()[:3])
    Wp = contract.resid(W)
    want = contract.linear_rows(x, Wp, b, act=act)
    assert tuple(want.shape) == (M, N) and want.is_contiguous()
    out = torch.full((M, ld), SENTINEL, device=dev())
    work = tuple(torch.full(s, SENTINEL, device=dev()) for s in ((M, Kd), (M, Kd), (M, ld), (M, ld)))
    got = contract.linear_rows(x, Wp, b, act=act, out=out, work=work)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (M, N)
    assert torch.equal(bits(got), bits(want))
    assert (out[:, N:] == SENTINEL).all() and all((t[:, N:] == SENTINEL).all() for t in work[2:])
    assert (want >= 0).all() if act else (want < 0).any()


@pytest.mark.parametrize("taps", [3])
def test_conv_with_out_and_work_equals_the_allocating_form_on_the_contiguous_copy(taps):
    from unast_amd import contract
    B, T, Cin, Cout = CONV
    x, W, b = (t.to(dev()) for t in conv_case(taps)[:3])
    Wp = contract.resid(W)
    want = contract.conv(x, Wp, b, taps // 2)
    wide = torch.full((B, T, 2 * Cin), SENTINEL, device=dev())
    wide[:, :, Cin // 2:Cin // 2 + Cin] = x
    for x3d in (wide[:, :, Cin // 2:Cin // 2 + Cin], x):    # a column slice, then the contiguous tensor itself
        out = torch.full((B, T, Cout), SENTINEL, device=dev())
        work = tuple(torch.full(s, SENTINEL, device=dev()) for s in ((B, T, Cin), (B, T, Cin), (B, T, Cout), (B, T, Cout)))
        got = contract.conv(x3d, Wp, b, taps // 2, out=out, work=work)
        assert got is out and torch.equal(bits(got), bits(want)), x3d.is_contiguous()


def test_three_launches_beat_one_and_stay_within_k_of_fp32():
    """Errors against fp64 on float32 inputs of mixed magnitude, relative to max |ref|: the three-launch form must not lose to the
    single-launch three-term contraction it exists to improve on, and must stay within K = 8 of float32 torch on the CPU.
    Measured (MI355X), error relative to max |ref|:
        linear_rows [37,80] x [13,80]:      three launches 1.49e-7, one launch 2.42e-6 (16 x), fp32 CPU 1.82e-7: three / fp32 = 0.82
        conv 5 taps [2,45,256] -> 256:      three launches 5.39e-7, one launch 4.30e-6 ( 8 x), fp32 CPU 1.16e-7: three / fp32 = 4.64"""
    from unast_amd import contract, ops
    M, Kd, N, _ = LIN
    x, W, b, ref, cpu32 = lin_case()
    xd, Wd, bd = x.to(dev()), W.to(dev()), b.to(dev())
    one = torch.empty(M, N, device=dev())
    ops.gemm(ops.OP_KC, ops.OP_KC, xd, Kd, Wd, Kd, one, N, M, N, Kd, bias=bd)
    e3, e1, e32 = relerr(contract.linear_rows(xd, contract.resid(Wd), bd), ref), relerr(one, ref), relerr(cpu32, ref)
    print("linear_rows [%d,%d]x[%d,%d]: three launches %.2e, one launch %.2e (x %.0f), fp32 cpu %.2e (three / fp32 = %.2f)"
          % (M, Kd, N, Kd, e3, e1, e1 / e3, e32, e3 / e32))
    assert e3 <= e1 and e3 <= K * e32
    taps = 5
    B, T, Cin, Cout = CONV
    x, W, b, ref, cpu32 = conv_case(taps)
    xd, Wd, bd = x.to(dev()), W.to(dev()), b.to(dev())
    one = torch.empty(B, T, Cout, device=dev())
    ops.conv_taps_fwd(xd, Wd, bd, one, taps // 2)
    c3, c1, c32 = relerr(contract.conv(xd, contract.resid(Wd), bd, taps // 2), ref), relerr(one, ref), relerr(cpu32, ref)
    print("conv %d taps [%d,%d,%d]->%d: three launches %.2e, one launch %.2e (x %.0f), fp32 cpu %.2e (three / fp32 = %.2f)"
          % (taps, B, T, Cin, Cout, c3, c1, c1 / c3, c32, c3 / c32))
    assert c3 <= c1 and c3 <= K * c32
