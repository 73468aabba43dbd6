"""The attention kernels (csrc/attention.hip) at the ragged-length edges against fp64, per sequence: key sets of one or a few keys, lengths
on and next to the 32-key chunk, 64-key tile and 128-key block edges, blocks entirely past the length, causal queries far past the length,
lens_k > Tk, lens_q independent of lens_k.  Cases, references and the metric are in tests/ragged_ref.py; tests/test_cpu_ragged_ref.py
shows that the metric at these tolerances sees a length that is off by one.

Every case runs both forward kernels, fp32 and pre-split operands, the one-pass and the two-kernel backward, into NaN-filled outputs."""
import pytest
import torch

from tests import ragged_ref as R

pytestmark = pytest.mark.gpu
D = torch.device("cuda:0")


def relerr(a, b):
    b = b.double().cpu()
    return ((a.double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@pytest.fixture
def fwd_variant_restore():
    from unast_amd._lib import lib
    old = lib().unast_attn_fwd_variant(-1)
    yield lib().unast_attn_fwd_variant
    lib().unast_attn_fwd_variant(old)


def nan(*shape):
    return torch.full(shape, float("nan"), device=D)


@pytest.mark.parametrize("variant", list(R.VARIANTS))
def test_ragged_attention_against_fp64(variant, monkeypatch, fwd_variant_restore):
    """Every figure is printed before it is judged (pytest -s): the per-sequence errors of every path and the whole-tensor differences
    between the forms, so that a kernel rewrite sees its headroom."""
    from unast_amd import config, ops
    epoch = int(ops.rng_epoch_counter().item())          # mixed into every mask; 0 unless an earlier test left it advanced
    x, ref, factor = R.inputs(variant), R.reference_cached(variant, epoch), R.drop_factor(variant, epoch)
    B, Tq, Tk, causal, nsplit, p = x["B"], x["Tq"], x["Tk"], x["causal"], x["nsplit"], x["p"]
    H, E = R.H, R.E
    fl = R.floors(x)
    klen = x["lens_k"].clamp(0, Tk)
    dead = (torch.arange(Tk)[None, :] >= klen[:, None])[..., None].expand(B, Tk, E)
    lens_d = x["lens_k"].to(torch.int32).to(D)
    lens_q = x["lens_q"]
    lens_q_d = lens_q.to(torch.int32).to(D) if lens_q is not None else None
    drop = dict(drop_p=p, seed=R.SEED, stream_id=R.STREAM)
    monkeypatch.setattr(config, "DETERMINISTIC_SUMS", False)
    monkeypatch.setattr(config, "ATTN_BWD_TERMS", 3)

    f32 = [x[n].float().to(D).reshape(-1, E).contiguous() for n in ("q", "k", "v", "do")]
    split = [torch.empty_like(t) for t in f32]
    for src, dst in zip(f32, split):
        ops.split_f32(src.view(-1), dst.view(-1))

    # The two forms of the backward and the two operand formats against each other: the bounds of test_attention_backward_one_pass_equals_
    # two_kernels and test_attention_on_presplit_operands.  (Every kernel splits an fp32 operand as unast_split_f32 does, so they hold at
    # nsplit = 1 as well: the same bf16 values enter the products of every form.)
    agree_dq, agree_split = 2e-5, 3e-5
    fails, lines = [], []

    def check(got, presplit, where):
        """finite everywhere, dead keys exactly zero, fp64 parity per sequence; returns the worst per-sequence error"""
        worst = 0.0
        for n, t in got.items():
            t = t.cpu()
            assert bool(torch.isfinite(t).all()), (variant, where, n, "not written / not finite")
            if n in ("dK", "dV"):
                assert bool((t.view(B, Tk, E)[dead] == 0).all()), (variant, where, n, "nonzero gradient at a key past the length")
            if n == "dQ" and lens_q is not None:
                pad = (torch.arange(Tq)[None, :] >= lens_q[:, None])[..., None].expand(B, Tq, E)
                assert bool((t.view(B, Tq, E)[pad] == 0).all()), (variant, where, "dQ nonzero at a query past lens_q")
            err = R.seq_err(t.view(ref[n].shape), ref[n], fl[n])
            tol = R.tolerance(nsplit, presplit)
            lines.append("  %-28s %-3s per sequence %s" % (where, n, " ".join("%.1e" % e for e in err.tolist())))
            if not bool((err < tol).all()):
                fails.append((where, n, err.tolist(), tol))
            worst = max(worst, float(err.max()))
        if lens_q is not None and "dQ" in got:
            for b in range(B):
                if int(lens_q[b]) == 0:          # no tile of this sequence is visited
                    assert all(bool((got[n].view(B, -1)[b] == 0).all()) for n in ("dQ", "dK", "dV")), (variant, where, b)
        return worst

    def whole(a, b, bound, what):
        """the suite's whole-tensor relerr of a against b, with the per-sequence differences for the log"""
        e = relerr(a, b)
        per = (a.double() - b.double()).abs().view(B, -1).amax(1).cpu()
        lines.append("  %-32s whole-tensor %.2e (bound %.0e); max |diff| per sequence %s over max |.| %.2e" % (
            what, e, bound, " ".join("%.1e" % v for v in per.tolist()), float(b.abs().max())))
        if not e < bound:
            fails.append((what, e, bound))

    modes = [("one-pass", True)] if lens_q is not None else [("two-kernel", False), ("one-pass", True)]
    res, worst = {}, {False: 0.0, True: 0.0}
    for presplit in (False, True):
        Q_, K_, V_, dO_ = split if presplit else f32
        for fv in (0, 1):
            fwd_variant_restore(fv)
            O, LSE = nan(B * Tq, E), nan(B, H, Tq)
            ops.attn_fwd(Q_, K_, V_, O, LSE, lens_d, B, H, Tq, Tk, causal, nsplit=nsplit, qkv_split=presplit, **drop)
            res[presplit, "fwd", fv] = {"O": O, "LSE": LSE}
            if factor is not None:          # one visible key: the row is V / (1 - p) (parity below) or, the key dropped, exactly 0
                for b in (klen == 1).nonzero().flatten().tolist():
                    gone = factor[b, :, :, 0] == 0
                    assert bool(gone.any()) and bool((O.view(B, Tq, H, 64)[b].transpose(0, 1).cpu()[gone] == 0).all()), (variant, fv, b)
            worst[presplit] = max(worst[presplit], check(res[presplit, "fwd", fv], presplit, (presplit, "fwd", fv)))
        for name, fused in modes:          # on the default forward kernel's O and LSE
            monkeypatch.setattr(config, "ATTN_FUSED_BWD", fused)
            dQ, dK, dV, ws = nan(B * Tq, E), nan(B * Tk, E), nan(B * Tk, E), nan(B, H, Tq)
            ops.attn_bwd(Q_, K_, V_, O, dO_, LSE, ws, dQ, dK, dV, lens_d, B, H, Tq, Tk, causal, nsplit=nsplit, qkv_split=presplit,
                         lens_q=lens_q_d, **drop)
            res[presplit, name] = {"dQ": dQ, "dK": dK, "dV": dV}
            worst[presplit] = max(worst[presplit], check(res[presplit, name], presplit, (presplit, name)))
        if len(modes) == 2:          # test_attention_backward_one_pass_equals_two_kernels, at short lengths
            a, b = res[presplit, "two-kernel"], res[presplit, "one-pass"]
            assert torch.equal(a["dK"], b["dK"]) and torch.equal(a["dV"], b["dV"]), (variant, presplit)
            whole(b["dQ"], a["dQ"], agree_dq, "one-pass vs two-kernel dQ%s" % (" (pre-split)" if presplit else ""))
    # test_attention_on_presplit_operands, at short lengths: the same hi / lo values enter the MFMAs
    for key in [k[1:] for k in res if k[0]]:
        for n, t in res[(True,) + key].items():
            whole(t, res[(False,) + key][n], agree_split, "pre-split vs fp32 %s %s" % (" ".join(map(str, key)), n))
    print("ragged %-10s worst per-sequence error: fp32 operands %.1e (bound %.0e), pre-split %.1e (bound %.0e)" % (
        variant, worst[False], R.tolerance(nsplit, False), worst[True], R.tolerance(nsplit, True)))
    print("\n".join(lines))
    assert not fails, fails
