#!/usr/bin/env python3
"""Where the gradient error of the vocoder's training step comes from: the fp64 mirror of one step
(tests/vocoder_train_mirror.py) with the split-bf16 rounding of the MFMA GEMM's operands (hi = RNE_bf16(x), lo = RNE_bf16(x - hi),
a_hi b_hi + a_hi b_lo + a_lo b_hi) emulated in the 18 convolutions -- in their forward products only, in their
backward products only, or in both -- against the clean fp64 mirror under the same gates.  Prints the four worst per-tensor gradient
errors (relative norm) and the output error of each variant.  CPU only; reads a fixture of tests/golden/.
Usage: python tools/vocoder_train_emu.py [--fixture vocoder_train_b2_t37] [--loss l1]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import vocoder_train_mirror as TM  # noqa: E402
from unast_amd.network import Vocoder  # noqa: E402
from unast_amd.portable import portable_tensor  # noqa: E402

MODE = {"fwd": False, "bwd": False}


def split(x):
    hi = x.float().bfloat16().double()
    return hi, (x - hi).float().bfloat16().double()


def mm3(a, b):
    ah, al = split(a)
    bh, bl = split(b)
    return ah @ bh + ah @ bl + al @ bh


class SplitMatmul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return mm3(a, b) if MODE["fwd"] else a @ b

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        if MODE["bwd"]:
            return mm3(g, b.t()), mm3(a.t(), g)
        return g @ b.t(), a.t() @ g


def conv(x, W, b):
    """TM.conv as an explicit contraction over (tap, channel): what the implicit GEMM multiplies."""
    B, T, Cin = x.shape
    k = W.shape[2]
    xp = F.pad(x, (0, 0, k // 2, k - 1 - k // 2))
    cols = torch.cat([xp[:, j:j + T] for j in range(k)], dim=2).reshape(B * T, k * Cin)
    return (SplitMatmul.apply(cols, W.permute(0, 2, 1).reshape(W.shape[0], k * Cin).t()) + b).view(B, T, -1)


def normerr(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixture", default="vocoder_train_b2_t37")
    ap.add_argument("--loss", default="l1", choices=["l1", "l2"])
    a = ap.parse_args()
    fx = np.load(os.path.join(ROOT, "tests", "golden", a.fixture + ".npz"))
    mel, mag = TM.fixture_inputs(fx)
    sd = {k: torch.from_numpy(portable_tensor(k, tuple(v.shape), int(fx["meta"][2]))) for k, v in Vocoder(80, 256, 2048).state_dict().items()}
    gates = TM.step(sd, mel, mag, a.loss, need_grads=False)["gates"]
    clean = TM.step(sd, mel, mag, a.loss, gates=gates)
    r32 = TM.step(sd, mel, mag, a.loss, dtype=torch.float32, gates=gates)
    names = [n for n in clean["grads"] if n not in TM.DEGENERATE]
    print("fp32 mirror under the same gates: worst %.2e" % max(normerr(r32["grads"][n], clean["grads"][n]) for n in names))
    TM.conv = conv
    for fwd, bwd in ((True, False), (False, True), (True, True)):
        MODE["fwd"], MODE["bwd"] = fwd, bwd
        r = TM.step(sd, mel, mag, a.loss, gates=gates)
        errs = {n: normerr(r["grads"][n], clean["grads"][n]) for n in names}
        worst = sorted(errs, key=errs.get)[-4:][::-1]
        print("split-bf16 products in the convolutions' %s: out %.2e; worst gradients %s"
              % ("forward and backward" if fwd and bwd else "forward" if fwd else "backward",
                 ((r["out"] - clean["out"]).abs().max() / clean["out"].abs().max()).item(), ", ".join("%s %.2e" % (n, errs[n]) for n in worst)))


if __name__ == "__main__":
    main()
