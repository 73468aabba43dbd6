#!/usr/bin/env python3
"""Golden vectors for one TRAINING step of the CBHG vocoder: runs the reference's own network.Vocoder(80, 256, 2048)
(src/network.py:627-655) in fp64 and train mode on the CPU with portable weights, forms the sum loss of src/train_vocoder.py:58-61, 91 and
calls loss.backward() (:94).  Writes tests/golden/vocoder_train_*.npz:

    mel, mag_sum                  the input, and the fp64 sum of the target: both are uniform in [0, 1) from a seeded numpy PCG64
                                  (tests/vocoder_train_mirror.py: inputs), the target is regenerated from the seed by the tests
    keys                          the 108 parameter names in model.parameters() order
    out, out_cols                 the prediction [B, T, 1025] at the fixed columns `out_cols` (the same for both losses)
    stat_keys, stats              the 36 running statistics after the forward, [36, 256]
    l1_loss, l2_loss              the loss
    l1_gnorm, l2_gnorm            the 108 per-parameter gradient norms
    l1_gsample, l2_gsample        a fixed strided sample of <= 256 elements of every gradient (flattened in the reference's shape),
    gsample_offsets, gsample_strides    concatenated: gradient i at [offsets[i], offsets[i+1]), elements 0, stride, 2 stride, ...

Build container only (imports the reference); fixtures are data only.  Usage: python tools/gen_golden_vocoder_train.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
from portable_init import portable_state_dict  # noqa: E402
from tests.vocoder_train_mirror import inputs  # noqa: E402

SEED = 1234
SAMPLE = 256


def sample_stride(numel):
    return max(1, -(-numel // SAMPLE))


def run(network, name, B, T, out_dir):
    mel, mag = inputs(B, T, SEED)
    out_cols = np.arange(0, 1025, 8)
    fx = {"mel": mel, "mag_sum": np.array(float(mag.astype(np.float64).sum())), "meta": np.array([B, T, SEED], np.int64), "out_cols": out_cols.astype(np.int64)}
    for lt in ("l1", "l2"):
        torch.manual_seed(0)
        model = network.Vocoder(80, 256, 2048)
        sd = portable_state_dict(model.state_dict(), seed=SEED)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        model = model.double().train()
        loss_fn = torch.nn.MSELoss(reduction='sum') if lt == "l2" else torch.nn.L1Loss(reduction='sum')
        out = model.forward(torch.from_numpy(mel).double())
        loss = loss_fn(out, torch.from_numpy(mag).double())
        loss.backward()
        named = list(model.named_parameters())
        assert len(named) == 108 and tuple(out.shape) == (B, T, 1025)
        strides = [sample_stride(p.numel()) for _, p in named]
        samples = [p.grad.reshape(-1)[::s].numpy() for (_, p), s in zip(named, strides)]
        assert all(len(s) <= SAMPLE for s in samples)
        fx[lt + "_loss"] = np.array(float(loss.detach()))
        fx[lt + "_gnorm"] = np.array([float(p.grad.norm()) for _, p in named])
        fx[lt + "_gsample"] = np.concatenate(samples)
        if lt == "l1":
            stat_keys = [k for k in model.state_dict() if "running_" in k]
            assert len(stat_keys) == 36
            fx.update(keys=np.array([n for n, _ in named]), out=out.detach()[:, :, torch.from_numpy(out_cols)].contiguous().numpy(),
                      stat_keys=np.array(stat_keys), stats=np.stack([model.state_dict()[k].numpy() for k in stat_keys]),
                      gsample_strides=np.array(strides, np.int64), gsample_offsets=np.cumsum([0] + [len(s) for s in samples]).astype(np.int64))
        print(name, lt, "loss %.6f" % float(loss), "max |bias grad in front of a BatchNorm| %.2e" %
              max(float(p.grad.abs().max()) for n, p in named if ("convbank" in n or "conv_projection" in n) and n.endswith("bias")))
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **fx)
    print(name, "->", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    module, network, utils, train = G.import_reference()
    out_dir = os.path.join(os.path.dirname(HERE), "tests", "golden")
    torch.set_num_threads(8)
    run(network, "vocoder_train_b2_t37", 2, 37, out_dir)
    run(network, "vocoder_train_b3_t64", 3, 64, out_dir)
