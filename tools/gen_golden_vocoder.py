#!/usr/bin/env python3
"""Golden vectors for the CBHG vocoder's eval forward: runs the reference's own network.Vocoder(80, 256, 2048)
(src/network.py:627-655) in eval mode on the CPU with portable weights and writes tests/golden/vocoder_*.npz:

    mel                          the input, uniform in [0, 1) (seeded numpy PCG64)
    keys, shapes_json, checksums the state_dict contract: names in order, shapes, per-tensor fp64 sums of the portable weights
    out                          the magnitude spectrogram [B, T, 1025]
    pre, bank1, bank2, bank16,   intermediates that locate a fault, token-major [B, T, C], taken by hooks on the reference's own
    proj, highway, gru           modules, at the columns `cols` of their 256 (all of them in the small fixture, a fixed sample in the
                                 large one: the output alone is 0.8 MB there)
    pooled, pooled_cols          the max-pooled concat [B, T, 4096] at the fixed columns `pooled_cols` (every bank stage is hit)

Build container only (imports the reference); fixtures are data only.  Usage: python tools/gen_golden_vocoder.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
from portable_init import portable_state_dict  # noqa: E402

SEED = 1234


def run(network, name, B, T, pad_tail, n_cols, n_pooled, out_dir):
    torch.manual_seed(0)
    model = network.Vocoder(80, 256, 2048)
    template = model.state_dict()
    sd = portable_state_dict(template, seed=SEED)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.eval()
    mel = np.random.Generator(np.random.PCG64([SEED, B, T])).random((B, T, 80), dtype=np.float32)
    for b, n in pad_tail.items():
        mel[b, T - n:] = 0.0                                # stands for padding: the vocoder runs over it all the same
    cols = np.arange(256) if n_cols == 256 else (np.arange(n_cols) * (256 // n_cols) + (np.arange(n_cols) * 5) % (256 // n_cols))
    pooled_cols = np.arange(n_pooled) * (4096 // n_pooled) + (np.arange(n_pooled) * 7) % (4096 // n_pooled)
    got = {}
    c = model.cbhg
    tm = lambda x: x.detach().transpose(1, 2)               # [B, C, T] -> token-major
    hooks = [model.pre_projection.register_forward_hook(lambda m, i, o: got.__setitem__("pre", tm(o))),
             c.max_pool.register_forward_hook(lambda m, i, o: got.__setitem__("pooled", tm(o[:, :, :-1]))),
             # (the reference calls highway.forward / fc.forward directly, which bypasses hooks: the highway's input is taken where its
             # first nn.Linear is called, its output where the GRU is)
             c.highway.linears[0].linear_layer.register_forward_pre_hook(lambda m, i: got.__setitem__("proj", i[0].detach())),
             c.gru.register_forward_hook(lambda m, i, o: got.update(highway=i[0].detach(), gru=o[0].detach()))]
    for k in (1, 2, 16):
        hooks.append(c.batchnorm_list[k - 1].register_forward_hook(lambda m, i, o, k=k: got.__setitem__("bank%d" % k, tm(torch.relu(o)))))
    with torch.no_grad():
        out = model(torch.from_numpy(mel))
    for h in hooks:
        h.remove()
    assert tuple(out.shape) == (B, T, 1025) and len(template) == 162
    fx = {"mel": mel, "meta": np.array([B, T, SEED], np.int64), "keys": np.array(list(template.keys())),
          "shapes_json": np.array(json.dumps([list(v.shape) for v in template.values()])),
          "checksums": np.array([float(np.asarray(sd[k], np.float64).sum()) for k in template]),
          "out": out.numpy(), "cols": cols.astype(np.int64), "pooled_cols": pooled_cols.astype(np.int64),
          "pooled": got["pooled"][:, :, torch.from_numpy(pooled_cols)].contiguous().numpy()}
    for k in ("pre", "bank1", "bank2", "bank16", "proj", "highway", "gru"):
        assert tuple(got[k].shape) == (B, T, 256), (k, got[k].shape)
        fx[k] = got[k][:, :, torch.from_numpy(cols)].contiguous().numpy()
    path = os.path.join(out_dir, name + ".npz")
    np.savez_compressed(path, **fx)
    print(name, "max|y| %.4f mean|y| %.4f" % (float(out.abs().max()), float(out.abs().mean())), "params",
          sum(p.numel() for p in model.parameters()), "->", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    module, network, utils, train = G.import_reference()
    out_dir = os.path.join(os.path.dirname(HERE), "tests", "golden")
    torch.set_num_threads(8)
    run(network, "vocoder_b2_t37", 2, 37, {1: 9}, 256, 64, out_dir)
    run(network, "vocoder_b3_t64", 3, 64, {}, 16, 32, out_dir)
