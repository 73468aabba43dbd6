#!/usr/bin/env python3
"""Golden vectors for the full train step with the discriminator at disc_hid=128: the reference's own step functions under its
src/configs/transformer_d_test.json (bidirectional 2-layer LSTM discriminator of width 128, t_eos_weight 3.0, linear schedule) with RNG
sites off and portable weights; writes tests/golden/step_b4_t24_m64_l2_dh128.npz (lr 1e-3) and ..._dh128_lr0.npz (lr 0) in the layout of gen_golden.py's step fixtures.
Build container only (imports /root/reference)."""
import json, os, sys
from types import SimpleNamespace
import torch
HERE = os.path.dirname(os.path.abspath(__file__)); sys.path.insert(0, HERE)
import gen_golden as G


def make_args(num_layers):
    cfg = json.load(open(os.path.join(G.REF_SRC, "configs", "transformer_d_test.json")))
    args = SimpleNamespace(**cfg)
    args.load_path = None
    args.num_layers = num_layers
    return args


if __name__ == "__main__":
    mods = G.import_reference()
    G.make_args = make_args                       # run_case builds its arguments through the module's make_args
    out_dir = os.path.join(os.path.dirname(HERE), "tests", "golden")
    torch.set_num_threads(8)
    # the ragged 2-layer case of gen_golden.py at this config; 1000 scheduler steps = the end of the linear warm-up (lr 1e-3)
    G.run_case(mods, "step_b4_t24_m64_l2_dh128", 4, 24, 64, 2, True, out_dir, lr_warm_steps=1000)
    # the same step at the schedule's first value, lr 0: the generator's AdamW step moves nothing, so the discriminator phase sees exactly
    # the parameters a second implementation has and its gradients compare element by element (gen_golden.py's *_lr0 case)
    G.run_case(mods, "step_b4_t24_m64_l2_dh128_lr0", 4, 24, 64, 2, True, out_dir, lr_warm_steps=0)
