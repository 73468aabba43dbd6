"""Host-side checks of the vocoder's training step (unast_amd.train_vocoder): the fp64 mirror of one step (tests/vocoder_train_mirror.py)
against the reference's own fp64 train-mode run (tests/golden/vocoder_train_*.npz, written by tools/gen_golden_vocoder_train.py), and
the refusals that happen before any kernel is launched.  No GPU needed.
"""
import os

import numpy as np
import pytest
import torch

from tests import vocoder_train_mirror as TM

FIXTURES = ["vocoder_train_b2_t37", "vocoder_train_b3_t64"]
TOL = 1e-9            # fp64 against fp64: two orders of summation


def portable_sd(seed):
    from unast_amd.network import Vocoder
    from unast_amd.portable import portable_tensor
    return {k: torch.from_numpy(portable_tensor(k, tuple(v.shape), seed)) for k, v in Vocoder(80, 256, 2048).state_dict().items()}


@pytest.mark.parametrize("loss_type", ["l1", "l2"])
@pytest.mark.parametrize("name", FIXTURES)
def test_mirror_matches_reference_step(golden_dir, name, loss_type):
    fx = np.load(os.path.join(golden_dir, name + ".npz"))
    torch.set_num_threads(min(8, torch.get_num_threads()))
    mel, mag = TM.fixture_inputs(fx)
    r = TM.step(portable_sd(int(fx["meta"][2])), mel, mag, loss_type)
    keys = [str(k) for k in fx["keys"]]
    assert keys == list(r["grads"].keys()) and len(keys) == 108
    worst = {}
    worst["loss"] = abs(r["loss"] - float(fx[loss_type + "_loss"])) / abs(float(fx[loss_type + "_loss"]))
    ref_out = torch.from_numpy(fx["out"])
    worst["out"] = ((r["out"][:, :, torch.from_numpy(fx["out_cols"])] - ref_out).abs().max() / ref_out.abs().max()).item()
    stats = torch.stack([r["stats"][str(k)] for k in fx["stat_keys"]])
    worst["stats"] = ((stats - torch.from_numpy(fx["stats"])).abs().max() / torch.from_numpy(fx["stats"]).abs().max()).item()
    off, strides = fx["gsample_offsets"], fx["gsample_strides"]
    gnorm, gsample = fx[loss_type + "_gnorm"], torch.from_numpy(fx[loss_type + "_gsample"])
    worst["grad"], worst["gnorm"], worst["degenerate"] = 0.0, 0.0, 0.0
    for i, k in enumerate(keys):
        g = r["grads"][k]
        if k in TM.DEGENERATE:                              # mathematically zero: rounding noise on both sides, absolute terms
            worst["degenerate"] = max(worst["degenerate"], g.abs().max().item())
            continue
        ref = gsample[off[i]:off[i + 1]]
        got = g.reshape(-1)[::int(strides[i])]
        worst["grad"] = max(worst["grad"], ((got - ref).abs().max() / gnorm[i]).item())
        worst["gnorm"] = max(worst["gnorm"], abs(g.norm().item() - gnorm[i]) / gnorm[i])
    print(name, loss_type, {k: "%.2e" % e for k, e in worst.items()})
    assert max(worst.values()) < TOL, worst


def test_vocoder_step_refuses_eval_mode_and_bad_batches():
    from unast_amd import train_vocoder as TV
    from unast_amd.network import Vocoder
    model = Vocoder(80, 256, 2048)
    mel, mag = torch.zeros(1, 4, 80), torch.zeros(1, 4, 1025)
    with pytest.raises(RuntimeError):
        TV.vocoder_step(model.eval(), mel, mag)
    model.train()
    for bad_mel, bad_mag in ((torch.zeros(1, 4, 81), mag), (mel, torch.zeros(1, 4, 1024)), (mel, torch.zeros(1, 5, 1025)),
                             (mel.double(), mag), (mel, mag.double()), (mel[0], mag[0]), (mel, mag)):          # (the last: not on the GPU)
        with pytest.raises(ValueError):
            TV.vocoder_step(model, bad_mel, bad_mag)
        with pytest.raises(ValueError):
            TV.valid_loss(model, bad_mel, bad_mag)
    with pytest.raises(TypeError):
        TV.vocoder_step(torch.nn.Linear(2, 2), mel, mag)
    assert all(p.grad is None for p in model.parameters())


def test_vocoder_forward_still_raises_in_train_mode():
    from unast_amd.network import Vocoder
    model = Vocoder(80, 256, 2048)
    with pytest.raises(NotImplementedError, match="vocoder_step"):
        model(torch.zeros(1, 4, 80))
    with pytest.raises(NotImplementedError):
        model.eval()(torch.zeros(1, 4, 80))


def test_new_names_are_exported_next_to_make_mags():
    from unast_amd import network, train_vocoder
    assert network.vocoder_step is train_vocoder.vocoder_step and network.valid_loss is train_vocoder.valid_loss
    assert network.FlatAdamW is train_vocoder.FlatAdamW and network.vocoder_train_step is train_vocoder.train_step


def test_training_wrappers_refuse_bad_layouts_before_any_launch():
    from unast_amd import ops
    z = torch.zeros
    with pytest.raises(ValueError):
        ops.gru_fwd_train(z(1, 2, 768), z(2, 384, 128), z(2, 128), z(1, 2, 256), z(1, 2, 2, 384))          # saved holds four values per unit
    with pytest.raises(ValueError):
        ops.gru_bwd(z(1, 2, 256), z(1, 2, 256), z(1, 2, 2, 512), z(2, 384, 128), z(1, 2, 2, 384), z(1, 2, 2, 64))
    with pytest.raises(ValueError):
        ops.gru_bwd(z(1, 3, 256), z(1, 2, 256), z(1, 2, 2, 512), z(2, 384, 128), z(1, 2, 2, 384), z(1, 2, 2, 128))
    with pytest.raises(ValueError):
        ops.maxpool_prev_bwd(z(2, 5, 8), z(2, 5, 8), z(2, 5, 4))
    with pytest.raises(ValueError):
        ops.maxpool_prev_bwd(z(2, 5, 8), z(2, 5, 8).transpose(0, 1), z(2, 5, 8))
    with pytest.raises(ValueError):
        ops.relu_bwd(z(10, 8), z(10, 4))
    with pytest.raises(ValueError):
        ops.highway_combine_bwd(z(10, 8), z(10, 8), z(10, 8), z(10, 16), z(10, 8))                           # ht must be [rows, 2C]
    with pytest.raises(ValueError):
        ops.sum_loss(z(3, 9), z(3, 8), None, False, z((), dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.sum_loss(z(3, 8), z(3, 8), None, False, z(()))                                                   # fp32 accumulator
    with pytest.raises(ValueError):
        ops.split_parts(z(8), hi=z(4))
    with pytest.raises(ValueError):
        ops.split_parts(z(8))
    with pytest.raises(ValueError):
        ops.conv_taps_dgrad(z(2, 5, 8), z(8, 3, 12), z(2, 5, 8), 1)                                          # Cin of the weights != Cin of dx
    with pytest.raises(ValueError):
        ops.conv_taps_dgrad(z(2, 5, 8), z(8, 17, 8), z(2, 5, 8), 1)                                          # 17 taps
    with pytest.raises(ValueError):
        ops.conv_taps_dgrad(z(2, 5, 8), z(8, 3, 8), z(2, 5, 8), 3)                                           # pad_left outside the kernel
    with pytest.raises(ValueError):
        ops.conv_taps_wgrad(z(2, 5, 8), z(2, 5, 8), z(8, 3, 4), 1)
    with pytest.raises(ValueError):
        ops.conv_taps_wgrad(z(2, 5, 8), z(2, 5, 8), z(8, 3, 8), 1, db=z(4))
    with pytest.raises(TypeError):
        ops.conv_taps_wgrad(z(2, 5, 8), z(2, 5, 8), z(8, 3, 8), 1)                                           # right layout, not on the GPU
