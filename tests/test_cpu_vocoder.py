"""The CBHG vocoder's contract that needs no GPU: state_dict keys, shapes and order against the reference's (recorded in the fixtures by
tools/gen_golden_vocoder.py), the fp64 mirror of its semantics (tests/vocoder_mirror.py) against the reference's outputs and
intermediates, and the refusal of a train-mode forward."""
import json
import os

import numpy as np
import pytest
import torch

from tests import vocoder_mirror as VM

FIXTURES = ["vocoder_b2_t37", "vocoder_b3_t64"]
# The reference's own fp32 forward differs from its fp64 one by 8e-7 of max |y| on these weights; 1e-5 leaves an order of magnitude of
# margin and still catches any semantic slip (chaining, even-kernel trimming, pooling edge, GRU gate order are errors of order 1).
MIRROR_TOL = 1e-5


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def portable_sd(fx):
    from unast_amd.portable import portable_tensor
    shapes = json.loads(str(fx["shapes_json"]))
    return {k: portable_tensor(k, tuple(s), int(fx["meta"][2])) for k, s in zip(fx["keys"].tolist(), shapes)}


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_keys_shapes_and_order_equal_the_reference(golden_dir, name):
    from unast_amd.network import Vocoder
    fx = load(golden_dir, name)
    model = Vocoder(80, 256, 2048)
    sd = model.state_dict()
    keys, shapes = fx["keys"].tolist(), json.loads(str(fx["shapes_json"]))
    assert len(keys) == 162
    assert list(sd.keys()) == keys
    assert [list(v.shape) for v in sd.values()] == shapes
    assert sum(p.numel() for p in model.parameters()) == 13672449
    # the portable weights the fixture was made with are the ones this side builds (per-tensor fp64 sums), and they load
    psd = portable_sd(fx)
    sums = np.array([float(np.asarray(psd[k], np.float64).sum()) for k in keys])
    assert np.array_equal(sums, fx["checksums"])
    model.load_state_dict({k: torch.from_numpy(v) for k, v in psd.items()})
    back = model.state_dict()
    assert all(torch.equal(back[k], torch.from_numpy(psd[k])) for k in keys)


@pytest.mark.parametrize("name", FIXTURES)
def test_fp64_mirror_reproduces_the_reference(golden_dir, name):
    fx = load(golden_dir, name)
    mag, st = VM.forward(portable_sd(fx), fx["mel"])
    cols, pcols = torch.from_numpy(fx["cols"]), torch.from_numpy(fx["pooled_cols"])
    got = {"out": mag, "pre": st["pre"][..., cols], "bank1": st["bank"][..., 0:256][..., cols], "bank2": st["bank"][..., 256:512][..., cols],
           "bank16": st["bank"][..., 3840:4096][..., cols], "pooled": st["pooled"][..., pcols], "proj": st["proj"][..., cols],
           "highway": st["highway"][..., cols], "gru": st["gru"][..., cols]}
    worst = {}
    for k, v in got.items():
        ref = torch.from_numpy(fx[k]).double()
        assert v.shape == ref.shape, k
        worst[k] = ((v - ref).abs().max() / ref.abs().max()).item()
    print(name, {k: "%.2e" % e for k, e in worst.items()})
    assert max(worst.values()) < MIRROR_TOL, worst


def test_train_mode_forward_raises():
    from unast_amd.network import Vocoder
    model = Vocoder(80, 256, 2048)
    assert model.training
    with pytest.raises(NotImplementedError):
        model(torch.zeros(1, 4, 80))
    with pytest.raises(NotImplementedError):            # eval mode, but autograd on: there is no backward on this path
        model.eval()(torch.zeros(1, 4, 80))


def test_unsupported_constructor_arguments_raise():
    from unast_amd.network import Vocoder
    with pytest.raises(NotImplementedError):
        Vocoder(80, 128, 2048)
    with pytest.raises(NotImplementedError):
        Vocoder(82, 256, 2048)


def test_wrappers_refuse_bad_layouts_before_any_launch():
    """The ctypes wrappers hand raw pointers to kernels that trust the shapes: mismatches are refused on the host."""
    from unast_amd import ops
    x = torch.zeros(2, 5, 8)
    with pytest.raises(ValueError):
        ops.conv_taps_fwd(x, torch.zeros(4, 3, 12), None, torch.zeros(2, 5, 4), 1)              # Cin of the weights != Cin of x
    with pytest.raises(ValueError):
        ops.conv_taps_fwd(x, torch.zeros(4, 3, 8), torch.zeros(3), torch.zeros(2, 5, 4), 1)     # short bias
    with pytest.raises(ValueError):
        ops.conv_taps_fwd(x, torch.zeros(4, 3, 8), None, torch.zeros(2, 5, 4), 1, R=torch.zeros(2, 4, 4))
    with pytest.raises(ValueError):
        ops.maxpool_prev(x, torch.zeros(2, 5, 4))
    with pytest.raises(ValueError):
        ops.highway_combine(torch.zeros(10, 8), torch.zeros(10, 8), torch.zeros(10, 8))
    with pytest.raises(ValueError):
        ops.gru_fwd(torch.zeros(1, 2, 768), torch.zeros(2, 384, 64), torch.zeros(2, 128), torch.zeros(1, 2, 256))
