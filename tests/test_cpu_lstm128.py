"""The discriminator at disc_hid=128 (the reference's src/configs/transformer_d_test.json), host side: construction through
train.initialize_model, the parameter contract against the reference-generated fixture, and the widths that stay refused."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "step_b4_t24_m64_l2_dh128.npz")


def _model(L=2):
    from unast_amd import train
    from unast_amd.configs import make_args
    args = make_args(num_layers=L, disc_hid=128, t_eos_weight=3.0, ae_steps=1, sp_steps=1, d_steps=1, cm_steps=0)
    train.DEVICE = torch.device("cpu")
    return train.initialize_model(args)[2]


def test_initialize_model_builds_the_128_wide_discriminator_with_the_reference_names():
    model = _model()
    g = np.load(FIXTURE)
    assert [n for n, _ in model.named_parameters()] == [str(n) for n in g["param_names"]]
    assert model.discriminator.hidden == 128 and model.discriminator.num_dir == 2 and model.discriminator.num_layers == 2


def test_discriminator_tensors_have_the_shapes_of_torch_lstm_256_128():
    from unast_amd.spec import state_dict_spec
    model = _model()
    sd = model.state_dict()
    ref = torch.nn.LSTM(256, 128, num_layers=2, bidirectional=True, batch_first=True)
    want = {"discriminator.rnn.rnn." + k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert len(want) == 16 and want["discriminator.rnn.rnn.weight_ih_l1_reverse"] == (512, 256)
    want.update({"discriminator.rnn.reduce_h_W.weight": (128, 256), "discriminator.rnn.reduce_h_W.bias": (128,),
                 "discriminator.rnn.reduce_c_W.weight": (128, 256), "discriminator.rnn.reduce_c_W.bias": (128,),
                 "discriminator.fc2.weight": (1, 128), "discriminator.fc2.bias": (1,)})
    got = {k: tuple(v.shape) for k, v in sd.items() if k.startswith("discriminator.")}
    assert got == want
    spec = state_dict_spec(2, disc_hid=128)
    assert list(sd.keys()) == list(spec.keys()) and all(tuple(sd[k].shape) == tuple(spec[k]) for k in spec)


def test_other_widths_and_output_sizes_are_still_refused():
    from unast_amd.network import LSTMDiscriminator
    with pytest.raises(NotImplementedError, match="64.*128"):
        LSTMDiscriminator(256, 96, bidirectional=True, num_layers=2)
    with pytest.raises(NotImplementedError, match="64.*128"):
        LSTMDiscriminator(256, 128, out=2, bidirectional=True, num_layers=2)
    with pytest.raises(NotImplementedError):
        LSTMDiscriminator(256, 64, out=2)
    assert LSTMDiscriminator(256, 64, bidirectional=True, num_layers=2).hidden == 64


def test_ops_refuse_operands_of_two_widths():
    """ops.lstm_fwd / lstm_bwd take the width from W_hh and cross-check it against the saved-state operand before any launch."""
    from unast_amd import ops
    whh = torch.zeros(2 * 512, 128)
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(ValueError, match="lstm_fwd"):
        ops.lstm_fwd(z(1, 2, 1024), whh, z(1024), z(1024), z(1).int(), z(1, 2, 256), z(1, 2, 2, 512), z(1, 2, 2, 64), z(1, 2, 2, 128), z(1, 256),
                     2, 512 * 128, 512)
    with pytest.raises(ValueError, match="lstm_bwd"):
        ops.lstm_bwd(None, z(1, 256), whh, z(1, 2, 2, 256), z(1, 2, 2, 128), z(1).int(), z(1, 2, 2, 512), 2, 512 * 128)
