"""Weights of the RNN model fixtures (tests/golden/rnn_*.npz), rebuilt from names: unast_amd.portable's seeded values plus the gains a fixture
records in its meta.  The fixtures store key names, shapes, seed and gains only (about 6 M parameters per model would not fit)."""
import json

import numpy as np
import torch

from unast_amd.portable import portable_tensor

PREFIX = {"text": "text_m.", "speech": "speech_m."}


def state_dict(side, keys, shapes, seed=1234, gains=()):
    """name -> float32 torch tensor for one model.  `gains`: list of [suffix-or-substring, op, value] applied in order to every key that
    contains the pattern; op 'scale' multiplies, 'fill' sets, 'eos' adds to element 2 (the EOS logit's bias)."""
    sd = {}
    for k, shp in zip(keys, shapes):
        v = portable_tensor(PREFIX[side] + k, tuple(shp), seed)
        for pat, op, val in gains:
            if pat in PREFIX[side] + k and v.dtype == np.float32:
                if op == "eos":                                        # a bias on the EOS logit (index 2) only
                    v = v.copy()
                    v[2] += np.float32(val)
                else:
                    v = (v * np.float32(val)) if op == "scale" else np.full_like(v, val)
        sd[k] = torch.from_numpy(np.ascontiguousarray(v))
    return sd


def meta_of(npz):
    return json.loads(str(npz["meta"]))


def fixture_state_dicts(npz):
    """(text state_dict, speech state_dict) of a fixture."""
    m = meta_of(npz)
    return tuple(state_dict(side, m[side + "_keys"], m[side + "_shapes"], m["seed"], m["gains"]) for side in ("text", "speech"))


def rnn_args(attn, attn_dim=32, hidden=256, num_layers=2, e_bi=True, num_mels=80):
    """The hyper-parameters of the reference's full-size RNN configs (src/configs/rnn_d_lsa.json, rnn_d_luong.json)."""
    from types import SimpleNamespace
    return SimpleNamespace(num_mels=num_mels, s_pre_hid=hidden, s_pre_drop=0.5, s_post_drop=0.1, t_emb_dim=hidden, t_pre_drop=0.5, t_post_drop=0.1,
                           hidden=hidden, e_in=hidden, e_drop=0.5, num_layers=num_layers, e_bi=e_bi, d_drop=0.3, d_attn=attn, attn_dim=attn_dim)
