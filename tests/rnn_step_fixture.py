"""What the CPU and the GPU tests of unast_amd.train_rnn_step share: reading tests/golden/rnn_step_{luong,lsa}.npz (tools/gen_golden_rnn_step.py),
the seeded weights, the bounds, and AdamW in fp64 on sampled elements.

Bounds.  Gradients are compared on the fixture's strided samples in relative L2 norm:
  * discriminator parameters, and every parameter under an encoder (text_m.prenet / text_m.encoder / speech_m.prenet / speech_m.encoder: both
    generator sub-steps put a discriminator term on the encoder outputs): 1e-3, the split-bf16 GEMM path's parity bar (the discriminator's
    contractions are those GEMMs);
  * every other parameter: min(1e-3, 16 x max(common e32, own e32)), the project's rule (tests/rnn_decoder_mirror.grad_bounds);
  * the three tensors the zero-variance [SOS] prefix leaves ill-conditioned at eps = 1e-5: 16 x their own e32, uncapped, and not
    below the 1e-3 they share with the other encoder-side tensors; at eps = 0.1 (case a_eps) they follow the encoder rule;
  * conv biases in front of a train-mode BatchNorm have mathematically zero gradients: max|g| <= 1e-6 x ||grad W|| of their conv (text prenet at
    eps = 1e-5: max(1e-6, 16 x e32 of conv1's weight), tests/test_gpu_text_rnn_decoder_train.py).
Losses: 1e-3 x max(1, |ref|), the project's forward bound.  Pre-clip norm: min(1e-3, 16 x its own e32), relative.
BatchNorm running statistics: 2e-5 x max(1, max|ref|) (tests/test_cpu_text_rnn_decoder_train.BUF_TOL).  After the discriminator step the encoders
have run on the parameters the generator step moved -- by lr * sign(g), which the ill-conditioned gradients do not pin (see below) -- and the
reference's own fp32 run is off by up to 2e-4 there (e32/<case>/disc/state): that phase's bound is max(the above, 16 x the buffer's largest e32
over the cases of the same eps in both fixtures; buffer_bound).
Post-step parameters: AdamW's first move is lr * g / (|g| + eps), a sign, which amplifies gradient error near zero.  Every sampled element is
held to |dp - dp_ref| <= lr * (1e-3 + min(2, 2 d / |g_ref|)) + 4 ulp(p) with d = 8 x bound x ||g_ref|| / sqrt(n), eight times the root-mean-square
element error the tensor's gradient bound allows: an element with |g_ref| >> d must move exactly as the reference's, one with |g_ref| <= d may
land on either side (2 lr apart).  No element is excluded; `loose_share` reports how many are allowed more than lr / 2 (the degenerate biases,
whose reference gradient is rounding noise, are not compared).
"""
import json
import math
import os

import numpy as np
import torch

from unast_amd.portable import portable_tensor

HERE = os.path.dirname(os.path.abspath(__file__))
ATTNS = ("luong", "lsa")
CASES = ("a", "b", "a_eps")
LOSS_KEYS = ("t_ae", "s_ae", "d_ae", "asr_", "tts_", "sp_d", "d")
GRAD_CAP, GRAD_MARGIN, DISC_BAR = 1e-3, 16.0, 1e-3
LOSS_TOL, NORM_TOL, BUF_TOL, DEG_ABS = 1e-3, 1e-3, 2e-5, 1e-6
SIGN_SIGMAS, MOVE_TOL = 8.0, 1e-3
ENCODER_SIDE = ("text_m.prenet.", "text_m.encoder.", "speech_m.prenet.", "speech_m.encoder.")
ILL = ["text_m.prenet.embed.weight", "text_m.prenet.conv1.conv.weight", "text_m.prenet.batch_norm1.bias"]
DEG_TEXT = ["text_m.prenet.conv%d.conv.bias" % i for i in (1, 2, 3)]
DEG_SPEECH = ["speech_m.postnet.conv1.conv.bias"] + ["speech_m.postnet.conv_list.%d.conv.bias" % i for i in range(3)]
DEGENERATE = DEG_TEXT + DEG_SPEECH
BUFFERS = ("running_mean", "running_var", "num_batches_tracked")
_FX = {}


def fixture(attn):
    if attn not in _FX:
        _FX[attn] = np.load(os.path.join(HERE, "golden", "rnn_step_%s.npz" % attn))
    return _FX[attn]


def meta(attn):
    return json.loads(str(fixture(attn)["meta"]))


def configs():
    return json.load(open(os.path.join(HERE, "golden", "rnn_configs.json")))


def group(fx, name):
    """{key: sample} of a packed group (tools/gen_golden_rnn_step.pack)."""
    keys, off, data = json.loads(str(fx[name + "/keys"])), fx[name + "/off"], fx[name + "/data"]
    return {k: data[off[i]:off[i + 1]] for i, k in enumerate(keys)}


def sample_index(n, limit):
    return np.arange(0, n, max(1, -(-n // limit)))


def sample(v, limit):
    flat = np.asarray(v, dtype=np.float64).reshape(-1)
    return flat[sample_index(flat.size, limit)]


def state_dict(attn):
    m = meta(attn)
    return {k: torch.from_numpy(np.asarray(portable_tensor(k, s, m["seed"]))) for k, s in zip(m["keys"], m["shapes"])}


def args_of(attn, drops=0.0, **over):
    from types import SimpleNamespace
    cfg = dict(configs()["rnn_d_" + attn])
    cfg.update(load_path=None, ae_steps=1, sp_steps=1, cm_steps=0, d_steps=1, grad_clip=1.0)
    if drops is not None:
        cfg.update(t_pre_drop=drops, t_post_drop=drops, s_pre_drop=drops, s_post_drop=drops, e_drop=drops, d_drop=drops)
    cfg.update(over)
    return SimpleNamespace(**cfg)


def batch(attn, case):
    fx, c = fixture(attn), "a" if case == "a_eps" else case
    return (torch.from_numpy(fx[c + "/text"]), torch.from_numpy(fx[c + "/mel"]).float(), torch.from_numpy(fx[c + "/text_len"]), torch.from_numpy(fx[c + "/mel_len"]))


def reference(attn, case, tag):
    """(grad samples, grad norms, e32s) of one optimizer step ('gen' / 'disc') of a case, each {key: ...}."""
    fx = fixture(attn)
    g = group(fx, "%s/%s/g" % (case, tag))
    keys = list(g)
    return g, dict(zip(keys, fx["%s/%s/gnorm" % (case, tag)].tolist())), dict(zip(keys, fx["e32/%s/%s/grad" % (case, tag)].tolist()))


def grad_bounds(e32, case):
    """{key: bound} for the non-degenerate tensors of one optimizer step; also returns the common e32 of the decoder-side tensors."""
    plain = {k: v for k, v in e32.items() if k not in DEGENERATE and not k.startswith(ENCODER_SIDE) and not k.startswith("discriminator.")}
    common = 0.0
    if plain:
        med = float(np.median(list(plain.values())))
        common = max(v for v in plain.values() if v <= 10 * med)
    out = {}
    for k, v in e32.items():
        if k in DEGENERATE:
            continue
        if k.startswith("discriminator."):
            out[k] = DISC_BAR
        elif k.startswith(ENCODER_SIDE):
            out[k] = max(DISC_BAR, GRAD_MARGIN * v) if (k in ILL and case != "a_eps") else DISC_BAR
        else:
            out[k] = min(GRAD_CAP, GRAD_MARGIN * max(common, v))
    return out, common


def rel(got, ref):
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def adamw_first_steps(p, g, total_norm, lr, wd, max_norm=1.0, step=1, m=None, v=None, betas=(0.9, 0.999), eps=1e-8, decoupled=True):
    """torch.optim.AdamW (or Adam with L2 decay) after clip_grad_norm_(max_norm) in fp64 on arrays of elements; returns p after the step."""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    g = g * min(1.0, max_norm / (total_norm + 1e-6))
    m = np.zeros_like(p) if m is None else m
    v = np.zeros_like(p) if v is None else v
    if decoupled:
        p = p * (1 - lr * wd)
    else:
        g = g + wd * p
    m = betas[0] * m + (1 - betas[0]) * g
    v = betas[1] * v + (1 - betas[1]) * g * g
    den = np.sqrt(v) / math.sqrt(1 - betas[1] ** step) + eps
    return p - lr / (1 - betas[0] ** step) * m / den


def move_slack(g_ref_sample, gnorm, n, bound):
    """The per-element allowance min(2, 2 d / |g_ref|) of the post-step check, in units of lr (see the module docstring)."""
    d = SIGN_SIGMAS * bound * gnorm / math.sqrt(n)
    return np.minimum(2.0, 2.0 * d / np.maximum(np.abs(g_ref_sample), 1e-300))


def loose_share(slacks):
    flat = np.concatenate([np.asarray(v).reshape(-1) for v in slacks])
    return float((flat > 0.5).mean())


def buffer_bound(key, want, case, phase):
    """Bound of one running-statistics sample after an optimizer phase (see the module docstring).  The reference's own fp32 error after the
    discriminator step comes from a handful of sign flips of the first AdamW move, a draw per run: the yardstick is the largest one the
    buffer shows over the cases of the same eps in both fixtures."""
    base = BUF_TOL * max(1.0, float(np.abs(want).max()))
    if phase == "gen":
        return base
    group_cases = ("a_eps",) if case == "a_eps" else ("a", "b")
    e32 = 0.0
    for attn in ATTNS:
        fx = fixture(attn)
        for c in group_cases:
            e32 = max(e32, dict(zip(group(fx, "%s/disc/state" % c), fx["e32/%s/disc/state" % c].tolist()))[key])
    return max(base, GRAD_MARGIN * e32)


def norm_bound(fx, case, phase):
    """Relative bound of the pre-clip norm: the project's rule on the norm's own e32."""
    want = float(fx["%s/%s/norm" % (case, phase)])
    return min(NORM_TOL, GRAD_MARGIN * float(fx["e32/%s/%s/norm" % (case, phase)]) / want)
