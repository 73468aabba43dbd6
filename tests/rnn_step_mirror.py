"""fp64 mirror of unast_amd.train_rnn_step: the reference's auto-encoder, supervised and discriminator sub-steps and its optimizer step
(src/train.py:199-259, 296-363, 365-416, 446-463) as a composition of the existing mirrors -- tests/rnn_train_mirror.py (the encoders),
tests/rnn_decoder_mirror.py (the speech decoder), tests/text_decoder_mirror.py (the text decoder) -- with the losses, the LSTM discriminator,
the shuffle, clip_grad_norm_ and Adam(W) written out in torch on the CPU.  The pieces are chained the way the entry points chain them: a
forward pass of every piece, the losses' gradients with respect to the pieces' outputs, then every piece again with those as its cotangents.

It takes the kernels' dropout masks per tape ({tape name: {site name: factor tensor}}, tests/dropout_mirror.py) and the permutation.
FAULTS are deliberate mistakes a test plants to show that the checks would catch them.  Pinned to the reference's fixtures by
tests/test_cpu_rnn_step.py."""
import math

import numpy as np
import torch
import torch.nn as nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from tests import rnn_decoder_mirror as RM
from tests import rnn_train_mirror as TM
from tests import text_decoder_mirror as XM

F = nn.functional
H = 256
EOS_IDX, PAD_IDX = 2, 0
BUFFERS = ("running_mean", "running_var", "num_batches_tracked")
FAULTS = ("targets_not_flipped", "disc_grad_not_added", "frozen_disc_live", "no_accum_scale", "eval_encoders_in_d")


def _sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def _apply_buffers(sd, prefix, res, bns, updates):
    """Write a mirror call's running statistics back into the full state dict; num_batches_tracked += updates."""
    for bn in bns:
        for n in ("running_mean", "running_var"):
            sd[prefix + bn + "." + n] = res[bn + "." + n].detach().clone()
        sd[prefix + bn + ".num_batches_tracked"] = sd[prefix + bn + ".num_batches_tracked"] + updates


def _add(grads, prefix, g):
    for k, v in g.items():
        grads[prefix + k] = grads[prefix + k] + v if prefix + k in grads else v.clone()


# ---- losses (src/train.py:100-122, 147-148) --------------------------------------------------------------------------------------------------------
def text_loss(logits, gold, eos_weight):
    w = torch.ones(logits.shape[-1], dtype=logits.dtype)
    w[EOS_IDX] = eos_weight
    return F.cross_entropy(logits.permute(0, 2, 1), gold, weight=w, ignore_index=PAD_IDX)


def speech_loss(gold, pre, post, stop, mel_len, eos_weight):
    B, T, M = pre.shape
    mask = (torch.arange(T)[None, :] < mel_len[:, None]).to(pre.dtype)[:, :, None].expand(B, T, M)
    mse = lambda p: (((gold - p) ** 2) * mask).sum() / mask.sum()                                  # noqa: E731
    label = F.one_hot(mel_len - 1, T).to(pre.dtype)
    pw = torch.where(label.eq(1), torch.tensor(float(eos_weight), dtype=pre.dtype), torch.ones(1, dtype=pre.dtype))
    return mse(pre) + mse(post) + F.binary_cross_entropy_with_logits(stop, label, pos_weight=pw)


def _loss_cots(fn, outs, scale):
    """(loss value, gradients of scale x loss with respect to outs)."""
    leaves = [o.detach().clone().requires_grad_(True) for o in outs]
    loss = fn(*leaves)
    (loss * scale).backward()
    return loss.detach(), [x.grad.detach() for x in leaves]


# ---- the discriminator (src/network.py:172-186, src/module.py:297-336) -----------------------------------------------------------------------------------
def discriminator(dsd, x, lens, dtype, masks=None, slope=0.2):
    """LSTMDiscriminator.forward in train mode: packed bidirectional LSTM stack, reduce_h_W on the top layer's final [h_fwd | h_bwd],
    LeakyReLU, dropout, fc2.  Returns (logits [Bd], {name: Parameter})."""
    masks = masks or {}
    P = {k: nn.Parameter(v.detach().to(dtype).clone()) for k, v in dsd.items()}
    hid = dsd["rnn.rnn.weight_hh_l0"].shape[1]
    L = 1 + max(int(k.split("_l")[1][0]) for k in dsd if k.startswith("rnn.rnn.weight_ih_l"))
    lens_t = torch.as_tensor(lens, dtype=torch.int64)
    cur, top = x, None
    for l in range(L):
        lstm = nn.LSTM(cur.shape[-1], hid, num_layers=1, bidirectional=True, batch_first=True).to(dtype)
        for sfx in ("", "_reverse"):
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                delattr(lstm, n + "_l0" + sfx)
                setattr(lstm, n + "_l0" + sfx, P["rnn.rnn.%s_l%d%s" % (n, l, sfx)])
        lstm._flat_weights = [getattr(lstm, n) for n in lstm._flat_weights_names]
        po, (hn, _) = lstm(pack_padded_sequence(cur, lens_t, batch_first=True, enforce_sorted=False))
        cur, _ = pad_packed_sequence(po, batch_first=True, total_length=x.shape[1])
        top = torch.cat([hn[0], hn[1]], -1)
        if l + 1 < L and "d_inter" in masks:
            cur = cur * masks["d_inter"].to(dtype).reshape(cur.shape)
    r = F.leaky_relu(F.linear(top, P["rnn.reduce_h_W.weight"], P["rnn.reduce_h_W.bias"]), slope)
    if "d_head" in masks:
        r = r * masks["d_head"].to(dtype).reshape(r.shape)
    return F.linear(r, P["fc2.weight"], P["fc2.bias"]).squeeze(-1), P


def shuffle_batch(t_out, t_len, s_out, s_len, perm, train_discriminator):
    """src/train.py:296-329: both outputs zero-padded to max(Tt, Ts), text rows then speech rows, label-smoothed targets (text 0.9, speech 0.1;
    flipped unless the discriminator trains), everything permuted."""
    B, Tt, D = t_out.shape
    Ts = s_out.shape[1]
    Tm = max(Tt, Ts)
    d_hid = torch.zeros(2 * B, Tm, D, dtype=t_out.dtype)
    d_hid[:B, :Tt], d_hid[B:, :Ts] = t_out, s_out
    d_len = torch.cat([torch.as_tensor(t_len, dtype=torch.int64), torch.as_tensor(s_len, dtype=torch.int64)])
    tgt = torch.cat([torch.full((B,), 0.9), torch.full((B,), 0.1)]).to(t_out.dtype)
    if not train_discriminator:
        tgt = 1 - tgt
    perm = torch.as_tensor(perm, dtype=torch.int64)
    return d_hid[perm], d_len[perm], tgt[perm]


def _disc_term(sd, te, tl, se, sl, perm, scale, dtype, train_discriminator, fault, masks):
    flip_off = train_discriminator or fault == "targets_not_flipped"
    d_hid, d_len, tgt = shuffle_batch(te["enc_output"].to(dtype), tl, se["enc_output"].to(dtype), sl, perm, flip_off)
    d_hid = d_hid.clone().requires_grad_(True)
    out, P = discriminator(_sub(sd, "discriminator."), d_hid, d_len, dtype, masks)
    loss = F.binary_cross_entropy_with_logits(out, tgt)
    (loss * scale).backward()
    B, Tt, Ts = te["enc_output"].shape[0], te["enc_output"].shape[1], se["enc_output"].shape[1]
    g = torch.zeros_like(d_hid)
    g[torch.as_tensor(perm, dtype=torch.int64)] = d_hid.grad
    pgrads = {"discriminator." + k: p.grad.detach() for k, p in P.items() if p.grad is not None}
    return loss.detach(), g[:B, :Tt].detach(), g[B:, :Ts].detach(), pgrads, d_hid.grad.detach()


# ---- the sub-steps ----------------------------------------------------------------------------------------------------------------------------------
class Mirror:
    """State of a mirrored run: the full state dict (fp64 parameters, BatchNorm buffers), accumulated gradients {key: tensor} (absent = None),
    Adam moments and step counts per parameter, the losses dict."""

    def __init__(self, sd, attn, args, dtype=torch.float64, eps_text=1e-5, fault=None):
        assert fault in (None,) + FAULTS
        self.sd = {k: (v.detach().to(dtype).clone() if v.is_floating_point() else v.detach().clone()) for k, v in sd.items()}
        self.attn, self.args, self.dtype, self.eps_text, self.fault = attn, args, dtype, eps_text, fault
        self.grads, self.m, self.v, self.steps = {}, {}, {}, {}
        self.losses = {}
        self.last_norm = None
        self.disc_frozen = True
        self.record = {}

    def _encode(self, side, x, lens, masks, update=True):
        sub = _sub(self.sd, side + "_m.")
        B, T = x.shape[:2]
        zero = (torch.zeros(B, T, 2 * H), torch.zeros(2, B, H), torch.zeros(2, B, H))
        r = TM.run(side, sub, x, lens, zero, masks=masks, dtype=self.dtype, eps=self.eps_text)
        if side == "text" and update:
            _apply_buffers(self.sd, "text_m.", r, XM.PRE_BN, 1)
        return dict(r, x=x, lens=lens, masks=masks, sub=sub, side=side)

    def _encode_backward(self, e, cot):
        r = TM.run(e["side"], e["sub"], e["x"], e["lens"], cot, masks=e["masks"], dtype=self.dtype, eps=self.eps_text)
        _add(self.grads, e["side"] + "_m.", r["grads"])

    def _text_decode(self, text, mem, lens_k, masks, scale):
        sub = _sub(self.sd, "text_m.")
        run = lambda cot: XM.run(sub, self.attn, text, mem["enc_output"], mem["h"], mem["c"], lens_k, cot, masks=masks, dtype=self.dtype, eps=self.eps_text)   # noqa: E731
        fwd = run(torch.zeros(text.shape[0], text.shape[1], 46))
        loss, (d_logits,) = _loss_cots(lambda lg: text_loss(lg, text, self.args.t_eos_weight), [fwd["logits"]], scale)
        r = run(d_logits)
        _apply_buffers(self.sd, "text_m.", r, XM.PRE_BN, text.shape[1])
        _add(self.grads, "text_m.", r["grads"])
        return loss, (r["d_enc_output"], r["d_h"], r["d_c"])

    def _speech_decode(self, mel, mel_len, mem, lens_k, masks, scale):
        sub = _sub(self.sd, "speech_m.")
        mel = mel.to(self.dtype)
        run = lambda cot: RM.run(sub, self.attn, mel, mem["enc_output"], mem["h"], mem["c"], lens_k, cot, masks=masks, dtype=self.dtype)   # noqa: E731
        B, T, M = mel.shape
        fwd = run((torch.zeros(B, T, M), torch.zeros(B, T, M), torch.zeros(B, T)))
        ml = torch.as_tensor(mel_len, dtype=torch.int64)
        loss, cots = _loss_cots(lambda a, b, c: speech_loss(mel, a, b, c, ml, self.args.s_eos_weight), [fwd["pre"], fwd["post"], fwd["stop"]], scale)
        r = run(tuple(cots))
        _apply_buffers(self.sd, "speech_m.", r, RM.POST_BN, 1)
        _add(self.grads, "speech_m.", r["grads"])
        return loss, (r["d_enc_output"], r["d_h"], r["d_c"])

    def _generator(self, keys, text, tl, mel, ml, accum_steps, masks, perm, td_mem, sd_mem, mel_enc=None):
        masks = masks or {}
        scale = 1.0 if self.fault == "no_accum_scale" else 1.0 / accum_steps
        B = text.shape[0]
        perm = list(range(2 * B)) if perm is None else perm
        te = self._encode("text", text, tl, masks.get("text_enc"))
        if td_mem == "text":
            t_loss, t_cot = self._text_decode(text, te, tl, masks.get("text_dec"), scale)
        se = self._encode("speech", mel if mel_enc is None else mel_enc.to(self.dtype), ml, masks.get("speech_enc"))
        s_loss, s_cot = self._speech_decode(mel, ml, se if sd_mem == "speech" else te, ml if sd_mem == "speech" else tl, masks.get("speech_dec"), scale)
        if td_mem == "speech":
            t_loss, t_cot = self._text_decode(text, se, ml, masks.get("text_dec"), scale)
        cots = {td_mem: list(t_cot), sd_mem: list(s_cot)}
        vals = [t_loss, s_loss]
        if self.args.use_discriminator:
            d_loss, dth, dsh, pg, _ = _disc_term(self.sd, te, tl, se, ml, perm, scale, self.dtype, False, self.fault, masks.get("disc"))
            vals.append(d_loss)
            self.record.update(d_t_enc=dth, d_s_enc=dsh)
            if self.fault != "disc_grad_not_added":
                cots["text"][0] = cots["text"][0] + dth
                cots["speech"][0] = cots["speech"][0] + dsh
            if self.fault == "frozen_disc_live":                                                  # its gradients kept: counted in the clip norm and stepped
                _add(self.grads, "", pg)
        self._encode_backward(te, tuple(cots["text"]))
        self._encode_backward(se, tuple(cots["speech"]))
        for k, v in zip(keys, vals):
            self.losses.setdefault(k, []).append(float(v))

    def ae_step(self, text, tl, mel, ml, accum_steps, masks=None, perm=None):
        """train_ae_step: masks may hold 'noise' row masks in text_enc / speech_enc."""
        self._generator(("t_ae", "s_ae", "d_ae"), text, tl, mel, ml, accum_steps, masks, perm, "text", "speech")

    def sp_step(self, text, tl, mel, ml, accum_steps, masks=None, perm=None, mel_aug=None):
        """train_sp_step; mel_aug: what the speech encoder reads (specaugment(mel); None = mel)."""
        self._generator(("asr_", "tts_", "sp_d"), text, tl, mel, ml, accum_steps, masks, perm, "speech", "text", mel_enc=mel_aug)

    def d_step(self, text, tl, mel, ml, accum_steps, masks=None, perm=None):
        masks = masks or {}
        update = self.fault != "eval_encoders_in_d"
        te = self._encode("text", text, tl, masks.get("text_enc"), update=update)
        se = self._encode("speech", mel, ml, masks.get("speech_enc"))
        B = text.shape[0]
        perm = list(range(2 * B)) if perm is None else perm
        scale = 1.0 if self.fault == "no_accum_scale" else 1.0 / accum_steps
        d_loss, _, _, pg, _ = _disc_term(self.sd, te, tl, se, ml, perm, scale, self.dtype, True, None, masks.get("disc"))
        _add(self.grads, "", pg)
        self.losses.setdefault("d", []).append(float(d_loss))

    # ---- clip_grad_norm_ -> Adam(W) -> zero_grad(set_to_none=True) (src/train.py:358-363) -----------------------------------------------------------
    def optimizer_step(self, lr, weight_decay, grad_clip=1.0, decoupled=True, betas=(0.9, 0.999), eps=1e-8):
        grads = self.grads
        step_keys = list(grads)
        norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads.values()))
        self.last_norm = norm
        coef = min(1.0, grad_clip / (norm + 1e-6)) if grad_clip > 0 else 1.0
        for k in step_keys:
            g, p = grads[k] * coef, self.sd[k]
            t = self.steps[k] = self.steps.get(k, 0) + 1
            if decoupled:
                p = p * (1 - lr * weight_decay)
            else:
                g = g + weight_decay * p
            m = self.m[k] = betas[0] * self.m.get(k, torch.zeros_like(p)) + (1 - betas[0]) * g
            v = self.v[k] = betas[1] * self.v.get(k, torch.zeros_like(p)) + (1 - betas[1]) * g * g
            self.sd[k] = p - lr / (1 - betas[0] ** t) * m / (v.sqrt() / math.sqrt(1 - betas[1] ** t) + eps)
        self.last_grads, self.grads = grads, {}
        return norm


def run_sequence(sd, attn, args, batch, dtype=torch.float64, eps_text=1e-5, fault=None, masks=None, perms=None, mel_aug=None):
    """The fixture's sequence: AE sub-step, SP sub-step, generator optimizer_step, D sub-step, discriminator optimizer_step (accum_steps 2,
    d_steps 1).  masks / perms: {'ae' | 'sp' | 'd': ...}; mel_aug: what the supervised sub-step's speech encoder read.  Returns the Mirror plus per optimizer step its gradients, norm and state."""
    text, mel, tl, ml = batch
    tl, ml = [int(v) for v in np.asarray(tl)], [int(v) for v in np.asarray(ml)]
    mel = mel.to(dtype)
    masks, perms = masks or {}, perms or {}
    mir = Mirror(sd, attn, args, dtype, eps_text, fault)
    out = {}
    mir.ae_step(text, tl, mel, ml, 2, masks.get("ae"), perms.get("ae"))
    mir.sp_step(text, tl, mel, ml, 2, masks.get("sp"), perms.get("sp"), mel_aug=mel_aug)
    out["gen_grads"] = dict(mir.grads)
    out["gen_norm"] = mir.optimizer_step(args.lr, args.weight_decay, args.grad_clip, args.optim_type == "adamw")
    out["gen_state"] = dict(mir.sd)
    mir.d_step(text, tl, mel, ml, 1, masks.get("d"), perms.get("d"))
    out["disc_grads"] = dict(mir.grads)
    out["disc_norm"] = mir.optimizer_step(args.lr, args.weight_decay, args.grad_clip, args.optim_type == "adamw")
    out["disc_state"] = dict(mir.sd)
    out["losses"] = {k: v[0] for k, v in mir.losses.items()}
    out["steps"] = dict(mir.steps)
    out["mirror"] = mir
    return out
