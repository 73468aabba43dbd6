"""Evaluating the RNN family on the HIP path: the reference's evaluate() (src/train.py:474-565) for UNAST(TextRNN, SpeechRNN[, LSTMDiscriminator])
as explicit entry points, like unast_amd.train_rnn_step's.  unast_amd.train's own dispatch for this family is left as it is.  DESIGN 5o.

    autoencoder_losses(model, batch, args)   -> (t_ae, s_ae[, d_ae])       src/train.py:199-229
    supervised_losses(model, batch, args)    -> (asr, tts[, d_sp])         src/train.py:231-259
    crossmodel_losses(model, batch, args)    -> (t_cm, s_cm[, d_cm])       src/train.py:261-294, src/network.py:103-123
    discriminator_eval(model, batch, args)   -> (d_loss, (d_out, d_target))    src/train.py:337-354
    evaluate(model, valid_dataloader, step, args, is_test=False), evaluate_main(args, test_dataloader)

Everything runs under torch.no_grad() on the current stream in model.eval() (each call puts the model there and leaves it there; the train
sub-steps switch back themselves): BatchNorm on its running statistics, no dropout, B = 1 legal.  Nothing keeps a tape or runs a backward;
parameters, gradients, optimizer state, model._rnn_touched and every BatchNorm buffer are left as they are.  noise_fn and specaugment do not
look at model.training, so the auto-encoder inputs are still noised (a row mask with p = 0.3 on the embedded text and on the input mel) and
the ASR input still augmented -- unless utils.is_deterministic(), as in the train sub-steps.  The cross-model losses generate with the EVAL
generation of unast_amd.rnn (the reference's evaluate() runs cm_speech_in / cm_text_in under model.eval()); a generated PAD id inside a
sequence's length stays an attention key (DESIGN 5m point 5), model._rnn_cm_live_pad counts them for the last call.  The losses are the
forward loss kernels (unast_text_loss_fwd, unast_speech_loss_fwd, unast_bce_logits); PER is utils.compute_per_device (csrc/metrics.hip).
With train_rnn_step.RECORD the seeds and mask sites of the two noise draws, the permutation, mel_aug and the generated sequences are left in
model._rnn_step_record.
"""
import json
import os
from collections import defaultdict

import torch

from . import ops, rnn, train_rnn_step as S
from .train_rnn import NOISE_P, S_NOISE, Site
from .utils import PAD_IDX, is_deterministic, next_seed, specaugment

_F32 = torch.float32
TEXT_MAX_LEN, SPEECH_MAX_LEN = 300, 815                    # infer_sequence's defaults (src/network.py:312, 586): the caps of every generation here (tests patch them down)


def _check(model, args):
    if not S.is_rnn_model(model):
        raise TypeError("model must be UNAST(TextRNN, SpeechRNN[, LSTMDiscriminator]) (train.initialize_model with model_type='rnn')")
    if args.use_discriminator and model.discriminator is None:
        raise ValueError("args.use_discriminator is set but the model has no discriminator")
    if next(model.parameters()).device.type != "cuda":
        raise RuntimeError("unast_amd runs on the GPU only: move the model to a CUDA (ROCm) device first; there is no CPU path")
    if model.training:
        model.eval()


def _process(batch):
    """process_batch (src/train.py:80-94): tensors on the device, lengths as host lists and as int32 device tensors."""
    from . import train as T
    text, mel, text_len, mel_len = batch
    dev = T._dev()
    tl, ml = [int(v) for v in text_len.tolist()], [int(v) for v in mel_len.tolist()]
    text, mel = text.to(dev, non_blocking=True), mel.to(dev, _F32, non_blocking=True).contiguous()
    return text, mel, tl, ml, torch.tensor(tl, dtype=torch.int32, device=dev), torch.tensor(ml, dtype=torch.int32, device=dev)


def _record(model):
    if not S.RECORD:
        return None
    rec = model.__dict__.setdefault("_rnn_step_record", {})
    rec.clear()
    return rec


def _encode(m, x, lens, noise_seed=None, lens_mask=False):
    """m.encode(x, lens) in eval mode, with noise_fn in front when a seed is given.  Returns (enc_outputs, mask, site): mask is what the
    decoders take -- the model's own pad mask, or (lens_mask) the int lengths, for generated text whose PAD ids must not shorten it."""
    m._check_call()
    li = m._enc_lens(x, lens)
    P = m._pack()
    noise = None if noise_seed is None else (NOISE_P, int(noise_seed), S_NOISE)
    if m._side == "text":
        ids = m._ids(x)
        front, mask = rnn.text_frontend(P, ids, noise), ids.eq(PAD_IDX)
    else:
        mel = m._mel(x)
        front, mask = rnn.speech_frontend(P, mel, noise), torch.arange(mel.shape[1], device=mel.device)[None, :] >= li[:, None]
    enc_outputs, mask = m._encode(P, front, li, mask)
    site = None if noise is None else Site("noise", NOISE_P, int(noise_seed), S_NOISE, 0, x.shape[0] * x.shape[1], 1, "row")
    return enc_outputs, (li if lens_mask else mask), site


def _text_loss(logits, gold, eos_weight):
    """text_loss (src/train.py:105-111) of teacher-forced logits [B,T,V]; the generation's own padded head buffer is read in place."""
    from . import train as T
    B, Tn, V = logits.shape
    ldl = (V + 3) // 4 * 4
    if logits.stride() == (Tn * ldl, ldl, 1):
        l2d = logits.as_strided((B * Tn, V), (ldl, 1))
    else:
        l2d = torch.zeros(B * Tn, ldl, dtype=_F32, device=logits.device)
        l2d[:, :V].copy_(logits.reshape(B * Tn, V))
    loss = torch.empty(1, dtype=_F32, device=logits.device)
    ops.text_loss_fwd(l2d, gold.contiguous().view(-1), V, float(eos_weight), T._loss_ws(logits.device), loss)
    return loss.view(())


def _speech_loss(pre, post, stop, gold, lens_dev, eos_weight):
    """speech_loss (src/train.py:113-122) of teacher-forced frames: [pre | stop | pad] gathered into the head layout the kernel reads."""
    from . import train as T
    B, Tn, M = pre.shape
    ldh = (M + 1 + 3) // 4 * 4
    head = torch.zeros(B, Tn, ldh, dtype=_F32, device=pre.device)
    head[:, :, :M].copy_(pre)
    head[:, :, M].copy_(stop.reshape(B, Tn))
    loss = torch.empty(1, dtype=_F32, device=pre.device)
    ops.speech_loss_fwd(gold, head, post.contiguous(), lens_dev, float(eos_weight), T._loss_ws(pre.device), loss)
    return loss.view(())


def _disc_term(model, t_enc, t_len, s_enc, s_len, train_discriminator, rec):
    """discriminator_shuffle_batch + discriminator_hidden_to_loss (src/train.py:296-335), forward only."""
    from . import train as T
    d_hid, d_len, d_target, perm = S._shuffle(t_enc, t_len, s_enc, s_len, train_discriminator)
    d_out = model.discriminator(d_hid, d_len).detach()
    d_loss = T.discriminator_loss(d_out, d_target).detach()
    if rec is not None:
        rec.update(perm=perm, d_len=d_len, d_target=d_target, d_out=d_out)
    return d_loss.view(()), (d_out, d_target)


@torch.no_grad()
def autoencoder_losses(model, batch, args):
    """autoencoder_step under model.eval(): (t_ae, s_ae[, d_ae]) as device scalars."""
    _check(model, args)
    text, mel, tl, ml, tl_dev, ml_dev = _process(batch)
    tm, sm = model.text_m, model.speech_m
    rec = _record(model)
    noise = not is_deterministic()
    te, t_mask, t_site = _encode(tm, text, tl, next_seed() if noise else None)
    logits = tm.decode_sequence(text, tl_dev, te, t_mask)
    se, s_mask, s_site = _encode(sm, mel, ml, next_seed() if noise else None)
    pre, post, stop, _ = sm.decode_sequence(mel, ml_dev, se, s_mask)
    out = [_text_loss(logits, text, args.t_eos_weight), _speech_loss(pre, post, stop, mel, ml_dev, args.s_eos_weight)]
    if args.use_discriminator:
        out.append(_disc_term(model, te, tl_dev, se, ml_dev, False, rec)[0])
    if rec is not None:
        rec.update(sites=dict(text_noise=t_site, speech_noise=s_site), seeds=[s.seed if s else None for s in (t_site, s_site)])
    return tuple(out)


@torch.no_grad()
def supervised_losses(model, batch, args):
    """supervised_step under model.eval(): (asr, tts[, d_sp]); specaugment on the ASR input unless deterministic."""
    _check(model, args)
    text, mel, tl, ml, tl_dev, ml_dev = _process(batch)
    tm, sm = model.text_m, model.speech_m
    rec = _record(model)
    mel_aug = mel if is_deterministic() else specaugment(mel, ml_dev)
    te, t_mask, _ = _encode(tm, text, tl)
    pre, post, stop, _ = sm.decode_sequence(mel, ml_dev, te, t_mask)
    se, s_mask, _ = _encode(sm, mel_aug, ml)
    logits = tm.decode_sequence(text, tl_dev, se, s_mask)
    out = [_text_loss(logits, text, args.t_eos_weight), _speech_loss(pre, post, stop, mel, ml_dev, args.s_eos_weight)]
    if args.use_discriminator:
        out.append(_disc_term(model, te, tl_dev, se, ml_dev, False, rec)[0])
    if rec is not None:
        rec.update(mel_aug=mel_aug)
    return tuple(out)


@torch.no_grad()
def crossmodel_losses(model, batch, args):
    """crossmodel_step under model.eval(), speech-in first: (t_cm, s_cm[, d_cm]).  The generated sequences are cut to their longest length
    before they are re-encoded (encode needs max(lens) == T); the discriminator term takes the GENERATED lengths."""
    _check(model, args)
    text, mel, tl, ml, tl_dev, ml_dev = _process(batch)
    tm, sm = model.text_m, model.speech_m
    rec = _record(model)
    dev = text.device
    # speech in: speech encoder -> greedy text -> text encoder -> teacher-forced speech decoder
    s_mem, s_mem_mask, _ = _encode(sm, mel, ml)
    tokens, t_lens = tm.generation(s_mem, s_mem_mask, TEXT_MAX_LEN).run()
    gtl = [int(v) for v in t_lens.tolist()]
    tokens = tokens[:, :max(gtl)].contiguous()
    gtl_dev = torch.tensor(gtl, dtype=torch.int32, device=dev)
    live = torch.arange(tokens.shape[1], device=dev)[None, :] < gtl_dev[:, None]
    model.__dict__["_rnn_cm_live_pad"] = int(((tokens == PAD_IDX) & live).sum())
    te, t_mask, _ = _encode(tm, tokens, gtl, lens_mask=True)
    pre, post, stop, _ = sm.decode_sequence(mel, ml_dev, te, t_mask)
    s_cm = _speech_loss(pre, post, stop, mel, ml_dev, args.s_eos_weight)
    # text in: text encoder -> greedy speech -> speech encoder -> teacher-forced text decoder
    t_mem, t_mem_mask, _ = _encode(tm, text, tl)
    g_pre, g_post, g_stop, s_lens = sm.generation(t_mem, t_mem_mask, SPEECH_MAX_LEN).run()
    gsl = [int(v) for v in s_lens.tolist()]
    frames = g_post[:, :max(gsl)].contiguous()
    gsl_dev = torch.tensor(gsl, dtype=torch.int32, device=dev)
    se, s_mask, _ = _encode(sm, frames, gsl)
    logits = tm.decode_sequence(text, tl_dev, se, s_mask)
    t_cm = _text_loss(logits, text, args.t_eos_weight)
    out = [t_cm, s_cm]
    if args.use_discriminator:
        out.append(_disc_term(model, te, gtl_dev, se, gsl_dev, False, rec)[0])
    if rec is not None:
        rec.update(gen_text=(tokens, t_lens), gen_speech=(g_pre, g_post, g_stop, s_lens), live_pad=model._rnn_cm_live_pad)
    return tuple(out)


@torch.no_grad()
def discriminator_eval(model, batch, args):
    """discriminator_step under model.eval(): eval encoders, unflipped targets; (d_loss, (d_out, d_target))."""
    _check(model, args)
    if model.discriminator is None:
        raise ValueError("discriminator_eval: the model has no discriminator")
    text, mel, tl, ml, tl_dev, ml_dev = _process(batch)
    rec = _record(model)
    te, _, _ = _encode(model.text_m, text, tl)
    se, _, _ = _encode(model.speech_m, mel, ml)
    return _disc_term(model, te, tl_dev, se, ml_dev, True, rec)


PER_ON_DEVICE = True       # evaluate()'s PER through utils.compute_per_device (csrc/metrics.hip); False: utils.compute_per on the host


def evaluate(model, valid_dataloader, step, args, is_test=False):
    """src/train.py:474-565 for model_type == 'rnn': (per, losses[, d_score]) with unast_amd.train.evaluate's loss keys and order.
    PER runs on the device (utils.compute_per_device), whose kernel takes min(B * T_text, B * generated length) <= ops.EDIT_MAX_COLS = 65536 ids
    of CAPACITY, padding included: a batch beyond that (eval_batch_size > 218 at the text cap of 300) raises ValueError; set
    PER_ON_DEVICE = False to take utils.compute_per on the host instead."""
    import numpy as np
    from . import train as T
    from .utils import compare_outputs, compute_per, compute_per_device
    _check(model, args)
    if is_test:
        os.makedirs(os.path.join(args.out_test_dir, 'mels'), exist_ok=True)
    losses = defaultdict(list)
    per, n_iters, d_score = 0, 0, 0
    text_pred_dict = {}
    with torch.no_grad():
        for batch in valid_dataloader:
            if is_test:
                batch, fnames = batch
            out = autoencoder_losses(model, batch, args)
            losses['t_ae'].append(out[0].item())
            losses['s_ae'].append(out[1].item())
            if args.use_discriminator:
                losses['d_ae'].append(out[2].item())
            out = supervised_losses(model, batch, args)
            losses['asr'].append(out[0].item())
            losses['tts'].append(out[1].item())
            if args.use_discriminator:
                losses['d_sp'].append(out[2].item())
            out = crossmodel_losses(model, batch, args)
            losses['s_cm'].append(out[1].item())
            losses['t_cm'].append(out[0].item())
            if args.use_discriminator:
                losses['d_cm'].append(out[2].item())
            if args.use_discriminator:
                d_loss, d_output = discriminator_eval(model, batch, args)
                losses['dis'].append(d_loss.item())
                if is_test:
                    d_score += T.compute_d_score(d_output[0], d_output[1]).item() / args.eval_batch_size / 2
            text, mel, tl, ml, tl_dev, ml_dev = _process(batch)
            s_mem, s_mask, _ = _encode(model.speech_m, mel, ml)               # model.asr(None, None, mel, mel_len, infer=True) under this module's cap
            text_pred, text_pred_len = model.text_m.generation(s_mem, s_mask, TEXT_MAX_LEN).run()
            if PER_ON_DEVICE:
                per += compute_per_device(text, text_pred, tl_dev, text_pred_len)
            else:
                per += compute_per(text, text_pred, tl_dev, text_pred_len)
            n_iters += 1
            if is_test:
                tp, tpl = text_pred.cpu(), text_pred_len.cpu()
                for gt, gt_len, pred, pred_len, fname in zip(text.cpu(), tl, tp, tpl, fnames):
                    text_pred_dict[fname] = {'gt': gt.tolist()[:gt_len], 'pred': pred.tolist()[:pred_len.item()]}
                t_mem, t_mask, _ = _encode(model.text_m, text, tl)              # model.tts(text, text_len, None, None, infer=True)
                _, post_pred, _, stop_lens = model.speech_m.generation(t_mem, t_mask, SPEECH_MAX_LEN).run()
                for pred, stop_len, fname in zip(post_pred.cpu(), stop_lens.cpu(), fnames):
                    np.save(os.path.join(args.out_test_dir, 'mels', fname + '.pt'), pred.numpy()[:stop_len.item()])
        if n_iters == 0:
            raise ValueError("evaluate: empty dataloader")
        compare_outputs(text[-1], text_pred[-1], tl[-1], text_pred_len[-1])
    if is_test:
        json.dump(text_pred_dict, open(os.path.join(args.out_test_dir, 'text_preds.json'), 'w'))
        return per / n_iters, losses, d_score / n_iters
    return per / n_iters, losses


def evaluate_main(args, test_dataloader):
    """src/train.py:985-999 with the dataloader passed in, as unast_amd.train.evaluate_main."""
    from . import train as T
    from .utils import set_seed
    set_seed(args.seed)
    s_epoch, _, model, _, _ = T.initialize_model(args)
    per, eval_losses, d_score = evaluate(model, test_dataloader, s_epoch, args, is_test=True)
    T.log_loss_metrics(eval_losses, s_epoch, eval=True)
    print("per : {}".format(per))
    print("d_score : {}".format(d_score))
    return per, eval_losses, d_score
