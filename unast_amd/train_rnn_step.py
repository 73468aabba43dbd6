"""Training the RNN family on the HIP path: the reference's auto-encoder, supervised and discriminator sub-steps and its optimizer step
(src/train.py:199-259, 296-363, 365-416, 446-463, 910-959) for UNAST(TextRNN, SpeechRNN[, LSTMDiscriminator]).  unast_amd.train's entry points
(initialize_model, train_ae_step, train_sp_step, train_discriminator_step, optimizer_step, discriminator_shuffle_batch, train, train_step)
dispatch here when args.model_type == 'rnn'.  DESIGN 5l.

The generators are not autograd modules: every sub-step composes the explicit tape calls of unast_amd.train_rnn (encoder_forward /
encoder_backward, decoder_forward / decoder_backward, text_decoder_forward / text_decoder_backward) with the loss kernels
(unast_text_loss_*, unast_speech_loss_*, unast_bce_logits, unast_scalar_combine) under torch.no_grad() on the current stream; the latent
discriminator is the transformer family's (functional.lstm_discriminator, split-bf16 GEMMs) and runs through its own autograd segment, fed a
leaf tensor whose gradient comes back as the discriminator's input gradient.  Gradients are scaled by 1 / accum_steps inside the loss
kernels' backward (their upstream-gradient scalar) and ADD into p.grad; optimizer_step leaves every gradient zero, so the first sub-step
after it starts from zero.

Where what lives.  The discriminator keeps living in the model's FlatStore (UNAST._store() of an RNN model covers the discriminator alone:
its kernels address its LSTM weights as spans of that buffer); the optimizer takes the store's 'disc' region as one more segment next to
its own two -- flat parameter and gradient buffers for text_m and for speech_m with p.data / p.grad as views (flat_adam.adopt;
contract.prepare_grads keeps such a .grad in place).  Segments, launch sequence and (de)serialisation are unast_amd.flat_adam's, shared with
the transformer's and the vocoder's optimizers; this module decides which segments step.  A segment whose gradients were not produced since
the last zero_grad is skipped entirely -- no decay, no moment update, no step count, no share in the clip norm: torch.optim's
`grad is None`.  'Produced' is tracked on the host (model._rnn_touched, FlatStore.touched).

The cross-model (back-translation) step is train_cm_step below, and train_step here is the step with cm_steps >= 0: both are explicit
entry points of this module.  unast_amd.train's own train_cm_step / crossmodel_step / train(args) with cm_steps > 0 keep raising CM_REASON for
model_type='rnn' (flipping that dispatch is a follow-up).

Data parallel.  With torch.distributed initialised every rank runs the sub-steps on its own batch, and RNNFlatAdamW.step sums the
flat gradient buffers of the segments it is about to step over the ranks and scales them by 1 / world before the clip norm is taken
(unast_amd.ddp.finish_segments: blocking, on the current stream, one collective per segment).  Which segments step is a function of the
phase -- text_m and speech_m after generator sub-steps, disc after discriminator sub-steps -- and is checked locally before the first
collective.  BatchNorm statistics stay per rank; sync_buffers() makes them rank `src`'s before evaluating or saving.

Out of scope (raise NotImplementedError): graph capture, side streams, B = 1, and autoencoder_step / supervised_step /
crossmodel_step called directly (they would have to return autograd-connected losses).  evaluate() lives in unast_amd.eval_rnn.
"""
import torch

from . import flat_adam, ops, train_rnn
from .rnn import PACK_SLOTS
from .utils import is_deterministic, next_seed, specaugment

_F32 = torch.float32
GEN_SEGMENTS = ("text_m", "speech_m")
PHASE_SEGMENTS = (GEN_SEGMENTS, ("disc",))                 # what one optimizer phase steps, in segment order: the generator phase, the D phase
CM_REASON = ("the cross-model step is not built for model_type='rnn' behind this entry point: UNAST.cm_text_in / cm_speech_in generate in train mode "
             "-- dropout is on inside greedy decoding and TextPrenet normalises each generated prefix [SOS, c0, ..] with its own batch statistics at "
             "every position -- which the eval generation of this path does not do; train with cm_steps = 0, or call the explicit entry points "
             "unast_amd.train_rnn_step.train_cm_step / unast_amd.train_rnn_step.train_step, which generate with "
             "unast_amd.train_rnn.text_generate_train / speech_generate_train")
DIRECT_REASON = ("%s is not built for model_type='rnn' (the RNN generators are explicit tape calls under torch.no_grad(); it would have to return "
                 "autograd-connected losses): call %s, which runs the forward, the losses and the backward into .grad")
RECORD = False          # True (tests): every sub-step leaves its tapes, permutation and discriminator batch in model._rnn_step_record


def is_rnn_model(model):
    from .network import _RNNModel
    return isinstance(getattr(model, "text_m", None), _RNNModel)


def _touched(model):
    return model.__dict__.setdefault("_rnn_touched", set())


def drop_cached_operands(model):
    """The optimizer's kernels write the parameters behind torch's version counters, on which the models' derived operands are keyed."""
    for m in (model.text_m, model.speech_m):
        for slot in PACK_SLOTS:
            m.__dict__.pop(slot, None)


def sync_buffers(model, src=0):
    """Data-parallel runs keep BatchNorm running statistics and num_batches_tracked per rank while training (the reference has no SyncBN; the
    transformer family's policy).  Before evaluating or saving, this makes every buffer of text_m and speech_m rank `src`'s -- one
    broadcast per buffer over the launcher's process group -- and drops the cached operand packs, since eval packs fold those statistics.
    Returns the number of buffers broadcast; 0, and nothing changes, when not distributed."""
    from . import ddp
    dist = ddp._dist()
    if dist is None:
        return 0
    n = 0
    with torch.no_grad():
        for m in (model.text_m, model.speech_m):
            for b in m.buffers():
                dist.broadcast(b, src=src)
                n += 1
    drop_cached_operands(model)
    return n


# ---- the optimizer ------------------------------------------------------------------------------------------------------------------------------
class RNNFlatAdamW(flat_adam.FlatAdam):
    """flat_adam.FlatAdam over UNAST(TextRNN, SpeechRNN[, D]): one unast_sumsq and one unast_adamw launch per segment that has gradients.
    Segments: text_m, speech_m (flat buffers this optimizer adopts the parameters into) and the discriminator (the 'disc' region of the model's
    FlatStore on the GPU; adopted like the other two on a CPU / meta model, where only state_dict() and load_state_dict() work)."""

    def __init__(self, model, lr, weight_decay=0.0, decoupled=True, betas=(0.9, 0.999), eps=1e-8):
        params = list(model.parameters())
        if not params or any(p.dtype is not _F32 for p in params):
            raise ValueError("RNNFlatAdamW: float32 parameters")
        segments = [flat_adam.adopt(n, list(getattr(model, n).parameters())) for n in GEN_SEGMENTS]
        disc = model.discriminator
        self.model, self._store = model, None
        if disc is not None:
            dparams = list(disc.parameters())
            if dparams[0].is_cuda:
                st = self._store = model._store()
                a, b = st.regions["disc"]
                names = {id(p): n for n, p in st.params.items()}
                live = [p for p in dparams if a <= st.offsets[names[id(p)]] < b]                   # (reduce_c_W sits in 'disc_unused': never has a gradient)
                segments.append(flat_adam.Segment("disc", live, [st.offsets[names[id(p)]] - a for p in live], st.flat[a:b], st.grad[a:b], st.flat_split[a:b]))
            else:
                segments.append(flat_adam.adopt("disc", dparams))
        super().__init__(params, segments, lr, weight_decay, betas, eps, decoupled)
        self.last_stepped = []
        drop_cached_operands(model)

    def _has_grads(self, seg):
        if seg.name == "disc":
            return self._store is not None and "disc" in self._store.touched
        return seg.name in _touched(self.model)

    def _adopt_grads(self, seg):
        """A .grad that was re-created outside the flat buffer (set to None and produced again) is copied in and re-pointed."""
        for p, o in zip(seg.params, seg.offsets):
            view = seg.grad[o:o + p.numel()].view(p.shape)
            g = p.grad
            if g is None or g.data_ptr() != view.data_ptr():
                if g is not None:
                    view.copy_(g)
                p.grad = view

    def _exchange(self, segs):
        """Data-parallel step: the gradients of exactly the segments about to step become their mean over the ranks, before the clip
        norm is taken -- one blocking all-reduce per segment on the current stream, in segment order, then the 1 / world scale.  The disc
        segment's buffer is the store's gradient range it already holds.
        Every rank has to issue the same collectives or none of them completes, so which segments step must not depend on a rank's data.  It
        does not: a generator sub-step (AE, CM or SP) touches both text_m and speech_m, a discriminator sub-step touches disc alone.  That is
        checked here, locally, before the first collective; a rank that sees anything else raises instead of waiting inside one.
        Nothing before this point takes part in a collective.  In particular the ranks of a cross-model sub-step generate sequences of
        different lengths, issue different numbers of launches and read the stop flags back (train_rnn.SYNC_EVERY) at different times: all
        of that stays local to the rank."""
        from . import ddp
        names = tuple(s.name for s in segs)
        if names not in PHASE_SEGMENTS:
            raise RuntimeError("data-parallel optimizer step: the segments with gradients are (%s); one optimizer phase steps (%s): generator "
                               "sub-steps touch text_m and speech_m, discriminator sub-steps touch disc, and every rank must exchange the same "
                               "segments" % (", ".join(names), ") or (".join(", ".join(p) for p in PHASE_SEGMENTS)))
        ddp.finish_segments([s.grad for s in segs], names)

    @torch.no_grad()
    def step(self, max_norm=0.0, closure=None):
        from . import ddp
        segs = [s for s in self.segments if self._has_grads(s)]
        self.last_stepped = [s.name for s in segs]
        if not segs:
            return                                         # (a phase without sub-steps: a function of args, the same on every rank)
        for s in segs:
            if s.name != "disc":
                self._adopt_grads(s)
        if ddp.active():
            self._exchange(segs)
        self._launch(segs, max_norm)
        if self._store is not None and "disc" in self.last_stepped:
            self._store.refresh_T(["disc"])                # W^T copies and tiled bf16 planes of what was just updated (train.FusedAdamW.step)
            self._store.refresh_planes(["disc"])
        drop_cached_operands(self.model)

    def zero_grad(self, set_to_none=True):
        """Gradients of the generators stay views of the flat buffers, zeroed (what the next sub-step adds into); the discriminator's go back to
        the store's convention (zeroed region, p.grad None)."""
        touched = _touched(self.model)
        for s in self.segments:
            if s.name != "disc" and s.name in touched:
                s.grad.zero_()
        touched.clear()
        if self._store is not None:
            self._store.zero_grad()


_MODEL_KEYS = ("hidden", "e_in", "t_emb_dim", "s_pre_hid", "num_layers", "e_bi", "d_attn", "attn_dim", "num_mels")      # what network._rnn_check_args reads
ENC_WIDTH = 512                                            # enc_output of the built configuration: 2 x hidden, the discriminator's input width


def build(args, device):
    """The model and optimizer of initialize_model for model_type == 'rnn' (src/train.py:914-932)."""
    from .network import TextRNN, SpeechRNN, LSTMDiscriminator, UNAST
    from .network import _RNN_BUILT
    from .utils import get_teacher_ratio
    missing = [k for k in _MODEL_KEYS if not hasattr(args, k)]
    if missing:                                            # an args that does not state the one configuration the family is built for
        raise NotImplementedError("%s; args does not set %s" % (_RNN_BUILT, ", ".join(missing)))
    text_m, speech_m, discriminator = TextRNN(args), SpeechRNN(args), None
    if args.use_discriminator:
        discriminator = LSTMDiscriminator(2 * args.hidden, args.disc_hid, bidirectional=args.disc_bidirectional, num_layers=args.disc_num_layers)
    model = UNAST(text_m, speech_m, discriminator, get_teacher_ratio(args)).to(device)
    if args.optim_type not in ('adam', 'adamw'):
        raise ValueError("optim_type must be adam or adamw")
    return model, RNNFlatAdamW(model, lr=args.lr, weight_decay=args.weight_decay, decoupled=(args.optim_type == 'adamw'))


def optimizer_step(model, optimizer, args):
    """src/train.py:358-363: clip_grad_norm_ -> optimizer.step() -> zero_grad, for RNNFlatAdamW."""
    optimizer.step(max_norm=float(args.grad_clip) if args.grad_clip > 0.0 else 0.0)
    optimizer.zero_grad(set_to_none=True)


# ---- the discriminator batch ----------------------------------------------------------------------------------------------------------------------
def _enc_out(hid):
    """`_, t_out = t_hid` (src/train.py:297-299): an encoder's ((h, c), enc_output) pair, an encoder tape, or enc_output itself."""
    if isinstance(hid, train_rnn.Tape):
        return hid.enc_output
    if isinstance(hid, (tuple, list)):
        return hid[1]
    return hid


def _shuffle(t_hid, t_len, s_hid, s_len, train_discriminator):
    from .utils import lens_i32
    t_out, s_out = _enc_out(t_hid).detach().contiguous(), _enc_out(s_hid).detach().contiguous()
    B, Tt, D = t_out.shape
    if D != ENC_WIDTH:
        raise NotImplementedError("discriminator_shuffle_batch(..., 'rnn'): the RNN family is built at hidden = 256, whose enc_output is %d wide (got %d)"
                                  % (ENC_WIDTH, D))
    if s_out.shape[0] != B or s_out.shape[2] != D:
        raise ValueError("discriminator_shuffle_batch: the two encoder outputs must share batch size and width")
    dev = t_out.device
    perm = torch.arange(2 * B, device=dev) if is_deterministic() else ops.randperm(2 * B, next_seed(), 1, dev)
    d_len = torch.empty(2 * B, dtype=torch.int32, device=dev)
    d_target = torch.empty(2 * B, dtype=_F32, device=dev)
    ops.disc_targets(perm, B, not train_discriminator, d_target)
    d_hid = torch.empty(2 * B, max(Tt, s_out.shape[1]), D, dtype=_F32, device=dev)
    ops.disc_gather(t_out, s_out, lens_i32(t_len, dev), lens_i32(s_len, dev), perm, d_hid, d_len)
    return d_hid, d_len, d_target, perm


@torch.no_grad()
def discriminator_shuffle_batch(t_hid, t_hid_len, s_hid, s_hid_len, train_discriminator=False):
    """src/train.py:296-329 for model_type == 'rnn': (hidden, enc_output) pairs in, (d_hid [2B, max(Tt, Ts), 512], d_len, d_target) out.  Under
    is_deterministic() the permutation is the identity."""
    return _shuffle(t_hid, t_hid_len, s_hid, s_hid_len, train_discriminator)[:3]


_GSCALE = {}


def _gscale(dev, accum_steps):
    """1 / accum_steps as a resident device scalar: the upstream gradient every loss kernel's backward multiplies by."""
    key = (dev, float(accum_steps))
    g = _GSCALE.get(key)
    if g is None:
        g = _GSCALE[key] = torch.full((1,), 1.0 / float(accum_steps), dtype=_F32, device=dev)
    return g


def _discriminator_term(model, te, tl, se, sl, gs, train_discriminator, rec):
    """Gather, discriminator forward, BCE and backward.  Generator phase (train_discriminator False): flipped targets, parameters frozen by the
    caller, returns the loss and the two encoders' d_enc_output shares.  Discriminator phase: unflipped targets, gradients into the
    discriminator's own (the store's 'disc' region), no input gradient."""
    from . import train as T
    d_hid, d_len, d_target, perm = _shuffle(te, tl, se, sl, train_discriminator)
    if not train_discriminator:
        d_hid.requires_grad_(True)
    with torch.enable_grad():
        d_out = model.discriminator(d_hid, d_len)
        d_loss = T.discriminator_loss(d_out, d_target)
        torch.autograd.backward([d_loss], [gs.view(())])
    if rec is not None:
        rec.update(perm=perm, d_len=d_len, d_target=d_target, d_out=d_out.detach())
    if train_discriminator:
        return d_loss.detach(), None, None
    dth, dsh = torch.empty_like(te.enc_output), torch.empty_like(se.enc_output)
    ops.disc_scatter(d_hid.grad.contiguous(), perm, dth, dsh)
    if rec is not None:
        rec.update(d_t_enc=dth, d_s_enc=dsh)
    return d_loss.detach(), dth, dsh


# ---- the sub-steps --------------------------------------------------------------------------------------------------------------------------------
def _process(batch):
    """process_batch (src/train.py:80-94) for the tape entry points: tensors on the device, lengths as host lists as well (the packed
    recurrences and the prefix layout are sized from them on the host)."""
    from . import train as T
    text, mel, text_len, mel_len = batch
    dev = T._dev()
    tl, ml = [int(v) for v in text_len.tolist()], [int(v) for v in mel_len.tolist()]
    text, mel = text.to(dev, non_blocking=True), mel.to(dev, torch.float32, non_blocking=True).contiguous()
    if text.shape[0] < 2:
        raise NotImplementedError("B = 1: TextRNN's decoder normalises B rows with batch statistics at position 0 (the reference raises too)")
    return text, mel, tl, ml, torch.tensor(tl, dtype=torch.int32, device=dev), torch.tensor(ml, dtype=torch.int32, device=dev)


def _check(model, args):
    if not is_rnn_model(model):
        raise TypeError("model must be UNAST(TextRNN, SpeechRNN[, LSTMDiscriminator]) (train.initialize_model with model_type='rnn')")
    if args.use_discriminator and model.discriminator is None:
        raise ValueError("args.use_discriminator is set but the model has no discriminator")
    if not model.training:
        model.train()


def _text_loss(tape, gold, eos_weight, gs):
    """text_loss on the decoder tape's padded head buffer; returns (loss [1], d_logits [B,T,V] view)."""
    from . import train as T
    P, B, Tn = tape.P, tape.B, tape.T
    head = tape.head
    dev = head.device
    ws, loss = T._loss_ws(dev), torch.empty(1, dtype=_F32, device=dev)
    gold = gold.contiguous().view(-1)
    ops.text_loss_fwd(head, gold, P.V, float(eos_weight), ws, loss)
    dl = torch.empty_like(head)
    ops.text_loss_bwd(head, gold, P.V, float(eos_weight), ws, gs, dl)
    return loss, dl.view(B, Tn, P.ldh)[:, :, :P.V]


def _speech_loss(tape, gold, lens_i32, eos_weight, gs):
    """speech_loss on the decoder tape's [pre | stop] head buffer and post-net output; returns (loss [1], d_pre, d_post, d_stop)."""
    from . import train as T
    P, B, Tn = tape.P, tape.B, tape.T
    head, post = tape.head, tape.post.contiguous()
    dev = head.device
    ws, loss = T._loss_ws(dev), torch.empty(1, dtype=_F32, device=dev)
    ops.speech_loss_fwd(gold, head, post, lens_i32, float(eos_weight), ws, loss)
    dh, dp = torch.empty_like(head), torch.empty_like(post)
    ops.speech_loss_bwd(gold, head, post, lens_i32, float(eos_weight), gs, dh, dp)
    return loss, dh[:, :, :P.M], dp, dh[:, :, P.M]


def _generator_substep(losses, keys, model, args, accum_steps, text, mel, ml_dev, tl_dev, te, se, td, sd, td_mem, sd_mem, enc_lens=None):
    """What the generator sub-steps share once their four tapes exist: the losses, the discriminator term on the two encoder outputs, and
    the backward.  te / se: the text / speech encoder tapes; td / sd: the text / speech decoder tapes; td_mem / sd_mem: the encoder tape each
    decoder attended to, which receives its cotangents.  enc_lens (the cross-model step): the (text, speech) lengths of what the two encoders
    read -- the generated sequences' -- where they differ from the targets' tl_dev / ml_dev."""
    from . import train as T
    dev = text.device
    gs = _gscale(dev, accum_steps)
    rec = model.__dict__.setdefault("_rnn_step_record", {}) if RECORD else None
    if rec is not None:
        rec.clear()
        rec.update(tapes=dict(text_enc=te, speech_enc=se, text_dec=td, speech_dec=sd))
    t_loss, d_logits = _text_loss(td, text, args.t_eos_weight, gs)
    s_loss, d_pre, d_post, d_stop = _speech_loss(sd, mel, ml_dev, args.s_eos_weight, gs)
    parts = [t_loss, s_loss]
    dth = dsh = None
    if args.use_discriminator:
        d_tl, d_sl = enc_lens if enc_lens is not None else (tl_dev, ml_dev)
        d_loss, dth, dsh = _discriminator_term(model, te, d_tl, se, d_sl, gs, False, rec)
        parts.append(d_loss.view(1))
    cots = {id(td_mem): train_rnn.text_decoder_backward(td, d_logits, accumulate=True),
            id(sd_mem): train_rnn.decoder_backward(sd, d_pre, d_post, d_stop, accumulate=True)}
    for enc, extra in ((te, dth), (se, dsh)):
        d_enc, d_h, d_c = cots[id(enc)]
        if extra is not None:
            ops.add_inplace(d_enc, extra)                  # the encoder's cotangent = its decoder's + the discriminator's
        train_rnn.encoder_backward(enc, d_enc, d_h, d_c, accumulate=True)
    _touched(model).update(GEN_SEGMENTS)
    out = torch.empty((), dtype=_F32, device=dev)
    ops.scalar_combine([p.view(()) for p in parts], float(accum_steps), out)
    for k, v in zip(keys, parts):
        losses[k].append(T._log(v.view(())))
    return out


def train_ae_step(losses, model, batch, step, accum_steps, args):
    """src/train.py:392-416 with autoencoder_step (199-229): text and speech auto-encoders on noised inputs, the discriminator term on the two
    encoder outputs.  Returns the sub-step's loss / accum_steps (a device scalar)."""
    _check(model, args)
    text, mel, tl, ml, tl_dev, ml_dev = _process(batch)
    tm, sm = model.text_m, model.speech_m
    noise = not is_deterministic()                                                              # (noise_fn does not look at model.training)
    with torch.no_grad():
        te = train_rnn.encoder_forward(tm, text, tl, noise_in=noise, seed=next_seed())
        td = train_rnn.text_decoder_forward(tm, text, te, tl, seed=next_seed())
        se = train_rnn.encoder_forward(sm, mel, ml, noise_in=noise, seed=next_seed())
        sd = train_rnn.decoder_forward(sm, mel, se, ml, seed=next_seed())
        return _generator_substep(losses, ('t_ae', 's_ae', 'd_ae'), model, args, accum_steps, text, mel, ml_dev, tl_dev, te, se, td, sd, te, se)


def train_sp_step(losses, model, batch, step, accum_steps, args):
    """src/train.py:365-390 with supervised_step (231-259): TTS (text encoder -> speech decoder) and ASR (speech encoder on specaugment(mel) ->
    text decoder), the discriminator term on the two encoder outputs.  losses: 'asr_', 'tts_', 'sp_d'."""
    _check(model, args)
    text, mel, tl, ml, tl_dev, ml_dev = _process(batch)
    tm, sm = model.text_m, model.speech_m
    with torch.no_grad():
        mel_aug = mel if is_deterministic() else specaugment(mel, ml_dev)
        te = train_rnn.encoder_forward(tm, text, tl, seed=next_seed())
        sd = train_rnn.decoder_forward(sm, mel, te, tl, seed=next_seed())
        se = train_rnn.encoder_forward(sm, mel_aug, ml, seed=next_seed())
        td = train_rnn.text_decoder_forward(tm, text, se, ml, seed=next_seed())
        out = _generator_substep(losses, ('asr_', 'tts_', 'sp_d'), model, args, accum_steps, text, mel, ml_dev, tl_dev, te, se, td, sd, se, te)
        if RECORD:
            model._rnn_step_record["mel_aug"] = mel_aug
        return out


def train_discriminator_step(losses, model, batch, step, accum_steps, args, log_out_to_tb=False):
    """src/train.py:446-463 with discriminator_step (337-354): both encoders in TRAIN mode without backward (the reference's no_grad: dropout
    on, BatchNorm on batch statistics, running statistics updated), unflipped targets, the discriminator forward and backward into its own
    gradients.  No generator gradient is produced."""
    _check(model, args)
    if model.discriminator is None:
        raise ValueError("train_discriminator_step: the model has no discriminator")
    text, mel, tl, ml, tl_dev, ml_dev = _process(batch)
    from . import train as T
    with torch.no_grad():
        te = train_rnn.encoder_forward(model.text_m, text, tl, seed=next_seed())
        se = train_rnn.encoder_forward(model.speech_m, mel, ml, seed=next_seed())
        rec = model.__dict__.setdefault("_rnn_step_record", {}) if RECORD else None
        if rec is not None:
            rec.clear()
            rec.update(tapes=dict(text_enc=te, speech_enc=se))
        d_loss, _, _ = _discriminator_term(model, te, tl_dev, se, ml_dev, _gscale(text.device, accum_steps), True, rec)
        out = torch.empty((), dtype=_F32, device=text.device)
        ops.scalar_combine([d_loss.view(())], float(accum_steps), out)
    losses['d'].append(T._log(d_loss.view(())))
    return out


# ---- the cross-model (back-translation) sub-step and the step that includes it; DESIGN 5m ----------------------------------------------------------
TEXT_MAX_LEN, SPEECH_MAX_LEN = 300, 815                    # infer_sequence's defaults (src/network.py:312, 586): what cm_speech_in / cm_text_in generate with


def train_cm_step(losses, model, batch, step, accum_steps, args):
    """src/train.py:418-444 with crossmodel_step (261-294) and UNAST.cm_speech_in / cm_text_in (src/network.py:103-123), speech-in first:
      speech-in: speech encoder (train mode, no noise) -> greedy text generation in train mode, both without backward; then the text encoder on
                 the generated tokens -> the teacher-forced speech decoder -> speech_loss ('s_cm');
      text-in:   text encoder -> greedy speech generation in train mode, without backward; then the speech encoder on the generated post-net
                 frames -> the teacher-forced text decoder -> text_loss ('t_cm');
    and the discriminator term ('d_cm', frozen discriminator, flipped targets) on the two re-encoded outputs with the generated lengths.
    Gradients stop at the generated sequences.  A generated PAD id inside a sequence's length stays an attention key here (the kernels mask by
    length; the reference masks text.eq(PAD)): model._rnn_cm_live_pad counts them for the last call."""
    _check(model, args)
    text, mel, tl, ml, tl_dev, ml_dev = _process(batch)
    tm, sm = model.text_m, model.speech_m
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=text.device)                      # noqa: E731
    with torch.no_grad():
        seeds = [next_seed() for _ in range(8)]
        s_mem = train_rnn.encoder_forward(sm, mel, ml, seed=seeds[0])
        gen_t = train_rnn.text_generate_train(tm, s_mem, ml, max_len=TEXT_MAX_LEN, seed=seeds[1])
        te = train_rnn.encoder_forward(tm, gen_t[0], gen_t.lens_host, seed=seeds[2])
        sd = train_rnn.decoder_forward(sm, mel, te, gen_t.lens_host, seed=seeds[3])
        t_mem = train_rnn.encoder_forward(tm, text, tl, seed=seeds[4])
        gen_s = train_rnn.speech_generate_train(sm, t_mem, tl, max_len=SPEECH_MAX_LEN, seed=seeds[5])
        se = train_rnn.encoder_forward(sm, gen_s[1], gen_s.lens_host, seed=seeds[6])
        td = train_rnn.text_decoder_forward(tm, text, se, gen_s.lens_host, seed=seeds[7])
        model.__dict__["_rnn_cm_live_pad"] = gen_t.live_pad
        out = _generator_substep(losses, ('t_cm', 's_cm', 'd_cm'), model, args, accum_steps, text, mel, ml_dev, tl_dev, te, se, td, sd, se, te,
                                 enc_lens=(i32(gen_t.lens_host), i32(gen_s.lens_host)))
        if RECORD:
            model._rnn_step_record.update(gen_text=gen_t, gen_speech=gen_s, seeds=seeds, live_pad=gen_t.live_pad, mem_tapes=dict(speech_mem=s_mem, text_mem=t_mem))
        return out


def train_step(losses, model, optimizer, scheduler, batches, step, args):
    """One iteration of train()'s hot loop (src/train.py:602-655) for model_type == 'rnn' with cm_steps >= 0, as unast_amd.train.train_step runs it
    with cm_steps = 0: the discriminator frozen, ae_steps AE sub-steps on batches['unsup'], cm_steps cross-model sub-steps on batches['cm'],
    sp_steps supervised sub-steps on batches['sup'] (every gradient scaled by 1 / their number), optimizer_step; then the discriminator
    unfrozen, d_steps discriminator sub-steps on batches['disc'] and its optimizer_step.  Eager, on the current stream."""
    # (the body of unast_amd.train.train_step's RNN branch plus the cm sub-steps: the two merge when train's dispatch stops refusing cm_steps > 0)
    from . import train as T
    _check(model, args)
    cm_steps = getattr(args, "cm_steps", 0)
    if args.use_discriminator:
        T.freeze_model_parameters(model.discriminator)
    accum_steps = args.ae_steps + cm_steps + args.sp_steps
    subs = [(train_ae_step, batches["unsup"][si]) for si in range(args.ae_steps)]
    subs += [(train_cm_step, batches["cm"][si]) for si in range(cm_steps)]
    subs += [(train_sp_step, batches["sup"][si]) for si in range(args.sp_steps)]
    for fn, b in subs:
        fn(losses, model, b, step, accum_steps, args)
    optimizer_step(model, optimizer, args)
    if args.use_discriminator:
        T.unfreeze_model_parameters(model.discriminator)
        for si in range(args.d_steps):
            train_discriminator_step(losses, model, batches["disc"][si], step, args.d_steps, args)
        optimizer_step(model, optimizer, args)
    if scheduler is not None:
        scheduler.step()
