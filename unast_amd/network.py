"""UNAST task graph, transformer autoencoders and discriminators with the reference's API (src/network.py), executed
by hand-written HIP kernels.

Public surface kept:
  UNAST(text_m, speech_m, discriminator=None, teacher=None): text_ae, speech_ae, tts, asr, num_params
  TextTransformer / SpeechTransformer(args): encode, decode_sequence, forward, preprocess
  TextRNN / SpeechRNN(args): encode, decode, decode_sequence, infer_sequence, postprocess, forward -- eval mode under torch.no_grad() at the
      full-size RNN configuration only (unast_amd.rnn; src/network.py:279-402, 503-624); they train through unast_amd.train_rnn's tape entry
      points, composed into the train step by unast_amd.train_rnn_step
  LSTMDiscriminator(d_in, hidden, out=1, bidirectional=False, num_layers=1, dropout=.2, relu=.2).forward(out, out_len)
  Discriminator(enc_dim, hidden=1024, out_classes=1, dropout=.2, relu=.2).forward(enc_output)
  Vocoder(num_mels, hidden_size, num_fft).forward(mel) -- eval mode under torch.no_grad() only (unast_amd.vocoder) -- and make_mags;
  its training step vocoder_step / valid_loss / FlatAdamW / vocoder_train_step (unast_amd.train_vocoder; src/train_vocoder.py:85-100)
`state_dict()` keys/shapes equal the reference's (unast_amd.spec).  The `masks` tuple returned by encode() is opaque
to callers in the reference (only passed back into decode_sequence); here it carries int32 lengths instead of bool
mask tensors — the kernels test `t < len[b]` themselves (no B x T host loop, cf. src/utils.py:77-83).
"""
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import functional as F
from . import ops
from .engine import Var, acc, run_segment, FlatStore, on_stream, ddp_hook
from .module import (SpeechPrenet, SpeechPostnet, TextPrenet, TextPostnet, PositionalEncoding, TransformerEncoder,
                     TransformerDecoder, RNNEncoder, RNNDecoder)
from .spec import state_dict_spec  # noqa: F401  (re-export)
from .utils import PAD_IDX, SOS_IDX, EOS_IDX, lens_i32, next_seed  # noqa: F401
from .vocoder import Vocoder, make_mags  # noqa: F401  (src/network.py:627-655, src/inf_vocoder.py:56-64; eval forward only)
from .train_vocoder import FlatAdamW, train_step as vocoder_train_step, valid_loss, vocoder_step  # noqa: F401,E402  (src/train_vocoder.py:85-100, 135-136)

_HP_KEYS = ("num_mels", "s_pre_hid", "s_pre_drop", "s_post_drop", "t_emb_dim", "t_pre_drop", "t_post_drop", "hidden", "e_in",
            "e_drop", "d_drop", "num_layers", "nhead", "ffn_dim")


def _hp(args):
    hp = SimpleNamespace(**{k: getattr(args, k) for k in _HP_KEYS if hasattr(args, k)})
    if hp.hidden != hp.e_in:
        raise ValueError("hidden must equal e_in (the heads read the decoder output; src/network.py:196 vs src/module.py:152-153)")
    return hp


def _as_padded(t, rows, ld, cols):
    """Recover (or build) the [rows, ld] padded buffer behind a [..., cols] view; device-memory plumbing only."""
    if t is None:
        return None
    if t.dim() >= 2 and t.stride(-1) == 1 and t.stride(-2) == ld and t.storage_offset() % 4 == 0 and \
            t.untyped_storage().nbytes() // 4 >= t.storage_offset() + rows * ld:
        lead = t.shape[:-1].numel()
        if lead == rows and (t.dim() == 2 or t.stride(0) == t.shape[1] * ld):
            return t.as_strided((rows, ld), (ld, 1))
    buf = torch.zeros(rows, ld, dtype=torch.float32, device=t.device)
    buf[:, :cols].copy_(t.reshape(rows, cols))
    return buf


class _Side(nn.Module):
    """Shared plumbing of TextTransformer / SpeechTransformer / LSTMDiscriminator: canonical name prefix, parameter
    store lookup (the enclosing UNAST's store when wrapped), BN buffers by canonical name."""
    _prefix = ""

    def _root(self):
        r = self.__dict__.get("_unast_root")
        return r() if r is not None else None

    def _store(self):
        root = self._root()
        if root is not None:
            return root._store()
        st = self.__dict__.get("_unast_store")
        dev = next(self.parameters()).device
        if st is None or st.device != dev:
            st = FlatStore(self, prefix=self._prefix)
            self.__dict__["_unast_store"] = st
        return st

    @property
    def buffers_dict(self):
        d = self.__dict__.get("_bufs")
        dev = next(self.parameters()).device
        if d is None or d["__dev"] != dev:
            d = {self._prefix + n: b for n, b in self.named_buffers()}
            d["__dev"] = dev
            self.__dict__["_bufs"] = d
        return d

    def _ctx(self):
        return F.Ctx(self._store(), self.training, next_seed())


class AutoEncoderNet(_Side):
    """src/network.py:12-86 (abstract interface), and what the text and the speech transformer share here: one n-ary code path for their
    encoder and decoder calls (n = 1: encode / decode_sequence; n = 2: encode_pair / decode_pair).  Subclasses name their side (`_side`),
    their functional.*_encode / *_decode (`_f_encode`, `_f_decode`) and turn a decoder call's result into output Vars (`_dec_outputs`)."""

    def preprocess(self, input_, input_lens):
        raise Exception("Please use a subclass for text or speech")

    def _encode_n(self, calls):
        """calls: [(input_, input_lens, noise_in)] of ONE shape: the front ends per call (BatchNorm statistics and running-stat updates in
        call order, as separate calls would make them), the encoder stack once over all.  Returns [(enc_outputs, masks)] per call."""
        n = len(calls)
        if any(c[0].shape != calls[0][0].shape for c in calls):
            raise ValueError("encode_pair: the two batches must have one shape")
        B, T = calls[0][0].shape[:2]
        lens = [lens_i32(c[1], c[0].device) for c in calls]
        lens_all = lens[0] if n == 1 else torch.cat(lens)       # (one call: its length vector as it is, no copy launch)
        cx = self._ctx()
        ins = [c[0].detach().contiguous() for c in calls]
        noises = [c[2] for c in calls]

        def run(tape, dummy):
            y = self._f_encode(cx, tape, self, ins, noises, lens_all)
            if n == 2:
                return _pair_outputs(tape, y, B, T)
            o = _out3d(tape, y, B, T)
            return [o, _alias(tape, o)]
        outs = run_segment(run, ddp_hook(self._side + "_enc", cx.st), cx.st.dummy)
        return [(outs[2 * i], (None, lens[i], outs[2 * i + 1])) for i in range(n)]

    def _decode_n(self, calls):
        """calls: [(tgt, tgt_lens, enc_outputs, masks, loss_hint)] with the targets in ONE shape: the decoder stack once over all
        (self-attention and feed-forward over n B sequences, cross-attention per call on its own memory), front ends, heads and loss terms per
        call.  Returns the calls' output tensors in call order, as run_segment gives them."""
        n = len(calls)
        if any(c[0].shape != calls[0][0].shape for c in calls):
            raise ValueError("decode_pair: the two targets must have one shape")
        B, T = calls[0][0].shape[:2]
        Tks = [c[2].shape[1] for c in calls]
        lq = [lens_i32(c[1], c[0].device) for c in calls]
        lens_q = lq[0] if n == 1 else torch.cat(lq)
        lens_ks = [c[3][1] for c in calls]
        cx = self._ctx()
        tgts = [c[0].detach().contiguous() for c in calls]
        hints = [c[4] for c in calls]

        def run(tape, dummy, *mem_in):
            mems = [_mem_in(tape, mem, B, Tk) for mem, Tk in zip(mem_in, Tks)]
            res = []
            for out in self._f_decode(cx, tape, self, tgts, lens_q, mems, lens_ks, Tks, loss_hints=hints):
                res += self._dec_outputs(tape, out, B, T)
            return res
        return run_segment(run, ddp_hook(self._side + "_dec", cx.st), cx.st.dummy, *[c[2] for c in calls])


def _lens_of_pad_mask(mask, T, device):
    """Lengths behind a key-padding mask.  The kernels mask by length, so a bool mask [B,T] (True = padded; the reference's form,
    src/network.py:411-413) must be a suffix mask, which is all the reference ever builds; int lengths (this package's masks[1])
    pass through; None = nothing padded."""
    if mask is None:
        raise ValueError("pass the key-padding mask (bool [B,T]) or the lengths (int [B])")
    if mask.dtype != torch.bool:
        return lens_i32(mask, device)
    if mask.shape[1] > 1 and bool((mask[:, 1:] < mask[:, :-1]).any()):
        raise ValueError("key-padding masks must pad a suffix of each sequence (lengths are what the attention kernels take)")
    return (T - mask.sum(dim=1)).to(device=device, dtype=torch.int32)


def _out3d(tape, var2d, B, T):
    """Expose a [B*T, C] Var as a [B, T, C] output Var (a view; its gradient flows back as a view)."""
    o = Var(var2d.v.view(B, T, var2d.v.shape[1]))
    if tape is not None:
        def bwd():
            if o.g is not None:
                acc(var2d, (o.g if o.g.is_contiguous() else o.g.contiguous()).view(B * T, -1))
        tape.record(bwd)
    return o


def _pair_outputs(tape, var2d, B, T):
    """The two row blocks of a [2 B T, C] Var (a paired encoder call's stack output) as [B, T, C] output Vars, each twice: the value and
    a second alias of it for its second consumer (see _alias: the decoder and the discriminator both read an encoder output, on two
    streams).  The four gradients arrive separately; the stack's backward wants one buffer: each block = value gradient + alias gradient,
    summed straight into its rows by one kernel per block (no memcpy node in a captured step, no separate accumulate pass)."""
    N, C = B * T, var2d.v.shape[1]
    outs = []
    for i in range(2):
        blk = var2d.v[i * N:(i + 1) * N].view(B, T, C)
        outs += [Var(blk), Var(blk.view(B, T, C))]
    if tape is not None:
        def bwd():
            if all(o.g is None for o in outs):
                return
            g = torch.empty_like(var2d.v)
            for i in range(2):
                parts = [o.g if o.g.is_contiguous() else o.g.contiguous() for o in outs[2 * i:2 * i + 2] if o.g is not None]
                dst = g[i * N:(i + 1) * N]
                if not parts:
                    dst.zero_()
                else:
                    ops.sum2(dst, parts[0], parts[1] if len(parts) > 1 else None)
            acc(var2d, g)
        tape.record(bwd)
    return outs


def _alias(tape, var):
    """A second output of the same activation (a view) for a second consumer.  Each of the two then has exactly one user in
    torch's autograd graph and THIS call's backward adds the two incoming gradients itself (on its own stream, after autograd
    has ordered it behind both producers).  Letting autograd sum gradients that arrive from different streams in a node's
    input buffer works eagerly but takes hipStreamEndCapture down when the step is captured into a HIP graph (ROCm 7.2;
    the round-2 capture probe, cases aedisc_* vs discdetach_ms, in the git history), and the encoder output has two users on two streams: the
    decoder (cross-attention memory) and the discriminator."""
    o = Var(var.v.view(var.v.shape))
    if tape is not None:
        def bwd():
            if o.g is not None:
                acc(var, o.g if o.g.is_contiguous() else o.g.contiguous())
        tape.record(bwd)                                   # recorded after var's own closure => runs before it
    return o


def _mem_in(tape, mem, B, Tk):
    """[B,Tk,E] input Var -> [B*Tk,E] Var; its closure (recorded first => runs last) hands the gradient back."""
    memv = Var(mem.v.contiguous().view(B * Tk, -1))
    if tape is not None:
        tape.record(lambda: setattr(mem, "g", None if memv.g is None else memv.g.view(B, Tk, -1)))
    return memv


def _speech_outputs(tape, head, post, B, T, M, device):
    """(pre, post, stop) output Vars of a speech decoder call over its head buffer [B T, ldh] and post-net output [B T, M]; their closure
    (recorded last => runs first) turns the three incoming gradients back into d(head) and d(post)."""
    ldh = head.v.shape[1]
    h3 = head.v.view(B, T, ldh)
    o_pre, o_post, o_stop = Var(h3[..., :M]), Var(post.v.view(B, T, M)), Var(h3[..., M])
    if tape is not None:
        def bwd():
            if o_post.g is not None:
                post.g = (o_post.g if o_post.g.is_contiguous() else o_post.g.contiguous()).view(B * T, M)
            gp, gs = o_pre.g, o_stop.g
            if gp is None and gs is None:
                return
            if gp is not None and gs is not None and gp.stride(-1) == 1 and gp.stride(-2) == ldh and \
                    gs.data_ptr() == gp.data_ptr() + 4 * M and gs.stride(-1) == ldh:
                head.g = gp.as_strided((B * T, ldh), (ldh, 1))          # both are views of one d_head buffer
            else:
                buf = torch.zeros(B * T, ldh, dtype=torch.float32, device=device)
                if gp is not None:
                    buf[:, :M].copy_(gp.reshape(B * T, M))
                if gs is not None:
                    buf[:, M].copy_(gs.reshape(B * T))
                head.g = buf
        tape.record(bwd)
    return [o_pre, o_post, o_stop]


class TextTransformer(AutoEncoderNet):
    """src/network.py:417-500."""
    _prefix = "text_m."

    def __init__(self, args):
        super().__init__()
        if args.t_emb_dim != args.e_in:
            raise ValueError("t_emb_dim must equal e_in (decoder input skips the conv prenet; src/network.py:435-438)")
        self.prenet = TextPrenet(args.t_emb_dim, args.e_in, p=args.t_pre_drop)
        self.pos_emb = PositionalEncoding(args.e_in)
        self.encoder = TransformerEncoder(args.e_in, args.nhead, args.ffn_dim, args.e_drop, args.num_layers)
        self.decoder = TransformerDecoder(args.e_in, args.nhead, args.ffn_dim, args.d_drop, args.num_layers)
        self.postnet = TextPostnet(args.hidden, args.t_post_drop)
        self.args = _hp(args)

    @property
    def pe(self):
        return self.pos_emb.pe[0]

    _side, _f_encode, _f_decode = "text", staticmethod(F.text_encode), staticmethod(F.text_decode)

    @on_stream("text")
    def encode(self, input_, input_lens, noise_in=False):
        return self._encode_n([(input_, input_lens, noise_in)])[0]

    @on_stream("text")
    def encode_pair(self, in_a, lens_a, noise_a, in_b, lens_b, noise_b):
        """encode(in_a, lens_a, noise_a) and encode(in_b, lens_b, noise_b) of two batches of ONE shape as a single call (_encode_n).
        Returns the two (enc_outputs, masks) pairs of the separate calls."""
        return tuple(self._encode_n([(in_a, lens_a, noise_a), (in_b, lens_b, noise_b)]))

    def _dec_outputs(self, tape, out, B, T):
        """The logits output Var [B, T, V] over a call's padded logits buffer."""
        V = self.postnet.fc1.weight.shape[0]
        ldl = out.v.shape[1]
        o = Var(out.v.view(B, T, ldl)[..., :V])
        if tape is not None:
            def bwd():
                if o.g is not None:
                    out.g = _as_padded(o.g, B * T, ldl, V)
            tape.record(bwd)                                                    # recorded last => runs first
        return [o]

    @on_stream("text")
    def decode_sequence(self, tgt, tgt_lens, enc_outputs, masks, teacher_ratio=1, loss_hint=None):
        """loss_hint (not in the reference's signature; unast_amd.train passes it): (gold, eos_weight, gscale, workspace) of the text_loss call
        that will follow on this call's logits -- the head GEMM then computes that loss and its gradient in the same launch."""
        return self._decode_n([(tgt, tgt_lens, enc_outputs, masks, loss_hint)])

    @on_stream("text")
    def decode_pair(self, tgt_a, lens_a, enc_a, masks_a, hint_a, tgt_b, lens_b, enc_b, masks_b, hint_b):
        """Two decode_sequence calls of one target shape as a single call (_decode_n).  Returns the two logits tensors."""
        return self._decode_n([(tgt_a, lens_a, enc_a, masks_a, hint_a), (tgt_b, lens_b, enc_b, masks_b, hint_b)])

    @on_stream("text")
    def decode(self, tgt, tgt_lens, tgt_pad_mask, enc_outputs, enc_mask):
        """src/network.py:446-450: one uncached generation step -- the decoder over all of `tgt` (token ids [B,T], fed as they are),
        logits [B,1,V] of its last position.  Forward only (no tape); generation proper runs on the K/V cache (infer_sequence)."""
        B, T = tgt.shape
        Tk = enc_outputs.shape[1]
        lens_q = _lens_of_pad_mask(tgt_pad_mask, T, tgt.device)
        lens_k = _lens_of_pad_mask(enc_mask, Tk, tgt.device)
        cx = self._ctx()
        with torch.no_grad():
            out, = F.text_decode(cx, None, self, [tgt.contiguous()], lens_q, [Var(enc_outputs.detach().contiguous().view(B * Tk, -1))], [lens_k], [Tk], shift=False)
        V = self.postnet.fc1.weight.shape[0]
        return out.v.view(B, T, -1)[:, -1:, :V]

    @on_stream("text")
    def postprocess(self, out):
        """src/network.py:452-453: TextPostnet on decoder states [B,T,E] -> logits [B,T,V].  Forward only (the train step's post-net is
        part of decode_sequence's segment)."""
        with torch.no_grad():
            return F.text_postnet(self._ctx(), self, out.detach())

    def forward(self, text, text_len, noise_in=False, teacher_ratio=1, ret_enc_hid=False):
        enc_outputs, masks = self.encode(text, text_len, noise_in)
        dec_out = self.decode_sequence(text, text_len, enc_outputs, masks)
        if ret_enc_hid:
            return dec_out, masks[2]                       # the encoder output once more, for its second user (see _alias)
        return dec_out

    def infer_sequence(self, memory, masks, max_len=300):
        """src/network.py:455-481 with a K/V cache (unast_amd.inference).  Returns (tokens [B,T], stop_lens [B])."""
        return self.generation(memory, masks, max_len).run()

    infer_max_len = 300      # the cap the cross-model paths generate with (= infer_sequence's default)

    def generation(self, memory, masks, max_len=None):
        """infer_sequence as a resumable unast_amd.inference._Generation (lets UNAST.cm_both_in run two of them in lock-step)."""
        max_len = max_len or self.infer_max_len
        from .inference import text_generation
        return text_generation(self, self._ctx(), memory.detach(), masks[1], max_len)


class SpeechTransformer(AutoEncoderNet):
    """src/network.py:188-276."""
    _prefix = "speech_m."

    def __init__(self, args):
        super().__init__()
        self.prenet = SpeechPrenet(args.num_mels, args.s_pre_hid, args.e_in, p=args.s_pre_drop)
        self.pos_emb = PositionalEncoding(args.e_in)
        self.encoder = TransformerEncoder(args.e_in, args.nhead, args.ffn_dim, args.e_drop, args.num_layers)
        self.decoder = TransformerDecoder(args.e_in, args.nhead, args.ffn_dim, args.d_drop, args.num_layers)
        self.postnet = SpeechPostnet(args.num_mels, args.hidden, p=args.s_post_drop)
        self.args = _hp(args)

    @property
    def pe(self):
        return self.pos_emb.pe[0]

    _side, _f_encode, _f_decode = "speech", staticmethod(F.speech_encode), staticmethod(F.speech_decode)

    @on_stream("speech")
    def encode(self, input_, input_lens, noise_in=False):
        return self._encode_n([(input_, input_lens, noise_in)])[0]

    @on_stream("speech")
    def encode_pair(self, in_a, lens_a, noise_a, in_b, lens_b, noise_b):
        """Two encode calls of one shape as one (see TextTransformer.encode_pair)."""
        return tuple(self._encode_n([(in_a, lens_a, noise_a), (in_b, lens_b, noise_b)]))

    def _dec_outputs(self, tape, out, B, T):
        head, post = out
        return _speech_outputs(tape, head, post, B, T, post.v.shape[1], head.v.device)

    @on_stream("speech")
    def decode_sequence(self, tgt, tgt_lens, enc_outputs, masks, teacher_ratio=1, loss_hint=None):
        """loss_hint (not in the reference's signature): (gold mel, lengths, eos_weight, gscale, workspace) of the speech_loss call that will
        follow on this call's outputs -- the head GEMM then computes the pre-net and stop terms and their gradient in the same launch."""
        pre, post, stop = self._decode_n([(tgt, tgt_lens, enc_outputs, masks, loss_hint)])
        return pre, post, stop, tgt_lens

    @on_stream("speech")
    def decode_pair(self, tgt_a, lens_a, enc_a, masks_a, hint_a, tgt_b, lens_b, enc_b, masks_b, hint_b):
        """decode_sequence(tgt_a, lens_a, enc_a, masks_a) and decode_sequence(tgt_b, lens_b, enc_b, masks_b) of two targets of ONE shape as
        a single call (_decode_n; the post-net's BatchNorm statistics: first a, then b).  Returns the two (pre, post, stop, lens) tuples of
        the separate calls."""
        pa, qa, sa, pb, qb, sb = self._decode_n([(tgt_a, lens_a, enc_a, masks_a, hint_a), (tgt_b, lens_b, enc_b, masks_b, hint_b)])
        return (pa, qa, sa, lens_a), (pb, qb, sb, lens_b)

    @on_stream("speech")
    def decode(self, tgt, tgt_lens, tgt_pad_mask, enc_outputs, enc_mask):
        """src/network.py:210-214: one uncached generation step -- the decoder over all of `tgt` ([B,T,M] frames, fed as they are),
        (mel [B,1,M], stop logit [B,1,1]) of its last position.  Forward only; generation proper runs on the K/V cache."""
        B, T, M = tgt.shape
        Tk = enc_outputs.shape[1]
        lens_q = _lens_of_pad_mask(tgt_pad_mask, T, tgt.device)
        lens_k = _lens_of_pad_mask(enc_mask, Tk, tgt.device)
        cx = self._ctx()
        with torch.no_grad():
            (head, _), = F.speech_decode(cx, None, self, [tgt.detach()], lens_q, [Var(enc_outputs.detach().contiguous().view(B * Tk, -1))], [lens_k], [Tk],
                                         shift=False, postnet=False)
        h = head.v.view(B, T, -1)[:, -1:, :]
        return h[..., :M], h[..., M:M + 1]

    @on_stream("speech")
    def postprocess(self, out):
        """src/network.py:216-217: SpeechPostnet on [B,T,M] frames (the residual term; callers add it to `out`).  Forward only."""
        with torch.no_grad():
            return F.speech_postnet_residual(self._ctx(), self, out.detach().contiguous(), residual=False)

    def forward(self, mel, mel_len, noise_in=False, teacher_ratio=1, ret_enc_hid=False):
        enc_outputs, masks = self.encode(mel, mel_len, noise_in)
        pre_pred, post_pred, stop_pred, stop_lens = self.decode_sequence(mel, mel_len, enc_outputs, masks)
        if ret_enc_hid:
            return pre_pred, post_pred, stop_pred, masks[2]
        return pre_pred, post_pred, stop_pred

    def infer_sequence(self, memory, masks, max_len=815):
        """src/network.py:219-252 with a K/V cache.  Returns (pre [B,T,M], post [B,T,M], stop [B,T], stop_lens [B])."""
        return self.generation(memory, masks, max_len).run()

    infer_max_len = 815

    def generation(self, memory, masks, max_len=None):
        max_len = max_len or self.infer_max_len
        from .inference import speech_generation
        return speech_generation(self, self._ctx(), memory.detach(), masks[1], max_len,
                                 lambda cx, fr, pos: F.speech_prenet_step(cx, self, fr, pos), lambda cx, mel: F.speech_postnet_residual(cx, self, mel))


_RNN_BUILT = ("the RNN family is built for eval mode under torch.no_grad() at hidden = e_in = t_emb_dim = s_pre_hid = 256, num_layers = 2, "
              "e_bi = True, d_attn 'luong' or 'lsa', attn_dim a multiple of 4 up to 64, num_mels a multiple of 4, teacher_ratio = 1, noise_in = False")


def _rnn_check_args(args):
    bad = [k for k in ("hidden", "e_in", "t_emb_dim", "s_pre_hid") if getattr(args, k) != 256]
    if bad or args.num_layers != 2 or not args.e_bi or args.d_attn not in ("luong", "lsa") or args.attn_dim % 4 or not 4 <= args.attn_dim <= 64 \
            or args.num_mels % 4 or args.num_mels <= 0:
        raise NotImplementedError("%s (got hidden=%r e_in=%r t_emb_dim=%r s_pre_hid=%r num_layers=%r e_bi=%r d_attn=%r attn_dim=%r num_mels=%r)" % (
            _RNN_BUILT, args.hidden, args.e_in, args.t_emb_dim, args.s_pre_hid, args.num_layers, args.e_bi, args.d_attn, args.attn_dim, args.num_mels))


class _RNNModel(AutoEncoderNet):
    """What TextRNN and SpeechRNN share (src/network.py:279-402, 503-624): the eval-path checks, the RNN encoder behind their front ends, and
    the reference's data structures: encode returns ((h, c), enc_output), pad_mask with h, c [2,B,256], enc_output [B,T,512] and pad_mask
    bool [B,T] (True = padded); the decoders take that pair and a pad mask (or int lengths) back."""

    def _init_rnn(self, args):
        _rnn_check_args(args)
        self.encoder = RNNEncoder(args.e_in, args.hidden, dropout=args.e_drop, num_layers=args.num_layers, bidirectional=args.e_bi)
        self.decoder = RNNDecoder(args.e_in, args.hidden * self.encoder.num_dir, args.hidden, dropout=args.d_drop, num_layers=args.num_layers,
                                  attention=args.d_attn, attn_dim=args.attn_dim)

    def _check_call(self, noise_in=False, teacher_ratio=1):
        if self.training:
            raise NotImplementedError("train() mode: " + _RNN_BUILT + "; call model.eval()")
        if torch.is_grad_enabled():
            raise NotImplementedError("a call with autograd enabled: " + _RNN_BUILT)
        if noise_in:
            raise NotImplementedError("noise_in=True is a training-time corruption: " + _RNN_BUILT)
        if teacher_ratio != 1:
            raise NotImplementedError("teacher_ratio=%r: %s" % (teacher_ratio, _RNN_BUILT))

    def _pack(self, noise_in=False, teacher_ratio=1):
        self._check_call(noise_in, teacher_ratio)
        if next(self.parameters()).device.type != "cuda":
            raise RuntimeError("unast_amd runs on the GPU only: move the model to a CUDA (ROCm) device first; there is no CPU path")
        from . import rnn
        return rnn.pack_of(self, self._side)

    @staticmethod
    def _enc_lens(x, lens):
        """The packing lengths of RNNEncoder.forward (src/module.py:315-317).  pad_packed_sequence there has no total_length, so enc_output is
        [B, max(lens), 2H] against a [B, T] pad mask: the reference only works when max(lens) == T."""
        T = x.shape[1]
        lens_l = [int(v) for v in (lens.tolist() if hasattr(lens, "tolist") else lens)]
        if len(lens_l) != x.shape[0] or min(lens_l) < 1 or max(lens_l) != T:
            raise ValueError("encode: lengths must lie in 1..T with max(lens) == T == %d, one per sequence (got %r)" % (T, lens_l))
        return torch.tensor(lens_l, dtype=torch.int32, device=x.device)

    def _encode(self, P, x, lens_i32, pad_mask):
        from . import rnn
        enc_output, h, c = rnn.encoder(P, x, lens_i32)
        return ((h, c), enc_output), pad_mask

    def _lsa_state(self, B, Tk, device):
        """The attention state a stand-alone decode() call continues from (LocationSensitiveAttention.init_memory, src/module.py:409-414)."""
        if self.decoder.attention != "lsa":
            return None
        st = self.__dict__.get("_lsa_memory")
        if st is None or st[0].shape != (B, Tk) or st[0].device != device:
            st = (torch.zeros(B, Tk, dtype=torch.float32, device=device), torch.zeros(B, Tk, dtype=torch.float32, device=device))
            self.__dict__["_lsa_memory"] = st
        return st

    def clear_memory(self):
        """LocationSensitiveAttention.clear_memory (src/module.py:416-419): drops the state of stand-alone decode() calls, so that the next one
        starts from zero weights.  decode_sequence and infer_sequence call it as the reference's do (src/network.py:340, 374, 559, 613); a
        caller that steps decode() itself calls it between sequences."""
        self.__dict__.pop("_lsa_memory", None)


class TextRNN(_RNNModel):
    """src/network.py:503-624, eval path."""
    _prefix, _side = "text_m.", "text"
    infer_max_len = 300

    def __init__(self, args):
        super().__init__()
        self.prenet = TextPrenet(args.t_emb_dim, args.e_in, p=args.t_pre_drop)
        self._init_rnn(args)
        self.postnet = TextPostnet(args.hidden, args.t_post_drop)

    def _ids(self, text, P=None):
        """`P` given: the ids feed the decoder's window kernel, which indexes the embedding table with them unchecked, so they are checked
        here (one read-back per call; generated ids are in range by construction)."""
        if text.dtype != torch.int64 or text.dim() != 2 or not text.is_cuda:
            raise ValueError("text must be an int64 CUDA tensor [B,T]")
        if P is not None and text.numel():
            lo, hi = (int(v) for v in torch.aminmax(text))
            if lo < 0 or hi >= P.emb.shape[0]:
                raise ValueError("token ids must lie in 0..%d (got %d..%d)" % (P.emb.shape[0] - 1, lo, hi))
        return text.contiguous()

    def preprocess(self, text, text_lens, noise_in=False):
        from . import rnn
        P = self._pack(noise_in)
        text = self._ids(text)
        return rnn.text_frontend(P, text), text.eq(PAD_IDX)

    def encode(self, text, text_lens, noise_in=False):
        from . import rnn
        self._check_call(noise_in)
        lens = self._enc_lens(text, text_lens)
        P = self._pack()
        text = self._ids(text)
        return self._encode(P, rnn.text_frontend(P, text), lens, text.eq(PAD_IDX))          # the mask is text.eq(PAD_IDX), not the lengths (src/network.py:518)

    def decode_sequence(self, target, tgt_lens, enc_outputs, enc_ctxt_mask, teacher_ratio=1):
        from . import rnn
        P = self._pack(teacher_ratio=teacher_ratio)
        Tk = enc_outputs[1].shape[1]
        lens_k = _lens_of_pad_mask(enc_ctxt_mask, Tk, target.device)
        self.clear_memory()
        return rnn.text_generation(P, enc_outputs, lens_k, target.shape[1], target=self._ids(target, P)).run()

    def decode(self, input_, hidden_state, enc_output, enc_ctxt_mask):
        """One step on a given prefix [B,L] (src/network.py:562-575): (logits [B,1,V], (h, c))."""
        from . import rnn
        P = self._pack()
        B, Tk = enc_output.shape[:2]
        lens_k = _lens_of_pad_mask(enc_ctxt_mask, Tk, input_.device)
        g = rnn.text_generation(P, (hidden_state, enc_output), lens_k, 1, tokens=self._ids(input_, P), pos0=input_.shape[1] - 1,
                                lsa_state=self._lsa_state(B, Tk, enc_output.device))
        g.step(None)
        return g.logits[:, None, :g.V].clone(), (g.core.h, g.core.c)

    def postprocess(self, dec_output, distrib=False):
        from . import contract
        P = self._pack()
        shp = dec_output.shape
        y = contract.linear_rows(dec_output.detach().reshape(-1, shp[-1]).contiguous(), P.head_rows, P.head[1]).view(*shp[:-1], -1)
        return torch.log_softmax(y, dim=-1) if distrib else y

    def infer_sequence(self, enc_outputs, enc_ctxt_mask, max_len=300):
        return self.generation(enc_outputs, enc_ctxt_mask, max_len).run()

    def generation(self, enc_outputs, enc_ctxt_mask, max_len=None):
        from . import rnn
        P = self._pack()
        Tk = enc_outputs[1].shape[1]
        self.clear_memory()
        return rnn.text_generation(P, enc_outputs, _lens_of_pad_mask(enc_ctxt_mask, Tk, enc_outputs[1].device), max_len or self.infer_max_len)

    def forward(self, text, text_len, noise_in=False, teacher_ratio=1, ret_enc_hid=False):
        encoder_outputs, pad_mask = self.encode(text, text_len, noise_in=noise_in)
        pred = self.decode_sequence(text, text_len, encoder_outputs, pad_mask, teacher_ratio=1)    # 1 whatever the caller gives (src/network.py:621)
        if ret_enc_hid:
            return pred, encoder_outputs
        return pred


class SpeechRNN(_RNNModel):
    """src/network.py:279-402, eval path."""
    _prefix, _side = "speech_m.", "speech"
    infer_max_len = 815

    def __init__(self, args):
        super().__init__()
        self.prenet = SpeechPrenet(args.num_mels, args.s_pre_hid, args.e_in, p=args.s_pre_drop)
        self._init_rnn(args)
        self.postnet = SpeechPostnet(args.num_mels, args.hidden, p=args.s_post_drop)

    def _mel(self, mel):
        if mel.dim() != 3 or mel.shape[2] != self.postnet.num_mels or not mel.is_cuda:
            raise ValueError("mel must be a CUDA tensor [B,T,%d]" % self.postnet.num_mels)
        return mel.detach().to(torch.float32).contiguous()

    def preprocess(self, mel, mel_lens):
        from . import rnn
        P = self._pack()
        mel = self._mel(mel)
        lens = lens_i32(mel_lens, mel.device)
        return rnn.speech_frontend(P, mel), torch.arange(mel.shape[1], device=mel.device)[None, :] >= lens[:, None]

    def encode(self, mel, mel_lens, noise_in=False):
        from . import rnn
        self._check_call(noise_in)
        lens = self._enc_lens(mel, mel_lens)
        P = self._pack()
        mel = self._mel(mel)
        pad_mask = torch.arange(mel.shape[1], device=mel.device)[None, :] >= lens[:, None]       # from the lengths (src/network.py:292)
        return self._encode(P, rnn.speech_frontend(P, mel), lens, pad_mask)

    def decode_sequence(self, target, target_len, enc_outputs, enc_ctxt_mask, teacher_ratio=1):
        """Teacher-forced (src/network.py:352-377): no masking by length, target_len is handed back as the lengths."""
        from . import rnn
        P = self._pack(teacher_ratio=teacher_ratio)
        Tk = enc_outputs[1].shape[1]
        lens_k = _lens_of_pad_mask(enc_ctxt_mask, Tk, target.device)
        self.clear_memory()
        pre, post, stop = rnn.speech_generation(P, enc_outputs, lens_k, target.shape[1], target=self._mel(target)).run()
        return pre, post, stop, target_len

    def decode(self, input_, hidden_state, enc_output, enc_ctxt_mask):
        """One step on a given frame [B,1,M] (src/network.py:379-392): ((mel [B,1,M], stop [B,1,1]), (h, c))."""
        from . import rnn
        P = self._pack()
        B, Tk = enc_output.shape[:2]
        lens_k = _lens_of_pad_mask(enc_ctxt_mask, Tk, input_.device)
        g = rnn.speech_generation(P, (hidden_state, enc_output), lens_k, 1, frame=self._mel(input_), lsa_state=self._lsa_state(B, Tk, enc_output.device))
        g.step(None)
        return (g.head[:, None, :g.M].clone(), g.head[:, None, g.M:g.M + 1].clone()), (g.core.h, g.core.c)

    def postprocess(self, dec_output, distrib=False):
        """SpeechPostnet on [B,T,M] frames: the residual term, callers add it to their frames (src/network.py:394-395)."""
        from . import rnn
        P = self._pack()
        x = self._mel(dec_output)
        return rnn.speech_postnet_sum(P, x) - x

    def infer_sequence(self, enc_outputs, enc_ctxt_mask, max_len=815):
        return self.generation(enc_outputs, enc_ctxt_mask, max_len).run()

    def generation(self, enc_outputs, enc_ctxt_mask, max_len=None):
        from . import rnn
        P = self._pack()
        Tk = enc_outputs[1].shape[1]
        self.clear_memory()
        return rnn.speech_generation(P, enc_outputs, _lens_of_pad_mask(enc_ctxt_mask, Tk, enc_outputs[1].device), max_len or self.infer_max_len)

    def forward(self, mel, mel_len, noise_in=False, ret_enc_hid=False, teacher_ratio=1):
        encoder_outputs, pad_mask = self.encode(mel, mel_len, noise_in=noise_in)
        pre_pred, post_pred, stop_pred, _ = self.decode_sequence(mel, mel_len, encoder_outputs, pad_mask, teacher_ratio=1)
        if ret_enc_hid:
            return pre_pred, post_pred, stop_pred, encoder_outputs
        return pre_pred, post_pred, stop_pred


class LSTMDiscriminator(_Side):
    """src/network.py:172-186."""
    _prefix = "discriminator."

    def __init__(self, d_in, hidden, out=1, bidirectional=False, num_layers=1, dropout=.2, relu=.2):
        super().__init__()
        if hidden not in (64, 128) or out != 1:
            raise NotImplementedError("the persistent LSTM kernels are built for hidden=64 and hidden=128 with out=1 (got hidden=%r, out=%r)"
                                      % (hidden, out))
        self.num_dir = 2 if bidirectional else 1
        self.num_layers = num_layers
        self.hidden = hidden
        self.rnn = RNNEncoder(d_in, hidden, bidirectional=bidirectional, num_layers=num_layers, dropout=dropout)
        self.fc2 = nn.Linear(hidden, out)
        self.dropout_p, self.relu_slope = dropout, relu

    @on_stream("disc")
    def forward(self, out, out_len):
        Bd, T, Dm = out.shape
        lens = lens_i32(out_len, out.device)
        cx = self._ctx()
        need_dx = out.requires_grad and torch.is_grad_enabled()

        def run(tape, dummy, x):
            xv = Var(x.v.contiguous().view(Bd * T, Dm))
            if tape is not None:
                tape.record(lambda: setattr(x, "g", None if xv.g is None else xv.g.view(Bd, T, Dm)))
            lg = F.lstm_discriminator(cx, tape, self, xv, lens, Bd, T, need_input_grad=need_dx)
            o = Var(lg.v[:, 0])
            if tape is not None:
                tape.record(lambda: setattr(lg, "g", _as_padded(o.g.unsqueeze(-1), Bd, 4, 1)) if o.g is not None else None)
            return [o]
        return run_segment(run, None, cx.st.dummy, out)


class Discriminator(_Side):
    """src/network.py:154-170 (MLP discriminator of Lample et al.; present in the reference but never built by train.py)."""
    _prefix = "discriminator."

    def __init__(self, enc_dim, hidden=1024, out_classes=1, dropout=.2, relu=.2):
        super().__init__()
        self.fc1 = nn.Linear(enc_dim, hidden)
        self.fc2 = nn.Linear(hidden, hidden)
        self.fc3 = nn.Linear(hidden, hidden)
        self.fc4 = nn.Linear(hidden, out_classes)
        self.dropout_p, self.relu_slope, self.out_classes = dropout, relu, out_classes

    @on_stream("disc")
    def forward(self, enc_output):
        shape = enc_output.shape
        N, Dm = shape[:-1].numel(), shape[-1]
        cx = self._ctx()
        st = cx.st
        oc = self.out_classes
        ldo = (oc + 3) // 4 * 4

        def run(tape, dummy, x):
            xv = x.v.contiguous().view(N, Dm)
            acts, pres = [xv], []
            p = cx.p(self.dropout_p)
            streams = []
            h = xv
            for i in (1, 2, 3):
                W, b = cx.P["discriminator.fc%d.weight" % i], cx.P["discriminator.fc%d.bias" % i]
                u = torch.empty(N, W.shape[0], dtype=torch.float32, device=xv.device)
                ops.linear_fwd(h, W, b, u)
                a = torch.empty_like(u)
                s = cx.stream()
                ops.leaky_dropout(u, None, a, self.relu_slope, drop_p=p, seed=cx.seed, stream_id=s)
                pres.append(u); acts.append(a); streams.append(s)
                h = a
            W4, b4 = cx.P["discriminator.fc4.weight"], cx.P["discriminator.fc4.bias"]
            lg = torch.zeros(N, ldo, dtype=torch.float32, device=xv.device)
            ops.linear_fwd(h, W4, b4, lg[:, :oc])
            o = Var(lg[:, :oc].view(*shape[:-1], oc).squeeze(-1) if oc == 1 else lg[:, :oc].view(*shape[:-1], oc))
            if tape is not None:
                seed = cx.seed

                def bwd():
                    if o.g is None:
                        return
                    d = _as_padded(o.g.reshape(N, oc), N, ldo, oc)
                    g4 = st.g("discriminator.fc4.weight")
                    if g4 is not None:
                        ops.linear_wgrad(d[:, :oc], acts[3], g4)
                        ops.colsum(d[:, :oc], st.g("discriminator.fc4.bias"))
                    da = torch.empty_like(acts[3])
                    ops.linear_dgrad(d[:, :oc], W4, da)
                    for i in (3, 2, 1):
                        du = torch.empty_like(da)
                        ops.leaky_dropout(pres[i - 1], da, du, self.relu_slope, drop_p=p, seed=seed, stream_id=streams[i - 1])
                        gW = st.g("discriminator.fc%d.weight" % i)
                        if gW is not None:
                            ops.linear_wgrad(du, acts[i - 1], gW)
                            ops.colsum(du, st.g("discriminator.fc%d.bias" % i))
                        if i == 1 and not x.v.requires_grad:
                            break
                        da = torch.empty_like(acts[i - 1])
                        ops.linear_dgrad(du, cx.P["discriminator.fc%d.weight" % i], da)
                    else:
                        x.g = da.view(shape)
                tape.record(bwd)
            return [o]
        return run_segment(run, None, cx.st.dummy, enc_output)


class UNAST(_Side):
    """src/network.py:88-152."""

    def __init__(self, text_m, speech_m, discriminator=None, teacher=None):
        """NOTE: text_m and speech_m should be same type"""
        super().__init__()
        self.text_m = text_m
        self.speech_m = speech_m
        self.discriminator = discriminator
        self.teacher = teacher
        import weakref
        for sub in (text_m, speech_m, discriminator):
            if sub is not None:
                sub.__dict__["_unast_root"] = weakref.ref(self)

    def _root(self):
        return None

    def _store(self):
        st = self.__dict__.get("_unast_store")
        dev = next(self.parameters()).device
        if st is None or st.device != dev:
            if isinstance(self.text_m, _RNNModel):
                # the RNN generators live in their optimizer's flat buffers (unast_amd.train_rnn_step); the store holds what reads it: the discriminator
                if self.discriminator is None:
                    raise RuntimeError("an RNN model without a discriminator has no parameter store (unast_amd.train_rnn_step)")
                st = FlatStore(self.discriminator, prefix="discriminator.")
            else:
                st = FlatStore(self, prefix="")
            self.__dict__["_unast_store"] = st
        return st

    def text_ae(self, text, text_len, ret_enc_hid=False):
        return self.text_m.forward(text, text_len, noise_in=True, teacher_ratio=1, ret_enc_hid=ret_enc_hid)

    def speech_ae(self, mel, mel_len, ret_enc_hid=False):
        return self.speech_m.forward(mel, mel_len, noise_in=True, ret_enc_hid=ret_enc_hid, teacher_ratio=1)

    def tts(self, text, text_len, mel, mel_len, infer=False, ret_enc_hid=False):
        t_e_o, t_masks = self.text_m.encode(text, text_len)
        if not infer:
            pre_pred, post_pred, stop_pred, stop_lens = self.speech_m.decode_sequence(mel, mel_len, t_e_o, t_masks, teacher_ratio=1)
        else:
            pre_pred, post_pred, stop_pred, stop_lens = self.speech_m.infer_sequence(t_e_o, t_masks)
        if ret_enc_hid:
            return pre_pred, post_pred, stop_pred, stop_lens, t_masks[2]
        return pre_pred, post_pred, stop_pred, stop_lens

    def asr(self, text, text_len, mel, mel_len, infer=False, ret_enc_hid=False):
        s_e_o, s_masks = self.speech_m.encode(mel, mel_len)
        if not infer:
            text_pred = self.text_m.decode_sequence(text, text_len, s_e_o, s_masks, teacher_ratio=1)
        else:
            text_pred = self.text_m.infer_sequence(s_e_o, s_masks)
        if ret_enc_hid:
            return text_pred, s_masks[2]
        return text_pred

    def tts_and_asr(self, text, text_len, mel, mel_len, mel_aug, ret_enc_hid=False):
        """`tts(text, text_len, mel, mel_len)` and `asr(text, text_len, mel_aug, mel_len)` of the supervised step
        (src/train.py:231-259) issued encoder-first: with the text side and the speech side on their own HIP streams the
        reference's call order (tts, then asr) makes the speech decoder wait for the text encoder while the speech encoder
        queues behind it, and leaves the text decoder alone at the end.  Same four calls, same arithmetic; only the issue
        order differs (text encoder | speech encoder, then speech decoder | text decoder)."""
        t_e_o, t_masks = self.text_m.encode(text, text_len)
        s_e_o, s_masks = self.speech_m.encode(mel_aug, mel_len)
        pre_pred, post_pred, stop_pred, stop_lens = self.speech_m.decode_sequence(mel, mel_len, t_e_o, t_masks, teacher_ratio=1)
        text_pred = self.text_m.decode_sequence(text, text_len, s_e_o, s_masks, teacher_ratio=1)
        if ret_enc_hid:
            return (pre_pred, post_pred, stop_pred, stop_lens, t_masks[2]), (text_pred, s_masks[2])
        return (pre_pred, post_pred, stop_pred, stop_lens), text_pred

    def cm_text_in(self, text, text_len, ret_enc_hid=False):
        """src/network.py:103-112: text -> (no grad) TTS inference -> speech encoder -> text decoder."""
        with torch.no_grad():
            t_e_o, t_mask = self.text_m.encode(text, text_len)
            _, post_pred, _, pred_lens = self.speech_m.infer_sequence(t_e_o, t_mask, self.speech_m.infer_max_len)
        cm_s_e_o, cm_mask = self.speech_m.encode(post_pred.detach(), pred_lens.detach())
        text_pred = self.text_m.decode_sequence(text, text_len, cm_s_e_o, cm_mask, teacher_ratio=1)
        if ret_enc_hid:
            return text_pred, cm_mask[2], pred_lens
        return text_pred

    def cm_speech_in(self, mel, mel_len, ret_enc_hid=False):
        """src/network.py:114-123: speech -> (no grad) ASR inference -> text encoder -> speech decoder."""
        with torch.no_grad():
            s_e_o, s_mask = self.speech_m.encode(mel, mel_len)
            text_pred, text_pred_len = self.text_m.infer_sequence(s_e_o, s_mask, self.text_m.infer_max_len)
        cm_t_e_o, cm_t_masks = self.text_m.encode(text_pred.detach(), text_pred_len.detach())
        pre_pred, post_pred, stop_pred, stop_lens = self.speech_m.decode_sequence(mel, mel_len, cm_t_e_o, cm_t_masks, teacher_ratio=1)
        if ret_enc_hid:
            return pre_pred, post_pred, stop_pred, cm_t_masks[2], text_pred_len
        return pre_pred, post_pred, stop_pred

    def cm_both_in(self, text, text_len, mel, mel_len, ret_enc_hid=False):
        """cm_speech_in and cm_text_in of one batch (src/network.py:103-123, called back to back by src/train.py:261-294) with
        their two generations -- which do not depend on each other -- decoded in lock-step (unast_amd.inference.run_pair).
        Returns (cm_speech_in's result, cm_text_in's result)."""
        from .inference import run_pair
        with torch.no_grad():
            s_e_o, s_mask = self.speech_m.encode(mel, mel_len)
            t_e_o, t_mask = self.text_m.encode(text, text_len)
            (text_pred, text_pred_len), (_, post_pred, _, pred_lens) = run_pair(self.text_m.generation(s_e_o, s_mask),
                                                                                self.speech_m.generation(t_e_o, t_mask))
        cm_t_e_o, cm_t_masks = self.text_m.encode(text_pred.detach(), text_pred_len.detach())
        pre_pred, post_pred_s, stop_pred, stop_lens = self.speech_m.decode_sequence(mel, mel_len, cm_t_e_o, cm_t_masks, teacher_ratio=1)
        cm_s_e_o, cm_mask = self.speech_m.encode(post_pred.detach(), pred_lens.detach())
        text_out = self.text_m.decode_sequence(text, text_len, cm_s_e_o, cm_mask, teacher_ratio=1)
        if ret_enc_hid:
            return (pre_pred, post_pred_s, stop_pred, cm_t_masks[2], text_pred_len), (text_out, cm_mask[2], pred_lens)
        return (pre_pred, post_pred_s, stop_pred), text_out

    def num_params(self):
        return sum(p.numel() for p in self.parameters() if p.requires_grad)

    def expose_grads(self):
        """Materialise p.grad (views into the flat gradient buffer) for inspection or third-party optimizers."""
        self._store().expose_grads()
