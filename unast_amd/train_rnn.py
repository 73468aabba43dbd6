"""Training the RNN family's encoders on the HIP path: the train-mode `encode` of TextRNN / SpeechRNN (src/network.py:295-310, 514-537;
src/module.py:95-110, 217-230, 313-336) and its backward, as two explicit entry points.  `model.encode()` stays the eval forward and keeps
refusing train mode, autograd and noise_in (unast_amd.network._RNNModel._check_call).

    tape = encoder_forward(model, x, lens, noise_in=False, seed=0)      # tape.hidden = (h, c), tape.enc_output, tape.pad_mask
    d_mel = encoder_backward(tape, d_enc_output, d_h, d_c)                  # writes p.grad of model.prenet and model.encoder

Arithmetic as the reference's train mode: dropout at every nn.Dropout of the prenets (SpeechPrenet has ONE, after fc1: its second
'dropout2' key replaces the first in the OrderedDict, src/module.py:95-102), nn.LSTM's inter-layer dropout on layer 0's output, noise_fn on
the embedded text / the mel, and BatchNorm on batch statistics over all B*T positions with the running statistics updated.  Masks come
from the package's counter-based RNG; the tape lists every site (name, p, seed, stream, epoch, rows, cols, kind) so that a test can rebuild
them (tests/dropout_mirror.py).  Contractions keep fp32-level products in both directions (unast_amd.contract: linear_rows and its gradient
forms).  The recurrence and its backward are unast_lstm_seq_fwd_train / unast_lstm_seq_bwd (csrc/rnn.hip); dW_ih, dW_hh, dx and the
bias gradients are GEMMs and column sums over the kernel's dxproj.  Everything runs under torch.no_grad() on the current stream.  DESIGN 5i.

SpeechRNN's decoder trains through two more entry points with the same conventions (the second half of this file):

    tape = decoder_forward(model, target, enc_outputs, lens_k, seed=0)      # tape.pre, tape.post [B,T,M], tape.stop [B,T], tape.sites
    d_enc_output, d_h, d_c = decoder_backward(tape, d_pre, d_post, d_stop)  # writes p.grad of model.prenet, model.decoder, model.postnet

so that the speech autoencoder is encoder_forward -> decoder_forward -> decoder_backward -> encoder_backward(..., accumulate=True).

TextRNN's decoder trains through the last pair (the end of this file); both decoders run the same position loop
(_loop_forward / _loop_backward), each supplying its own prenet rows and head.  The packs (TrainPack for the encoders, DecoderPack /
TextDecoderPack over _LoopPack for the decoders) are built from unast_amd.rnn's extractors and cached by contract.cached_operands:

    tape = text_decoder_forward(model, target, enc_outputs, lens_k, seed=0) # tape.logits [B,T,len(symbols)], tape.sites
    d_enc_output, d_h, d_c = text_decoder_backward(tape, d_logits)          # writes p.grad of model.prenet, model.decoder, model.postnet

Greedy generation in TRAIN mode -- infer_sequence as UNAST.cm_speech_in / cm_text_in run it under no_grad with the modules in train() -- is the
last section; no backward, no tape, and the same position as the teacher-forced loop's (_TrainCell):

    tokens, lens = text_generate_train(model, enc_outputs, lens_k, max_len=300, seed=0)
    pre, post, stop, lens = speech_generate_train(model, enc_outputs, lens_k, max_len=815, seed=0)
"""
import collections

import torch

from . import contract, ops, rnn
from .contract import ALL, buf, detached
from .utils import EOS_IDX, PAD_IDX, SOS_IDX

_F32 = torch.float32
NOISE_P = 0.3                     # noise_fn's mask_p (src/utils.py:40)
# stream ids of the mask sites (one seed per call, one stream per site)
S_EMB, S_NOISE, S_PRE1, S_PRE2, S_PRE3, S_EDROP = 1, 2, 3, 4, 5, 6

Site = collections.namedtuple("Site", "name p seed stream epoch rows cols kind")      # kind: 'element' (dropout, 1/(1-p) rescale) or 'row' (noise_fn)


class TrainPack:
    """The operands the train kernels read, derived from the parameters of model.prenet and model.encoder (batch-statistics BatchNorm cannot
    use rnn.Pack's folded conv weights)."""

    def __init__(self, m, side):
        self.layers = [dict(w_ih=w_ih, wfrag=wfrag, wfrag_t=ops.lstm_whh_fragments_bwd(whh), b_ih=b_ih, b_hh=b_hh, params=dirs)
                       for dirs, (w_ih, wfrag, b_ih, b_hh), whh in rnn.encoder_layers(m.encoder)]
        self.reduce = [(w, b, lin.weight.detach().t().contiguous(), lin) for w, b, lin in rnn.encoder_reduce(m.encoder)]
        if side == "text":
            self.emb = detached(m.prenet.embed.weight)
            self.convs = [contract.tap_major(conv) + (conv, bn) for conv, bn in rnn.text_prenet_stages(m.prenet)]  # (tap-major weight pair, bias, conv, bn)
        else:
            self.fcs = rnn.speech_prenet_linears(m.prenet)


def train_pack_of(m, side):
    return contract.cached_operands(m, rnn.ENCODER_TRAIN_SLOT, _encoder_params(m), lambda: TrainPack(m, side))


class Tape:
    """What encoder_forward returns and encoder_backward consumes (once)."""

    def __init__(self):
        self.sites = []
        self.used = False

    def site(self, name, p, stream, rows, cols, kind="element"):
        if p > 0.0:
            self.sites.append(Site(name, float(p), self.seed, stream, self.epoch, rows, cols, kind))


def _encoder_params(model):
    return list(model.prenet.parameters()) + list(model.encoder.parameters())


def _check_model(model, what):
    from .network import TextRNN, SpeechRNN
    if not isinstance(model, (TextRNN, SpeechRNN)):
        raise TypeError("%s: model must be a unast_amd.network.TextRNN or SpeechRNN" % what)
    if not model.training:
        raise RuntimeError("%s is the train-mode entry point: call model.train() first (model.encode() is the eval forward)" % what)


# ---- forward -------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def encoder_forward(model, x, lens, noise_in=False, seed=0):
    """Train-mode `encode`: x = token ids [B,T] int64 (TextRNN) or mel [B,T,num_mels] (SpeechRNN) on the GPU, lens as encode takes them
    (max(lens) == T).  Returns a Tape: .hidden = (h, c) [2,B,256], .enc_output [B,T,512] (zero rows at t >= lens[b]), .pad_mask bool [B,T].
    Updates the BatchNorm running statistics (text)."""
    _check_model(model, "encoder_forward")
    if not torch.is_tensor(x) or x.dim() < 2:
        raise ValueError("encoder_forward: x must be a tensor [B,T] (text) or [B,T,num_mels] (speech)")
    side = model._side
    lens_i32 = model._enc_lens(x, lens)
    if not x.is_cuda:
        raise ValueError("encoder_forward: x must be a CUDA tensor")
    if next(model.parameters()).device.type != "cuda":
        raise RuntimeError("unast_amd runs on the GPU only: move the model to a CUDA (ROCm) device first; there is no CPU path")
    P = train_pack_of(model, side)
    tape = Tape()
    tape.model, tape.side, tape.P, tape.lens, tape.noise_in = model, side, P, lens_i32, bool(noise_in)
    tape.seed, tape.epoch = int(seed), ops.rng_epoch_counter().clone()
    dev = x.device
    noise_p = NOISE_P if noise_in else 0.0
    if side == "text":
        ids = model._ids(x)
        B, T = ids.shape
        N = B * T
        p = float(model.prenet.p)
        x0 = buf(N, P.emb.shape[1], dev=dev)
        ops.embed_fwd(ids, P.emb, x0, T, drop_p=p, seed=seed, stream_id=S_EMB, noise_p=noise_p, noise_stream=S_NOISE)
        tape.site("emb_dropout", p, S_EMB, N, x0.shape[1])
        tape.site("noise", noise_p, S_NOISE, N, 1, "row")
        tape.ids = ids
        tape.pad_mask = ids.eq(PAD_IDX)
        front = _bn_stages_forward(tape, x0.view(B, T, -1), P.convs, 2, 1, p, S_PRE1, ["dropout1", "dropout2", "dropout3"], "encoder_forward")
    else:
        mel = model._mel(x)
        B, T, M = mel.shape
        N = B * T
        p = float(model.prenet.p)
        m2 = mel.view(N, M)
        if noise_in:
            mn = torch.empty_like(m2)
            ops.rowmask(m2, mn, noise_p, seed, S_NOISE)
            m2 = mn
        tape.site("noise", noise_p, S_NOISE, N, 1, "row")
        (w1, b1, _), (w2, b2, _) = P.fcs
        a1 = contract.linear_rows(m2, w1, b1)
        h1 = torch.empty_like(a1)
        ops.leaky_dropout(a1, None, h1, 0.0, p, seed, S_PRE1)
        tape.site("dropout2", p, S_PRE1, N, a1.shape[1])
        h2 = contract.linear_rows(h1, w2, b2, act=1)
        tape.m2, tape.a1, tape.h1, tape.h2 = m2, a1, h1, h2
        tape.pad_mask = torch.arange(T, device=dev)[None, :] >= lens_i32[:, None]
        front = h2
    # ---- RNNEncoder.forward: packed bidirectional LSTM stack, inter-layer dropout, reduce_h_W / reduce_c_W ------------------------------------
    e_drop = float(model.encoder.rnn.dropout)
    L = len(P.layers)
    h, c = buf(L, B, 256, dev=dev), buf(L, B, 256, dev=dev)
    tape.B, tape.T, tape.e_drop = B, T, e_drop
    tape.lstm = []
    x2 = front
    for l, lay in enumerate(P.layers):
        xproj = contract.linear_rows(x2, lay["w_ih"], None).view(B, T, -1)
        y, hn, cn = buf(B, T, 512, dev=dev), buf(B, 512, dev=dev), buf(B, 512, dev=dev)
        saved, hprev = buf(B, T, 2, 5, 256, dev=dev), buf(B, T, 512, dev=dev)
        ops.lstm_seq_fwd_train(xproj, lay["wfrag"], lay["b_ih"], lay["b_hh"], lens_i32, y, hn, cn, saved, hprev)
        ops.rnn_linear(hn, P.reduce[0][0], P.reduce[0][1], h[l])
        ops.rnn_linear(cn, P.reduce[1][0], P.reduce[1][1], c[l])
        tape.lstm.append(dict(x=x2, hn=hn, cn=cn, saved=saved, hprev=hprev))
        x2 = y.view(N, 512)
        if l + 1 < L and e_drop > 0.0:
            yd = torch.empty_like(x2)
            ops.leaky_dropout(x2, None, yd, 1.0, e_drop, seed, S_EDROP + l)
            tape.site("e_drop%d" % l, e_drop, S_EDROP + l, N, 512)
            x2 = yd
    tape.hidden, tape.enc_output = (h, c), y
    return tape


# ---- backward ------------------------------------------------------------------------------------------------------------------------------
def _cot(t, shape, name, dev, what="encoder_backward"):
    if t is None:
        return None
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype is _F32 and tuple(t.shape) == tuple(shape)):
        raise ValueError("%s: %s must be a float32 CUDA tensor %s" % (what, name, tuple(shape)))
    return t.detach().contiguous()


@torch.no_grad()
def encoder_backward(tape, d_enc_output=None, d_h=None, d_c=None, accumulate=False):
    """Backward of encoder_forward for the scalar whose gradients with respect to enc_output [B,T,512], h and c [2,B,256] are given (None =
    zero).  Writes p.grad of exactly the parameters under model.prenet and model.encoder, in the reference's shapes: overwritten
    (accumulate=False; an existing dense fp32 .grad is kept in place) or added to (accumulate=True).  Returns d_mel [B,T,num_mels] (speech)
    or None (text).  A tape is used once."""
    if not isinstance(tape, Tape) or isinstance(tape, DecoderTape):
        raise TypeError("encoder_backward: tape must come from encoder_forward")
    if tape.used:
        raise RuntimeError("encoder_backward: this tape has been used; run encoder_forward again")
    model, P, B, T, seed = tape.model, tape.P, tape.B, tape.T, tape.seed
    N = B * T
    dev = tape.enc_output.device
    L = len(P.layers)
    d_enc_output = _cot(d_enc_output, (B, T, 512), "d_enc_output", dev)
    d_h, d_c = _cot(d_h, (L, B, 256), "d_h", dev), _cot(d_c, (L, B, 256), "d_c", dev)
    tape.used = True
    contract.prepare_grads(_encoder_params(model), accumulate)

    dy = d_enc_output.view(N, 512) if d_enc_output is not None else torch.zeros(N, 512, dtype=_F32, device=dev)
    for l in range(L - 1, -1, -1):
        lay, st = P.layers[l], tape.lstm[l]
        dfin = []
        for d_state, (W, _, Wt, lin), fin in ((d_h, P.reduce[0], st["hn"]), (d_c, P.reduce[1], st["cn"])):
            if d_state is None:
                dfin.append(None)
                continue
            g = d_state[l]                                                                 # [B,256]: the gradient of reduce_*_W's output
            dfin.append(ops.rnn_linear(g, Wt, None, buf(B, 512, dev=dev)))                 # g W [256,512]
            contract.wgrad_rows(contract.parts(g), ALL, fin, contract.resid_of(fin), lin.weight.grad, (lin.bias.grad,))
        if l + 1 < L and tape.e_drop > 0.0:
            dyd = torch.empty_like(dy)
            ops.leaky_dropout(dy, dy, dyd, 1.0, tape.e_drop, seed, S_EDROP + l)            # slope 1: the mask and its 1/(1-p) only
            dy = dyd
        dxproj = buf(B, T, 2048, dev=dev)
        ops.lstm_seq_bwd(dy.view(B, T, 512), lay["wfrag_t"], st["saved"], tape.lens, dxproj, dhfinal=dfin[0], dcfinal=dfin[1])
        dxp = contract.parts(dxproj.view(N, 2048))
        xin, hprev = st["x"], st["hprev"].view(N, 512)
        xin_res, hprev_res = contract.resid_of(xin), contract.resid_of(hprev)
        for d, (w_ih, w_hh, b_ih, b_hh) in enumerate(lay["params"]):
            cols = slice(1024 * d, 1024 * (d + 1))
            contract.wgrad_rows(dxp, cols, xin, xin_res, w_ih.grad, (b_ih.grad, b_hh.grad))
            contract.wgrad_rows(dxp, cols, hprev[:, 256 * d:256 * (d + 1)], hprev_res[:, 256 * d:256 * (d + 1)], w_hh.grad)
        dy = contract.dgrad_rows(dxp, lay["w_ih"], buf(N, xin.shape[1], dev=dev))

    if tape.side == "text":
        C = 256
        p = float(model.prenet.p)
        bn_ws = torch.empty(2 * C, dtype=torch.float64, device=dev)
        for i in (2, 1, 0):
            wpair, _, conv, bn = P.convs[i]
            dz = buf(N, C, dev=dev)
            ops.bn_bwd(dy, tape.zs[i], tape.mean[i], tape.rstd[i], bn.weight, bn.bias, dz, bn.weight.grad, bn.bias.grad, bn_ws, 1, drop_p=p, seed=seed,
                       stream_id=S_PRE1 + i)
            dy = contract.conv_grads(dz, tape.xs[i], B, T, wpair, conv, 2)
        noise_p = NOISE_P if tape.noise_in else 0.0
        ops.embed_bwd(tape.ids, dy, model.prenet.embed.weight.grad, T, drop_p=p, seed=seed, stream_id=S_EMB, noise_p=noise_p, noise_stream=S_NOISE,
                      padding_idx=model.prenet.embed.padding_idx)
        return None

    p = float(model.prenet.p)
    (w1, _, fc1), (w2, _, fc2) = P.fcs
    ops.relu_bwd(dy, tape.h2)
    dyp = contract.parts(dy)
    contract.wgrad_rows(dyp, ALL, tape.h1, contract.resid_of(tape.h1), fc2.weight.grad, (fc2.bias.grad,))
    dh1 = contract.dgrad_rows(dyp, w2, buf(N, tape.h1.shape[1], dev=dev))
    da1 = torch.empty_like(dh1)
    ops.leaky_dropout(tape.a1, dh1, da1, 0.0, p, seed, S_PRE1)
    dap = contract.parts(da1)
    contract.wgrad_rows(dap, ALL, tape.m2, contract.resid_of(tape.m2), fc1.weight.grad, (fc1.bias.grad,))
    M = tape.m2.shape[1]
    d_mel = contract.dgrad_rows(dap, w1, buf(N, M, dev=dev))
    if tape.noise_in:
        out = torch.empty_like(d_mel)
        ops.rowmask(d_mel, out, NOISE_P, seed, S_NOISE)
        d_mel = out
    return d_mel.view(B, T, M)


# ==== SpeechRNN decoder: teacher-forced train-mode decode_sequence (src/network.py:352-377) and its backward; DESIGN 5j ============================
S_DPRE, S_DDROP, S_DOUT, S_POST = 8, 9, 10, 11      # decoder prenet dropout, nn.LSTM inter-layer, dropout1, the four post-net dropouts (11..14)

class _LoopPack:
    """The operands of the position loop both decoders share (RNNDecoder: the attention layer, the two LSTM cells, the projection): the
    fp32-level weight pairs of the many-row contractions, and the transposed weights the per-position input-gradient contractions
    (unast_rnn_linear: Y = X W^T) take as their W."""

    def __init__(self, m, what):
        dec = m.decoder
        if dec.num_layers != 2 or dec.attention not in ("luong", "lsa"):
            raise NotImplementedError("%s: two decoder layers with 'luong' or 'lsa' attention (what the eval path supports)" % what)
        r = dec.rnn
        w0 = r.weight_ih_l0.detach()
        if tuple(w0.shape) != (1024, 768) or tuple(r.weight_ih_l1.shape) != (1024, 256):
            raise NotImplementedError("%s: hidden = e_in = 256 with a 512-wide encoder output" % what)
        self.w_ih0_p, self.w_ih0_c = contract.resid(w0[:, :256]), detached(w0[:, 256:])     # the prenet columns (batched) and the context columns
        self.w_hh0, self.w_ih1, self.w_hh1 = detached(r.weight_hh_l0), detached(r.weight_ih_l1), detached(r.weight_hh_l1)
        self.bias = [detached(getattr(r, n)) for n in ("bias_ih_l0", "bias_hh_l0", "bias_ih_l1", "bias_hh_l1")]
        tr = lambda w: w.detach().t().contiguous()                                          # noqa: E731
        self.wt_ihc0, self.wt_hh0, self.wt_ih1, self.wt_hh1 = tr(w0[:, 256:]), tr(r.weight_hh_l0), tr(r.weight_ih_l1), tr(r.weight_hh_l1)
        operands, (self.q_lin, self.mem_lin, self.v_lin, self.conv_mod, self.dense_lin) = rnn.attention_operands(dec)
        vars(self).update(operands)                                                         # mode, Wq, Wmem, v, conv_w, dense_w
        self.A = self.Wq.shape[0]
        if self.A % 4 or self.A > 64:
            raise NotImplementedError("%s: attn_dim must be a multiple of 4, at most 64 (got %d)" % (what, self.A))
        self.proj_lin = dec.linear_projection.linear_layer
        self.proj = (contract.resid(self.proj_lin.weight), detached(self.proj_lin.bias))


class DecoderPack(_LoopPack):
    """SpeechRNN: the loop's operands plus the prenet's two linears, the [linear_project | stop_linear] head and the post-net."""

    def __init__(self, m):
        super().__init__(m, "decoder_forward")
        po = m.postnet
        self.fcs = rnn.speech_prenet_linears(m.prenet)
        self.M = po.linear_project.weight.shape[0]
        self.head, self.ldh = rnn.padded_head(po.linear_project, po.stop_linear)            # [linear_project | stop_linear | zero rows] as one head
        self.post = [contract.tap_major(conv) + (conv, bn) for conv, bn in rnn.speech_postnet_stages(po)]
        self.post_out = contract.tap_major(po.conv2.conv) + (po.conv2.conv,)


def _decoder_params(model):
    return list(model.prenet.parameters()) + list(model.decoder.parameters()) + list(model.postnet.parameters())


class TextDecoderPack(_LoopPack):
    """TextRNN: the loop's operands plus the prefix prenet's embedding, convs and BatchNorms and the TextPostnet head (fc1, rows padded to a
    multiple of 4 with zeros)."""

    def __init__(self, m):
        super().__init__(m, "text_decoder_forward")
        pn, fc = m.prenet, m.postnet.fc1
        self.emb = detached(pn.embed.weight)
        self.convs = [contract.tap_major(conv) + (conv, bn) for conv, bn in rnn.text_prenet_stages(pn)]
        E = self.emb.shape[1]
        if E % 4 or 256 % (E // 4) or any(tuple(wp[0].shape[::2]) != (256, cin) or wp[0].shape[1] != 5 for (wp, _, _, _), cin in zip(self.convs, (E, 256, 256))):
            raise NotImplementedError("text_decoder_forward: three 5-tap convs into 256 channels over an embedding whose width / 4 divides 256")
        if tuple(fc.weight.shape[1:]) != (256,):
            raise NotImplementedError("text_decoder_forward: TextPostnet.fc1 over 256 features")
        self.V = fc.weight.shape[0]
        self.head, self.ldh = rnn.padded_head(fc)


def decoder_pack_of(m, cls=DecoderPack):
    return contract.cached_operands(m, rnn.DECODER_TRAIN_SLOT, _decoder_params(m), lambda: cls(m))


class DecoderTape(Tape):
    """What decoder_forward returns and decoder_backward consumes (once): .pre, .post [B,T,M], .stop [B,T], .sites."""

    def saved_bytes(self):
        """Bytes of the state kept for the backward (the slabs of the forward loop and of the batched stages)."""
        seen, n = set(), 0
        for v in self.__dict__.values():
            for t in (v if isinstance(v, (list, tuple)) else [v]):
                if torch.is_tensor(t) and t.is_cuda and t.untyped_storage().data_ptr() not in seen:
                    seen.add(t.untyped_storage().data_ptr())
                    n += t.untyped_storage().nbytes()
        return n


def _drop_factor(p, seed, stream, rows, cols, dev):
    """The factor tensor of a dropout site [rows, cols] (0 or 1/(1-p)): the element-wise kernel's mask applied to ones."""
    ones = torch.ones(rows, cols, dtype=_F32, device=dev)
    f = torch.empty_like(ones)
    ops.leaky_dropout(ones, None, f, 1.0, p, seed, stream)
    return f


@torch.no_grad()
def decoder_forward(model, target, enc_outputs, lens_k, seed=0, mark=None):
    """Train-mode, teacher-forced SpeechRNN.decode_sequence (teacher_ratio = 1): target [B,T,num_mels] on the GPU, enc_outputs = ((h, c)
    [2,B,256], enc_output [B,Tk,512]) or an encoder Tape, lens_k the live keys per sequence (1..Tk).  Returns a DecoderTape: .pre and .post
    [B,T,num_mels], .stop [B,T].  Updates the post-net's BatchNorm running statistics and drops the model's cached eval operands.
    mark (optional): called with 'loop_begin' / 'loop_end' around the position loop (a caller that times it records an event there)."""
    from .network import TextRNN, SpeechRNN
    if isinstance(model, TextRNN):
        raise NotImplementedError("decoder_forward: SpeechRNN only -- TextRNN.decode runs TextPrenet over the whole prefix at every position "
                                  "(batch-statistics BatchNorm over the prefix's rows and a running-statistics update per position, O(T^2)): "
                                  "text_decoder_forward / text_decoder_backward train it")
    if not isinstance(model, SpeechRNN):
        raise TypeError("decoder_forward: model must be a unast_amd.network.SpeechRNN")
    if not model.training:
        raise RuntimeError("decoder_forward is the train-mode entry point: call model.train() first (model.decode_sequence() is the eval forward)")
    mel = model._mel(target)
    B, T, M = mel.shape
    tape = _begin_decoder_tape("decoder_forward", model, DecoderPack, enc_outputs, lens_k, B, T, seed, mel.device)
    P, N = tape.P, B * T
    p_pre, p_post = float(model.prenet.p), float(model.postnet.p)

    # ---- batched before the loop: the prenet on all fed frames ------------------------------------------------------------------------------
    feed = ops.shift_frames(mel, torch.empty_like(mel)).view(N, M)                          # feed_0 = 0, feed_i = target[:, i-1]
    (w1, b1, _), (w2, b2, _) = P.fcs
    a1 = contract.linear_rows(feed, w1, b1)
    h1 = torch.empty_like(a1)
    ops.leaky_dropout(a1, None, h1, 0.0, p_pre, seed, S_DPRE)
    tape.site("d_prenet_dropout", p_pre, S_DPRE, N, a1.shape[1])
    pre = contract.linear_rows(h1, w2, b2, act=1)
    tape.feed, tape.a1, tape.h1 = feed, a1, h1
    o = _loop_forward(tape, pre, mark)

    # ---- batched after the loop: the head, the post-net -----------------------------------------------------------------------------------------
    dev = mel.device
    head = contract.linear_rows(o, P.head[0], P.head[1]).view(B, T, P.ldh)
    outs = torch.zeros(B, T + 1, M, dtype=_F32, device=dev)                                 # position 0 = the all-zero go frame
    outs[:, 1:].copy_(head[:, :, :M])
    tape.stop = head[:, :, M].contiguous()
    tape.head = head                                                                        # [pre | stop | zero columns]: what the loss kernels read
    post = _postnet_forward(tape, outs, S_POST, "decoder_forward")
    tape.pre, tape.post = outs[:, 1:], post[:, 1:]
    return tape


def _postnet_forward(tape, outs, stream0, what):
    """SpeechPostnet in train mode over outs [B, T+1, M] (the go frame included, as the reference runs it): four conv + BatchNorm + tanh +
    dropout stages (_bn_stages_forward; stream0 = the first of their stream ids) and conv2, plus the residual.  Returns outs + postnet(outs)
    [B, T+1, M].  Shared by decoder_forward and speech_generate_train."""
    P, (B, T1, _) = tape.P, outs.shape
    y = _bn_stages_forward(tape, outs, P.post, 4, 2, float(tape.model.postnet.p), stream0, ["post_dropout%d" % k for k in range(4)], what)
    post = contract.conv(y.view(B, T1, 256), P.post_out[0], P.post_out[1], 4)
    ops.add_inplace(post, outs)
    return post


def _bn_stages_forward(tape, cur, stages, pad_left, act, p, stream0, names, what):
    """The conv + BatchNorm + activation (1 ReLU, 2 tanh) + dropout stages of TextPrenet / SpeechPostnet in train mode over cur [B,T,Cin]: batch
    statistics over all B T rows, running statistics updated (so the cached eval operands are dropped).  Leaves the stages' inputs, conv outputs
    and statistics on the tape (xs, zs, mean, rstd: what the backward reads) and the dropout sites `names`; returns the last output [B*T,256]."""
    B, T, _ = cur.shape
    N, dev = B * T, cur.device
    tape.xs, tape.zs = [cur.view(N, -1)], []
    tape.mean, tape.rstd = buf(len(stages), 256, dev=dev), buf(len(stages), 256, dev=dev)
    bn_ws = torch.empty(512, dtype=torch.float64, device=dev)
    for k, (wp, bias, _, bn) in enumerate(stages):
        contract.check_bn(bn, what)
        z = contract.conv(cur, wp, bias, pad_left).view(N, 256)
        y = buf(N, 256, dev=dev)
        ops.bn_fwd(z, bn.weight, bn.bias, y, tape.mean[k], tape.rstd[k], bn.running_mean, bn.running_var, bn_ws, act, drop_p=p, seed=tape.seed,
                   stream_id=stream0 + k, eps=bn.eps, momentum=bn.momentum, num_batches_tracked=bn.num_batches_tracked)
        tape.site(names[k], p, stream0 + k, N, 256)
        tape.zs.append(z)
        tape.xs.append(y)
        cur = y.view(B, T, 256)
    rnn.drop_eval_pack(tape.model)
    return y


def _begin_decoder_tape(what, model, pack_cls, enc_outputs, lens_k, B, T, seed, dev):
    """The memory-side checks and the tape header both decoder entry points share."""
    if isinstance(enc_outputs, Tape):
        enc_outputs = (enc_outputs.hidden, enc_outputs.enc_output)
    (h0, c0), enc = enc_outputs
    if T < 1 or not (torch.is_tensor(enc) and enc.is_cuda and enc.dim() == 3 and enc.shape[0] == B and enc.shape[2] == 512):
        raise ValueError("%s: enc_output must be a CUDA tensor [B,Tk,512] with target's B, T >= 1" % what)
    Tk = enc.shape[1]
    if not 1 <= Tk <= 2048:
        raise ValueError("%s: 1 <= Tk <= 2048 (got %d)" % (what, Tk))
    for t, n in ((h0, "h"), (c0, "c")):
        if not (torch.is_tensor(t) and t.is_cuda and tuple(t.shape) == (2, B, 256)):
            raise ValueError("%s: %s must be a CUDA tensor [2,B,256]" % (what, n))
    lens_l = [int(v) for v in (lens_k.tolist() if hasattr(lens_k, "tolist") else lens_k)]
    if len(lens_l) != B or min(lens_l) < 1 or max(lens_l) > Tk:
        raise ValueError("%s: lens_k must hold one length in 1..Tk = %d per sequence (got %r)" % (what, Tk, lens_l))
    if next(model.parameters()).device.type != "cuda":
        raise RuntimeError("unast_amd runs on the GPU only: move the model to a CUDA (ROCm) device first; there is no CPU path")
    P = decoder_pack_of(model, pack_cls)
    enc, h0, c0 = (t.detach().to(_F32).contiguous() for t in (enc, h0, c0))
    tape = DecoderTape()
    tape.model, tape.P, tape.B, tape.T, tape.Tk, tape.entry = model, P, B, T, Tk, what
    tape.lens = torch.tensor(lens_l, dtype=torch.int32, device=dev)
    tape.seed, tape.epoch = int(seed), ops.rng_epoch_counter().clone()
    tape.enc, tape.h0, tape.c0 = enc, h0, c0
    return tape


class _TrainCell:
    """One decoder position in train mode (RNNDecoder.forward, src/module.py:362-374, up to the projection's input): attention, then the two
    LSTM cells with the saved state the backward reads -- 7 launches.  The teacher-forced loop (_loop_forward: rows of [B,T,...] slabs) and the
    train-mode generations (_GenState.step: ping-pong halves) each hand it views of where their rows live.
    (The eval step rnn._Core.step stays apart: its kernels update the state in place and save nothing, and it splits the projection differently.)"""

    def __init__(self, tape):
        P, enc, B, Tk = tape.P, tape.enc, tape.B, tape.Tk
        self.P, self.enc, self.lens, self.h0, self.c0 = P, enc, tape.lens, tape.h0, tape.c0
        self.mem = contract.linear_rows(enc.view(B * Tk, 512), P.Wmem, None).view(B, Tk, P.A)  # memory-side projection, once for all positions
        self.ga, self.gb = buf(B, 1024, dev=enc.device), buf(B, 1024, dev=enc.device)

    def __call__(self, first, xp0, mask, h0d, q, w_in, w_out, cum_in, cum_out, ctx, h0_in, h0_out, s0, c0_in, s1, c1_in, h1_out):
        """xp0 = W_ih_l0[:, :256] prenet + b_ih; mask / h0d: nn.LSTM's inter-layer dropout factors and the dropped h0_out (None with dropout off);
        q: the top layer's h from BEFORE this position's LSTM (src/module.py:365); w_* / cum_* [B,Tk]: the attention weights and (lsa, else None)
        their running sum, read / written; ctx, h0_out, h1_out: destinations; s0, s1 [B,5,256]: the layers' saved state, c0_in / c1_in their
        previous cell states.  first: position 0 -- the encoder's final states stand in for q, c0_in and c1_in, which are not read."""
        P, ga, gb = self.P, self.ga, self.gb
        if first:
            q, c0_in, c1_in = self.h0[1], self.c0[0], self.c0[1]
        _, b_hh0, b_ih1, b_hh1 = P.bias
        ops.rnn_attn_step_train(P.mode, q, P.Wq, self.mem, P.v, self.enc, self.lens, ctx, w_out, prev_in=w_in, cum_in=cum_in, cum_out=cum_out,
                                conv_w=P.conv_w, dense_w=P.dense_w)
        ops.rnn_linear(ctx, P.w_ih0_c, None, gb, R=xp0)                                     # LSTM input = [prenet | context] (src/module.py:367)
        ops.rnn_linear(h0_in, P.w_hh0, b_hh0, ga, R=gb)
        ops.lstm_cell_train(ga, c0_in, s0, h0_out, mask=mask, hd=h0d)
        ops.rnn_linear(h0d if mask is not None else h0_out, P.w_ih1, b_ih1, gb)
        ops.rnn_linear(q, P.w_hh1, b_hh1, ga, R=gb)
        ops.lstm_cell_train(ga, c1_in, s1, h1_out)


def _loop_forward(tape, pre, mark):
    """RNNDecoder over all positions, shared by both decoders: pre [B*T,256] = the prenet's row for every position (with teacher forcing it
    does not depend on the recurrence).  Hoists W_ih_l0[:, :256] pre + b_ih and the memory-side projection, runs the position loop, then
    the projection + tanh + dropout1 for all positions.  Keeps the loop's state on the tape; returns o [B*T,256], the head's input."""
    model, P, B, T, Tk, seed = tape.model, tape.P, tape.B, tape.T, tape.Tk, tape.seed
    dev = tape.enc.device
    N, lsa = B * T, P.mode == ops.ATTN_LSA
    p_dec = float(model.decoder.p)
    xp0 = contract.linear_rows(pre, P.w_ih0_p, P.bias[0]).view(B, T, 1024)
    cell = _TrainCell(tape)
    tape.pre_act, tape.mem = pre, cell.mem

    # ---- the loop: per position the cell's 7 launches on host-indexed slices of [B,T,...] slabs ------------------------------------------------
    Tkp = (Tk + 3) // 4 * 4
    W = torch.zeros(B, T + 1, Tkp, dtype=_F32, device=dev)                                  # W[:, i+1] = w_i; W[:, 0] = 0 is position 0's prev
    CUM = torch.zeros(B, T + 1, Tkp, dtype=_F32, device=dev) if lsa else None               # CUM[:, i] = what position i read
    HC = buf(B, T, 768, dev=dev)                                                            # [h1_i | ctx_i]: the projection's input rows
    H0 = buf(B, T + 1, 256, dev=dev)                                                        # H0[:, i] = layer 0's h before position i
    H0[:, 0].copy_(tape.h0[0])
    S0, S1 = buf(B, T, 5, 256, dev=dev), buf(B, T, 5, 256, dev=dev)
    F1 = _drop_factor(p_dec, seed, S_DDROP, N, 256, dev).view(B, T, 256) if p_dec > 0.0 else None
    tape.site("d_drop0", p_dec, S_DDROP, N, 256)
    H0d = buf(B, T, 256, dev=dev) if F1 is not None else None
    if mark is not None:
        mark("loop_begin")
    for i in range(T):                                                                      # (index -1 at i = 0: the cell does not read those views)
        cell(i == 0, xp0[:, i], F1[:, i] if F1 is not None else None, H0d[:, i] if F1 is not None else None, HC[:, i - 1, :256], W[:, i, :Tk], W[:, i + 1, :Tk],
             CUM[:, i, :Tk] if lsa else None, CUM[:, i + 1, :Tk] if lsa else None, HC[:, i, 256:], H0[:, i], H0[:, i + 1], S0[:, i], S0[:, i - 1, 4], S1[:, i],
             S1[:, i - 1, 4], HC[:, i, :256])
    if mark is not None:
        mark("loop_end")
    tape.W, tape.CUM, tape.HC, tape.H0, tape.H0d, tape.S0, tape.S1, tape.F1 = W, CUM, HC, H0, H0d, S0, S1, F1

    # ---- batched after the loop: projection + tanh + dropout1 ------------------------------------------------------------------------------------
    tz = ops.tanh_rows(contract.linear_rows(HC.view(N, 768), P.proj[0], P.proj[1]))
    o = tz
    if p_dec > 0.0:
        o = torch.empty_like(tz)
        ops.leaky_dropout(tz, None, o, 1.0, p_dec, seed, S_DOUT)
    tape.site("d_dropout1", p_dec, S_DOUT, N, 256)
    tape.tz, tape.o = tz, o
    return o


def _add_over_b(part, grad):
    """grad += sum_b part[b] in the fixed order b = 0, 1, ... (the per-sequence partial sums of unast_rnn_attn_step_bwd)."""
    flat = grad.view(-1)
    for b in range(part.shape[0]):
        ops.add_inplace(flat, part[b])


@torch.no_grad()
def decoder_backward(tape, d_pre=None, d_post=None, d_stop=None, accumulate=False, mark=None):
    """Backward of decoder_forward for the scalar whose gradients with respect to pre, post [B,T,num_mels] and stop [B,T] are given (None =
    zero).  Writes p.grad of exactly the parameters under model.prenet, model.decoder and model.postnet (overwritten, or added to with
    accumulate=True; an existing dense fp32 .grad is kept in place).  Returns (d_enc_output [B,Tk,512], d_h, d_c [2,B,256]), the cotangents
    encoder_backward takes.  A tape is used once.  mark: as decoder_forward's."""
    if not isinstance(tape, DecoderTape) or getattr(tape, "entry", "decoder_forward") != "decoder_forward":
        raise TypeError("decoder_backward: tape must come from decoder_forward")
    if tape.used:
        raise RuntimeError("decoder_backward: this tape has been used; run decoder_forward again")
    model, P, B, T, seed = tape.model, tape.P, tape.B, tape.T, tape.seed
    M, ldh = P.M, P.ldh
    N, N1 = B * T, B * (T + 1)
    dev = tape.enc.device
    d_pre, d_post = _cot(d_pre, (B, T, M), "d_pre", dev, "decoder_backward"), _cot(d_post, (B, T, M), "d_post", dev, "decoder_backward")
    d_stop = _cot(d_stop, (B, T), "d_stop", dev, "decoder_backward")
    tape.used = True
    contract.prepare_grads(_decoder_params(model), accumulate)
    po = model.postnet
    p_pre, p_post = float(model.prenet.p), float(po.p)

    # ---- batched before the loop: the post-net into d_outputs, the head, dropout1, tanh, the projection -----------------------------------------
    d_head = torch.zeros(B, T, ldh, dtype=_F32, device=dev)
    if d_post is not None:
        dpf = torch.zeros(B, T + 1, M, dtype=_F32, device=dev)
        dpf[:, 1:].copy_(d_post)
        dy = contract.conv_grads(dpf.view(N1, M), tape.xs[4], B, T + 1, P.post_out[0], P.post_out[2], 4)
        bn_ws = torch.empty(512, dtype=torch.float64, device=dev)
        for k in (3, 2, 1, 0):
            wpair, _, conv, bn = P.post[k]
            dz = buf(N1, 256, dev=dev)
            ops.bn_bwd(dy, tape.zs[k], tape.mean[k], tape.rstd[k], bn.weight, bn.bias, dz, bn.weight.grad, bn.bias.grad, bn_ws, 2, drop_p=p_post, seed=seed,
                       stream_id=S_POST + k)
            dy = contract.conv_grads(dz, tape.xs[k], B, T + 1, wpair, conv, 4)
        ops.add_inplace(dpf, dy)                                                            # outputs + postnet(outputs): the residual's share
        d_head[:, :, :M].copy_(dpf[:, 1:])                                                  # (the go frame's gradient is dropped: a constant)
    if d_pre is not None:
        d_head[:, :, :M].add_(d_pre)
    if d_stop is not None:
        d_head[:, :, M].copy_(d_stop)
    dhp = contract.parts(d_head.view(N, ldh))
    gW, gb = torch.zeros(ldh, 256, dtype=_F32, device=dev), torch.zeros(ldh, dtype=_F32, device=dev)
    contract.wgrad_rows(dhp, ALL, tape.o, contract.resid_of(tape.o), gW, (gb,))
    po.linear_project.weight.grad.add_(gW[:M])
    po.linear_project.bias.grad.add_(gb[:M])
    po.stop_linear.weight.grad.add_(gW[M:M + 1])
    po.stop_linear.bias.grad.add_(gb[M:M + 1])
    d_o = contract.dgrad_rows(dhp, P.head[0], buf(N, 256, dev=dev))
    dg0p, d_enc, d_h, d_c = _loop_backward(tape, d_o, mark)
    # the prenet (shared with the encoder)
    d_p = contract.dgrad_rows(dg0p, P.w_ih0_p, buf(N, 256, dev=dev))
    (w1, _, fc1), (w2, _, fc2) = P.fcs
    ops.relu_bwd(d_p, tape.pre_act)
    dpp = contract.parts(d_p)
    contract.wgrad_rows(dpp, ALL, tape.h1, contract.resid_of(tape.h1), fc2.weight.grad, (fc2.bias.grad,))
    dh1p = contract.dgrad_rows(dpp, w2, buf(N, tape.h1.shape[1], dev=dev))
    da1 = torch.empty_like(dh1p)
    ops.leaky_dropout(tape.a1, dh1p, da1, 0.0, p_pre, seed, S_DPRE)
    contract.wgrad_rows(contract.parts(da1), ALL, tape.feed, contract.resid_of(tape.feed), fc1.weight.grad, (fc1.bias.grad,))
    return d_enc, d_h, d_c


def _loop_backward(tape, d_o, mark):
    """Backward of _loop_forward, shared by both decoders: d_o [B*T,256] = the gradient of the head's input.  Writes the gradients of
    model.decoder's parameters (all of W_ih_l0 included: its first 256 columns contract with the prenet rows on the tape).  Returns
    (dg0p, d_enc_output, d_h, d_c): dg0p = contract.parts of layer 0's gate gradients [B*T,1024] -- the caller's prenet gradient is
    dg0p . W_ih_l0[:, :256] -- and the three cotangents encoder_backward takes."""
    model, P, B, T, Tk, seed, lens = tape.model, tape.P, tape.B, tape.T, tape.Tk, tape.seed, tape.lens
    A, lsa, N = P.A, P.mode == ops.ATTN_LSA, B * T
    dev = tape.enc.device
    dec = model.decoder
    p_dec = float(dec.p)
    if p_dec > 0.0:
        d_od = torch.empty_like(d_o)
        ops.leaky_dropout(d_o, d_o, d_od, 1.0, p_dec, seed, S_DOUT)                         # slope 1: the mask and its 1/(1-p) only
        d_o = d_od
    dzp = contract.parts(ops.tanh_bwd(d_o, tape.tz))
    HC2 = tape.HC.view(N, 768)
    HC2res = contract.resid_of(HC2)
    contract.wgrad_rows(dzp, ALL, HC2, HC2res, P.proj_lin.weight.grad, (P.proj_lin.bias.grad,))
    DHC = contract.dgrad_rows(dzp, P.proj[0], buf(N, 768, dev=dev)).view(B, T, 768)         # [d_h1 | d_ctx] of the projection, all positions

    # ---- the loop, i = T-1 .. 0: 7 launches per position --------------------------------------------------------------------------------------------
    z = lambda *s: torch.zeros(*s, dtype=_F32, device=dev)                                  # noqa: E731
    Tkp = tape.W.shape[2]
    dh0, dh1, dc0, dc1 = z(B, 256), z(B, 256), z(B, 256), z(B, 256)
    DG0, DG1 = buf(B, T, 1024, dev=dev), buf(B, T, 1024, dev=dev)
    DCTX, DQ = buf(B, T, 512, dev=dev), buf(B, T, A, dev=dev)
    d_mem, dv_part = z(B, Tk, A), z(B, A)
    dd_part, dcv_part = (z(B, A, 32), z(B, 32, 2, 31)) if lsa else (None, None)
    dprev, dcum = ([z(B, Tkp), z(B, Tkp)], [z(B, Tkp), z(B, Tkp)]) if lsa else ([None, None], [None, None])
    ws = ops.rnn_attn_step_bwd_ws(B, Tk, A, dev)
    t256, dh_att = buf(B, 256, dev=dev), buf(B, 256, dev=dev)
    W, CUM, HC, S0, S1, F1, h0, c0 = tape.W, tape.CUM, tape.HC, tape.S0, tape.S1, tape.F1, tape.h0, tape.c0
    sl = lambda t: t[:, :Tk] if t is not None else None                                     # noqa: E731
    if mark is not None:
        mark("loop_begin")
    for i in range(T - 1, -1, -1):
        cur, nxt = (T - 1 - i) & 1, (T - i) & 1
        ops.lstm_cell_bwd(S1[:, i], S1[:, i - 1, 4] if i else c0[1], DG1[:, i], dc1, dh=dh1, dh2=DHC[:, i, :256], dc_in=dc1)
        ops.rnn_linear(DG1[:, i], P.wt_ih1, None, t256)                                     # dG1 W_ih_l1: layer 0's output gradient, masked below
        ops.lstm_cell_bwd(S0[:, i], S0[:, i - 1, 4] if i else c0[0], DG0[:, i], dc0, dh=dh0, dh2=t256, mask=F1[:, i] if F1 is not None else None, dc_in=dc0)
        ops.rnn_linear(DG0[:, i], P.wt_ihc0, None, DCTX[:, i], R=DHC[:, i, 256:])           # d_ctx = the projection's share + dG0 W_ih_l0[:, 256:]
        q = HC[:, i - 1, :256] if i else h0[1]
        ops.rnn_attn_step_bwd(P.mode, DCTX[:, i], W[:, i + 1, :Tk], q, P.Wq, tape.mem, P.v, tape.enc, lens, dh_att, DQ[:, i], d_mem, dv_part, ws,
                              prev=W[:, i, :Tk], cum=CUM[:, i, :Tk] if lsa else None, conv_w=P.conv_w, dense_w=P.dense_w, d_w_a=sl(dprev[cur]),
                              d_w_b=sl(dcum[cur]), carry=True, ddense_part=dd_part, dconv_part=dcv_part, d_prev=sl(dprev[nxt]), d_cum=sl(dcum[nxt]))
        ops.rnn_linear(DG1[:, i], P.wt_hh1, None, dh1, R=dh_att)                            # the query was h1_{i-1}: its gradient joins layer 1's carry
        ops.rnn_linear(DG0[:, i], P.wt_hh0, None, dh0)
    if mark is not None:
        mark("loop_end")

    # ---- batched after the loop: every weight and bias gradient, the prenet, the memory side ---------------------------------------------------------
    r = dec.rnn
    dg0p, dg1p = contract.parts(DG0.view(N, 1024)), contract.parts(DG1.view(N, 1024))
    pre = tape.pre_act
    contract.wgrad_rows(dg0p, ALL, pre, contract.resid_of(pre), r.weight_ih_l0.grad[:, :256], (r.bias_ih_l0.grad, r.bias_hh_l0.grad))
    contract.wgrad_rows(dg0p, ALL, HC2[:, 256:], HC2res[:, 256:], r.weight_ih_l0.grad[:, 256:])
    h0prev = tape.H0[:, :T].contiguous().view(N, 256)
    contract.wgrad_rows(dg0p, ALL, h0prev, contract.resid_of(h0prev), r.weight_hh_l0.grad)
    x1 = (tape.H0d if F1 is not None else tape.H0[:, 1:].contiguous()).view(N, 256)
    contract.wgrad_rows(dg1p, ALL, x1, contract.resid_of(x1), r.weight_ih_l1.grad, (r.bias_ih_l1.grad, r.bias_hh_l1.grad))
    qry = torch.cat([h0[1][:, None, :], HC[:, :T - 1, :256]], 1).contiguous().view(N, 256)  # h1 before each position: W_hh_l1's input and the queries
    qry_res = contract.resid_of(qry)
    contract.wgrad_rows(dg1p, ALL, qry, qry_res, r.weight_hh_l1.grad)
    contract.wgrad_rows(contract.parts(DQ.view(N, A)), ALL, qry, qry_res, P.q_lin.weight.grad)
    _add_over_b(dv_part, P.v_lin.weight.grad)
    if lsa:
        _add_over_b(dd_part, P.dense_lin.weight.grad)
        _add_over_b(dcv_part, P.conv_mod.weight.grad)
    # the memory side: dW_mem = d_mem^T enc, d_enc = d_mem W_mem + per sequence w_b^T [Tk,T] . d_ctx_b [T,512] (formed once, after the loop)
    enc2 = tape.enc.view(B * Tk, 512)
    dmp = contract.parts(d_mem.view(B * Tk, A))
    contract.wgrad_rows(dmp, ALL, enc2, contract.resid_of(enc2), P.mem_lin.weight.grad)
    d_enc = contract.dgrad_rows(dmp, P.Wmem, buf(B * Tk, 512, dev=dev)).view(B, Tk, 512)
    wparts = contract.parts(W[:, 1:])
    dctx_res = contract.resid_of(DCTX)
    for b in range(B):
        contract.wgrad_rows(tuple(t[b] for t in wparts), slice(0, Tk), DCTX[b], dctx_res[b], d_enc[b])
    return dg0p, d_enc, torch.stack([dh0, dh1]), torch.stack([dc0, dc1])


# ==== TextRNN decoder: teacher-forced train-mode decode_sequence (src/network.py:539-575) and its backward; DESIGN 5k ==============================
# TextRNN.decode runs TextPrenet over the whole prefix at every position and keeps the last row: position 0 sees [SOS], position i >= 1 sees
# target[:, :i] (no SOS), each call with its own dropout masks, its own batch statistics over the B * L_i rows of that prefix (PAD included) and
# its own running-statistics update.  All prefixes are computed before the loop in one slab of rows (prefix_layout); csrc/prefix.hip.
S_TEMB, S_TPRE, S_TPOST = 16, 17, 20               # the slab's emb_dropout, dropout1..3 (17..19), TextPostnet.dropout1
GAP = 2                                            # zero rows after every sequence of the slab: a 5-tap conv's padding on either side
MAX_SLAB_BYTES = 0x7FFFFFF0                        # rows * 256 channels * 4 bytes: the kernels' 32-bit row arithmetic and buffer ranges

PrefixLayout = collections.namedtuple("PrefixLayout", "off lens total")


def prefix_layout(B, T):
    """The prefix slab's geometry.  Segment s = 0..T-1 is position s's prenet input: B sequences of lens[s] = max(s, 1) live rows ([SOS] at
    s = 0, target[b, 0:s] after that), each followed by GAP = 2 zero rows, sequences b = 0..B-1 back to back:

        row(s, b, j) = off[s] + b * (lens[s] + GAP) + j,   0 <= j < lens[s] live,   j = lens[s], lens[s] + 1 the gap

    Segments follow one another without further padding (off[s+1] = off[s] + B * (lens[s] + GAP)); total = off[T-1] + B * (lens[T-1] + GAP) rows.
    Read as ONE sequence of `total` rows, the slab gives a 5-tap 'same' convolution exactly the zero padding every prefix had on its own."""
    if B < 1 or T < 1:
        raise ValueError("prefix_layout: B >= 1 and T >= 1")
    lens = [max(s, 1) for s in range(T)]
    off, r = [], 0
    for L in lens:
        off.append(r)
        r += B * (L + GAP)
    return PrefixLayout(off, lens, r)


_PREFIX_TABLES = {}
PrefixTables = collections.namedtuple("PrefixTables", "B T rows nchunks segoff chunks chunk_start")
PREFIX_CHUNK = 64                                  # rows per workgroup of the slab kernels (csrc/prefix.hip PFX_CHUNK)


def prefix_tables(B, T, dev):
    """The device-side tables of csrc/prefix.hip for prefix_layout(B, T): segoff [T+1], chunks [nchunks, 2] = {segment, first row} of runs of
    at most 64 rows that stay inside one segment, chunk_start [T+1] = the first chunk of each segment."""
    key = (B, T, str(dev))
    t = _PREFIX_TABLES.get(key)
    if t is None:
        lay = prefix_layout(B, T)
        chunks, start = [], []
        for s in range(T):
            start.append(len(chunks))
            end = lay.off[s] + B * (lay.lens[s] + GAP)
            chunks.extend((s, r) for r in range(lay.off[s], end, PREFIX_CHUNK))
        start.append(len(chunks))
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)                          # noqa: E731
        if len(_PREFIX_TABLES) >= 16:
            _PREFIX_TABLES.clear()
        t = _PREFIX_TABLES[key] = PrefixTables(B, T, lay.total, len(chunks), i32(lay.off + [lay.total]), i32(chunks).view(-1, 2).contiguous(), i32(start))
    return t


@torch.no_grad()
def text_decoder_forward(model, target, enc_outputs, lens_k, seed=0, mark=None):
    """Train-mode, teacher-forced TextRNN.decode_sequence (teacher_ratio = 1): target [B,T] int64 on the GPU, enc_outputs = ((h, c)
    [2,B,256], enc_output [B,Tk,512]) or an encoder Tape of either side, lens_k the live keys per sequence (1..Tk).  2 <= B (one row cannot be
    normalised: the reference raises at position 0), 1 <= T <= 512.  Returns a DecoderTape: .logits [B,T,len(symbols)].  Updates the prenet's
    BatchNorm running statistics T times each (num_batches_tracked += T) and drops the model's cached eval operands.  mark (optional): called
    with 'prefix_begin' / 'prefix_end' around the prefix prenet and 'loop_begin' / 'loop_end' around the position loop."""
    from .network import TextRNN
    if not isinstance(model, TextRNN):
        raise TypeError("text_decoder_forward: model must be a unast_amd.network.TextRNN (decoder_forward trains a SpeechRNN)")
    if not model.training:
        raise RuntimeError("text_decoder_forward is the train-mode entry point: call model.train() first (model.decode_sequence() is the eval forward)")
    if not torch.is_tensor(target) or target.dim() != 2:
        raise ValueError("text_decoder_forward: target must be an int64 tensor [B,T]")
    B, T = target.shape
    if B < 2:
        raise ValueError("text_decoder_forward: B >= 2 -- position 0 normalises B rows with batch statistics, one row cannot be normalised "
                         "(the reference raises 'Expected more than 1 value per channel')")
    if not 1 <= T <= 512:
        raise ValueError("text_decoder_forward: 1 <= T <= 512 (got %d)" % T)
    lay = prefix_layout(B, T)
    if lay.total * 256 * 4 >= MAX_SLAB_BYTES:
        raise ValueError("text_decoder_forward: the prefix slab of B = %d, T = %d has %d rows; rows * 1024 bytes must stay below 2 GiB" % (B, T, lay.total))
    ids = model._ids(target)
    dev = ids.device
    tape = _begin_decoder_tape("text_decoder_forward", model, TextDecoderPack, enc_outputs, lens_k, B, T, seed, dev)
    P, N, R = tape.P, B * T, lay.total
    ids = model._ids(ids, P).contiguous()
    tabs = prefix_tables(B, T, dev)
    p_pre, p_post = float(model.prenet.p), float(model.postnet.p)

    # ---- the prefix prenet: every stage once over the slab ------------------------------------------------------------------------------------
    if mark is not None:
        mark("prefix_begin")
    E = P.emb.shape[1]
    x0 = buf(R, E, dev=dev)
    ops.prefix_embed_fwd(ids, P.emb, tabs, x0, SOS_IDX, drop_p=p_pre, seed=seed, stream_id=S_TEMB)
    tape.site("t_emb_dropout", p_pre, S_TEMB, R, E)
    tape.ids, tape.tabs = ids, tabs
    tape.xs, tape.zs = [x0], []
    tape.mean, tape.rstd = buf(3, T, 256, dev=dev), buf(3, T, 256, dev=dev)
    varu = buf(T, 256, dev=dev)
    ws = ops.prefix_bn_ws(tabs, 256, dev)
    pre = buf(B, T, 256, dev=dev)
    cur = x0
    for i, (wp, bias, _, bn) in enumerate(P.convs):
        contract.check_bn(bn, "text_decoder_forward")
        z = contract.conv(cur.view(1, R, -1), wp, bias, 2).view(R, 256)                     # the gaps are every neighbour's zero padding
        y = buf(R, 256, dev=dev) if i < 2 else None
        ops.prefix_bn_fwd(z, tabs, bn.weight, bn.bias, tape.mean[i], tape.rstd[i], varu, ws, y=y, p_last=pre if i == 2 else None,
                          running_mean=bn.running_mean, running_var=bn.running_var, num_batches_tracked=bn.num_batches_tracked, eps=bn.eps,
                          momentum=bn.momentum, drop_p=p_pre, seed=seed, stream_id=S_TPRE + i)
        tape.site("t_dropout%d" % (i + 1), p_pre, S_TPRE + i, R, 256)
        tape.zs.append(z)
        if y is not None:
            tape.xs.append(y)
            cur = y
    rnn.drop_eval_pack(model)
    if mark is not None:
        mark("prefix_end")

    o = _loop_forward(tape, pre.view(N, 256), mark)

    # ---- TextPostnet: its own dropout1 on top of the decoder's, then fc1 ---------------------------------------------------------------------------
    o2 = o
    if p_post > 0.0:
        o2 = torch.empty_like(o)
        ops.leaky_dropout(o, None, o2, 1.0, p_post, seed, S_TPOST)
    tape.site("t_post_dropout", p_post, S_TPOST, N, 256)
    tape.o2 = o2
    tape.head = contract.linear_rows(o2, P.head[0], P.head[1])                              # [N, ldh] padded logits: what the loss kernels read
    tape.logits = tape.head.view(B, T, P.ldh)[:, :, :P.V].contiguous()
    return tape


@torch.no_grad()
def text_decoder_backward(tape, d_logits, accumulate=False, mark=None):
    """Backward of text_decoder_forward for the scalar whose gradient with respect to logits [B,T,V] is given.  Writes p.grad of exactly the
    parameters under model.prenet, model.decoder and model.postnet (overwritten, or added to with accumulate=True; an existing dense fp32
    .grad is kept in place).  Returns (d_enc_output [B,Tk,512], d_h, d_c [2,B,256]), the cotangents encoder_backward takes.  A tape is used once.
    mark: as text_decoder_forward's."""
    if not isinstance(tape, DecoderTape) or getattr(tape, "entry", None) != "text_decoder_forward":
        raise TypeError("text_decoder_backward: tape must come from text_decoder_forward")
    if tape.used:
        raise RuntimeError("text_decoder_backward: this tape has been used; run text_decoder_forward again")
    model, P, B, T, seed, tabs = tape.model, tape.P, tape.B, tape.T, tape.seed, tape.tabs
    N, R, V, ldh = B * T, tabs.rows, P.V, P.ldh
    dev = tape.enc.device
    d_logits = _cot(d_logits, (B, T, V), "d_logits", dev, "text_decoder_backward")
    if d_logits is None:
        raise ValueError("text_decoder_backward: d_logits must be a float32 CUDA tensor %s" % ((B, T, V),))
    tape.used = True
    contract.prepare_grads(_decoder_params(model), accumulate)
    p_pre, p_post = float(model.prenet.p), float(model.postnet.p)
    fc = model.postnet.fc1

    d_head = torch.zeros(B, T, ldh, dtype=_F32, device=dev)
    d_head[:, :, :V].copy_(d_logits)
    dhp = contract.parts(d_head.view(N, ldh))
    gW, gb = torch.zeros(ldh, 256, dtype=_F32, device=dev), torch.zeros(ldh, dtype=_F32, device=dev)
    contract.wgrad_rows(dhp, ALL, tape.o2, contract.resid_of(tape.o2), gW, (gb,))
    fc.weight.grad.add_(gW[:V])
    fc.bias.grad.add_(gb[:V])
    d_o = contract.dgrad_rows(dhp, P.head[0], buf(N, 256, dev=dev))
    if p_post > 0.0:
        d_od = torch.empty_like(d_o)
        ops.leaky_dropout(d_o, d_o, d_od, 1.0, p_post, seed, S_TPOST)
        d_o = d_od
    dg0p, d_enc, d_h, d_c = _loop_backward(tape, d_o, mark)

    # ---- the prefix prenet: d_P sits on each prefix's last row and spreads through the statistics to every row of the prefix -------------------------
    if mark is not None:
        mark("prefix_begin")
    dy = contract.dgrad_rows(dg0p, P.w_ih0_p, buf(N, 256, dev=dev)).view(B, T, 256)
    ws = ops.prefix_bn_ws(tabs, 256, dev)
    for i in (2, 1, 0):
        wpair, _, conv, bn = P.convs[i]
        dz = buf(R, 256, dev=dev)
        ops.prefix_bn_bwd(dy, tape.zs[i], tabs, tape.mean[i], tape.rstd[i], bn.weight, bn.bias, dz, bn.weight.grad, bn.bias.grad, ws, last_only=(i == 2),
                          drop_p=p_pre, seed=seed, stream_id=S_TPRE + i)
        dy = contract.conv_grads(dz, tape.xs[i], 1, R, wpair, conv, 2)                      # its gap rows hold the neighbours' spill: nobody reads them
    emb = model.prenet.embed
    G = buf(B, T + 1, dy.shape[1], dev=dev)
    ops.prefix_embed_bwd(dy, tabs, G, drop_p=p_pre, seed=seed, stream_id=S_TEMB)
    ids_ext = torch.cat([torch.full((B, 1), SOS_IDX, dtype=torch.int64, device=dev), tape.ids], 1).contiguous()
    ops.embed_bwd(ids_ext, G.view(B * (T + 1), -1), emb.weight.grad, T + 1, padding_idx=emb.padding_idx if emb.padding_idx is not None else -1)
    if mark is not None:
        mark("prefix_end")
    return d_enc, d_h, d_c


# ==== greedy generation in TRAIN mode: infer_sequence under UNAST.cm_speech_in / cm_text_in (src/network.py:103-123, 312-349, 586-617); DESIGN 5m =========
# The modules are in train() under no_grad, so every dropout is live inside the decoding loop, TextPrenet normalises each generated prefix
# [SOS, c_0 .. c_{i-1}] with that prefix's own batch statistics (one momentum update per position), and the speech post-net runs on batch
# statistics over all generated frames.  No backward, no tape: the per-position buffers are scratch.  The loop is eager; the host knows the
# position and reads the device-side `running` flag back every SYNC_EVERY positions.  Positions launched after every sequence has stopped write
# neither tokens, frames, lengths, running statistics nor num_batches_tracked (the flag gates them on the device), so the results do not depend
# on SYNC_EVERY.  Mask sites 21..34; a site's mask row is (position, sequence): i * B + b for the [B,256] rows of a position, and
# B * L (L - 1) / 2 + b * L + j for row j of sequence b's prefix of length L = i + 1 (the rows of all shorter prefixes come first).
SYNC_EVERY = 8
S_GEMB, S_GPRE, S_GDROP, S_GOUT, S_GPOST = 21, 22, 25, 26, 27          # text: emb_dropout, dropout1..3 (22..24), nn.LSTM inter-layer, dropout1, TextPostnet.dropout1
S_SGPRE, S_SGDROP, S_SGOUT, S_SGPOST = 28, 29, 30, 31                  # speech: prenet dropout, nn.LSTM inter-layer, dropout1, the four post-net dropouts (31..34)


class Generated(tuple):
    """What a train-mode generation returns: the reference's tuple, plus .lens_host (list), .steps (positions the host launched), .sites (the mask
    sites, as a tape lists them), .max_len and -- text -- .live_pad (PAD ids inside a sequence's length)."""


def prefix_row0(B, L):
    """The first mask row of the prefix of length L: the rows of the prefixes of lengths 1 .. L-1 come before it."""
    return B * (L * (L - 1) // 2)


class _GenState:
    """The position loop's scratch, shared by both generations: the attention state and the two LSTM cells, each ping-ponged between positions."""

    def __init__(self, tape, max_len, stream_drop):
        P, B, Tk, dev = tape.P, tape.B, tape.Tk, tape.enc.device
        self.tape, self.lsa = tape, P.mode == ops.ATTN_LSA
        Tkp = (Tk + 3) // 4 * 4
        z = lambda *s: torch.zeros(*s, dtype=_F32, device=dev)                              # noqa: E731
        self.cell = _TrainCell(tape)
        self.W, self.CUM = z(2, B, Tkp), (z(2, B, Tkp) if self.lsa else None)
        self.HC, self.H0, self.H0d = z(2, B, 768), z(2, B, 256), buf(B, 256, dev=dev)
        self.S0, self.S1 = z(2, B, 5, 256), z(2, B, 5, 256)
        self.H0[0].copy_(tape.h0[0])
        W, CUM, HC, H0, S0, S1 = self.W, self.CUM, self.HC, self.H0, self.S0, self.S1
        # where the cell's rows live at even and at odd positions (c = i & 1, p the other half); H0[c] = layer 0's h before position i
        self.halves = [(HC[p, :, :256], W[p, :, :Tk], W[c, :, :Tk], CUM[p, :, :Tk] if self.lsa else None, CUM[c, :, :Tk] if self.lsa else None, HC[c, :, 256:],
                        H0[c], H0[p], S0[c], S0[p, :, 4], S1[c], S1[p, :, 4], HC[c, :, :256]) for c, p in ((0, 1), (1, 0))]
        self.xp0, self.tz, self.o = buf(B, 1024, dev=dev), buf(B, 256, dev=dev), buf(B, 256, dev=dev)
        self.p_dec = float(tape.model.decoder.p)
        self.F1 = _drop_factor(self.p_dec, tape.seed, stream_drop, max_len * B, 256, dev).view(max_len, B, 256) if self.p_dec > 0.0 else None
        tape.site("g_drop0", self.p_dec, stream_drop, max_len * B, 256)
        self.stop_lens = torch.full((B,), max_len, dtype=torch.int64, device=dev)
        self.running = torch.ones((), dtype=torch.int32, device=dev)

    def step(self, i, pre):
        """RNNDecoder on position i from the prenet's rows pre [B,256] up to the projection: xp0's row, the cell, the projection (9 launches);
        leaves [h1 | ctx] in HC[i & 1] and returns the projection's pre-activation [B,256]."""
        P, F1 = self.tape.P, self.F1
        ops.rnn_linear(pre, P.w_ih0_p[0], P.bias[0], self.xp0)
        self.cell(i == 0, self.xp0, F1[i] if F1 is not None else None, self.H0d if F1 is not None else None, *self.halves[i & 1])
        return ops.rnn_linear(self.HC[i & 1], P.proj[0][0], P.proj[1], self.tz)


def _begin_generation(what, model, cls, pack_cls, enc_outputs, lens_k, max_len, seed):
    if not isinstance(model, cls):
        raise TypeError("%s: model must be a unast_amd.network.%s" % (what, cls.__name__))
    if not model.training:
        raise RuntimeError("%s generates in train mode (dropout and batch statistics live): call model.train() first (model.infer_sequence() is the "
                           "eval generation)" % what)
    max_len = int(max_len)
    if not 1 <= max_len <= 2048:
        raise ValueError("%s: 1 <= max_len <= 2048 (got %d)" % (what, max_len))
    enc = enc_outputs.enc_output if isinstance(enc_outputs, Tape) else enc_outputs[1]
    if not torch.is_tensor(enc) or enc.dim() != 3:
        raise ValueError("%s: enc_outputs must be ((h, c), enc_output [B,Tk,512]) or an encoder tape" % what)
    B = enc.shape[0]
    if B < 2:
        raise ValueError("%s: B >= 2 -- position 0 normalises B rows with batch statistics, one row cannot be normalised "
                         "(the reference raises 'Expected more than 1 value per channel')" % what)
    return _begin_decoder_tape(what, model, pack_cls, enc_outputs, lens_k, B, max_len, seed, enc.device), B, max_len


def _run_positions(st, max_len, one):
    """one(i) launches position i; the running flag is read back every SYNC_EVERY positions.  Returns the number of positions launched."""
    steps = 0
    for i in range(max_len):
        one(i)
        steps = i + 1
        if steps % SYNC_EVERY == 0 and steps < max_len and not int(st.running.item()):
            break
    return steps


@torch.no_grad()
def text_generate_train(model, enc_outputs, lens_k, max_len=300, seed=0):
    """TextRNN.infer_sequence with the modules in train mode (what UNAST.cm_speech_in runs under no_grad): enc_outputs = ((h, c) [2,B,256],
    enc_output [B,Tk,512]) or an encoder tape of either side, lens_k the live keys per sequence.  Returns Generated((tokens [B,T] int64, PAD past each
    sequence's length, lens [B] int64)): T = max(lens) positions ran, a sequence that never drew EOS has length max_len.  The prenet's three
    BatchNorms take T momentum updates (num_batches_tracked += T); the model's cached eval operands are dropped."""
    from .network import TextRNN
    what = "text_generate_train"
    tape, B, max_len = _begin_generation(what, model, TextRNN, TextDecoderPack, enc_outputs, lens_k, max_len, seed)
    P, dev = tape.P, tape.enc.device
    E = P.emb.shape[1]
    if E % 64 or E > 256:
        raise NotImplementedError("%s: an embedding width that is a multiple of 64, at most 256 (got %d)" % (what, E))
    bns = [bn for _, _, _, bn in P.convs]
    for bn in bns:
        contract.check_bn(bn, what)
    p_pre, p_post = float(model.prenet.p), float(model.postnet.p)
    st = _GenState(tape, max_len, S_GDROP)
    rows = B * max_len
    tape.site("g_emb_dropout", p_pre, S_GEMB, prefix_row0(B, max_len + 1), E)
    for k in range(3):
        tape.site("g_dropout%d" % (k + 1), p_pre, S_GPRE + k, prefix_row0(B, max_len + 1), 256)
    tape.site("g_dropout_out", st.p_dec, S_GOUT, rows, 256)
    tape.site("g_post_dropout", p_post, S_GPOST, rows, 256)
    tokens = torch.zeros(B, max_len, dtype=torch.int64, device=dev)
    zs = [buf(rows, 256, dev=dev) for _ in range(3)]
    parts = torch.empty(3 * ops.prefix_gen_tiles(B, max_len) * 512, dtype=torch.float64, device=dev)
    pre, o2, logits = buf(B, 256, dev=dev), buf(B, 256, dev=dev), buf(B, P.ldh, dev=dev)
    Ws = [(wp[0], bias) for wp, bias, _, _ in P.convs]

    def one(i):
        L = i + 1
        row0 = prefix_row0(B, L)
        part = parts[:3 * ops.prefix_gen_tiles(B, L) * 512].view(3, -1, 2, 256)
        ops.prefix_gen_conv(Ws[0][0], Ws[0][1], zs[0], part[0], B, L, tokens=tokens, emb=P.emb, sos=SOS_IDX, drop_p=p_pre, seed=seed, stream_id=S_GEMB, row0=row0)
        for k in (1, 2):
            bn = bns[k - 1]
            ops.prefix_gen_conv(Ws[k][0], Ws[k][1], zs[k], part[k], B, L, x=zs[k - 1], part_in=part[k - 1], bn=(bn.weight, bn.bias, bn.eps), drop_p=p_pre,
                                seed=seed, stream_id=S_GPRE + k - 1, row0=row0)
        ops.prefix_gen_finish(zs[2], part, bns, pre, B, L, running=st.running, drop_p=p_pre, seed=seed, stream_id=S_GPRE + 2, row0=row0)
        tz = st.step(i, pre)
        ops.prefix_gen_act_drop(tz, o2, ops.PGEN_TANH, drop_a=st.p_dec, stream_a=S_GOUT, drop_b=p_post, stream_b=S_GPOST, seed=seed, row0=i * B)
        ops.rnn_linear(o2, P.head[0][0], P.head[1], logits)
        ops.prefix_gen_end_text(logits, P.V, tokens, i, st.stop_lens, max_len, EOS_IDX, st.running)

    steps = _run_positions(st, max_len, one)
    rnn.drop_eval_pack(model)
    host = torch.cat([st.stop_lens.view(B, 1), tokens[:, :steps]], 1).cpu()                 # the one read-back after the loop: lengths and tokens
    lens_host = [int(v) for v in host[:, 0]]
    T = max(lens_host)
    live = torch.arange(T)[None, :] < host[:, :1]
    out = Generated((tokens[:, :T] * live.to(dev), st.stop_lens))
    out.lens_host, out.steps, out.sites, out.max_len = lens_host, steps, tape.sites, max_len
    out.live_pad = int(((host[:, 1:T + 1] == PAD_IDX) & live).sum())
    return out


@torch.no_grad()
def speech_generate_train(model, enc_outputs, lens_k, max_len=815, seed=0):
    """SpeechRNN.infer_sequence with the modules in train mode (what UNAST.cm_text_in runs under no_grad).  Returns Generated((pre, post [B,T,M],
    stop [B,T], lens [B] int64)), zero past each sequence's length: T = max(lens), a sequence whose stop logit never reached sigmoid >= .5 has
    length max_len.  The post-net runs once over all B (T+1) frames, go frame and stopped sequences' frames included, and is masked afterwards
    (its BatchNorms take one update); the model's cached eval operands are dropped."""
    from .network import SpeechRNN
    what = "speech_generate_train"
    tape, B, max_len = _begin_generation(what, model, SpeechRNN, DecoderPack, enc_outputs, lens_k, max_len, seed)
    P, dev, M = tape.P, tape.enc.device, tape.P.M
    p_pre = float(model.prenet.p)
    st = _GenState(tape, max_len, S_SGDROP)
    rows = B * max_len
    (w1, b1, _), (w2, b2, _) = P.fcs
    tape.site("g_prenet_dropout", p_pre, S_SGPRE, rows, w1[0].shape[0])
    tape.site("g_dropout_out", st.p_dec, S_SGOUT, rows, 256)
    frames = torch.zeros(B, max_len + 1, M, dtype=_F32, device=dev)                         # position 0 = the all-zero go frame
    stops = torch.zeros(B, max_len, dtype=_F32, device=dev)
    a1, h1, pre = buf(B, w1[0].shape[0], dev=dev), buf(B, w1[0].shape[0], dev=dev), buf(B, 256, dev=dev)
    head = buf(B, P.ldh, dev=dev)

    def one(i):
        ops.rnn_linear(frames[:, i], w1[0], b1, a1)
        ops.prefix_gen_act_drop(a1, h1, ops.PGEN_RELU, drop_a=p_pre, stream_a=S_SGPRE, seed=seed, row0=i * B)
        ops.rnn_linear(h1, w2[0], b2, pre, act=1)
        tz = st.step(i, pre)
        ops.prefix_gen_act_drop(tz, st.o, ops.PGEN_TANH, drop_a=st.p_dec, stream_a=S_SGOUT, seed=seed, row0=i * B)
        ops.rnn_linear(st.o, P.head[0][0], P.head[1], head)
        ops.prefix_gen_end_speech(head, M, frames, stops, i, st.stop_lens, max_len, st.running)

    steps = _run_positions(st, max_len, one)
    lens_host = [int(v) for v in st.stop_lens.tolist()]                                     # the one read-back after the loop
    T = max(lens_host)
    outs = frames[:, :T + 1].contiguous()
    post = _postnet_forward(tape, outs, S_SGPOST, what)
    live = (torch.arange(T, device=dev)[None, :] < st.stop_lens[:, None]).to(_F32)
    out = Generated((outs[:, 1:] * live[:, :, None], post[:, 1:] * live[:, :, None], stops[:, :T] * live, st.stop_lens))
    out.lens_host, out.steps, out.sites, out.max_len = lens_host, steps, tape.sites, max_len
    return out
