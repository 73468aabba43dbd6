"""The RNN model family's eval path (TextRNN / SpeechRNN, src/network.py:279-402, 503-624; src/module.py:297-497) on HIP kernels.

Built for the configuration every full-size reference config uses: hidden = e_in = t_emb_dim = s_pre_hid = 256, two layers, a bidirectional
encoder, Luong or location-sensitive attention of width <= 64; eval mode under torch.no_grad() only (unast_amd.network refuses the rest).

Encoder: per layer one GEMM for X W_ih^T of both directions and one unast_lstm_seq_fwd launch (csrc/rnn.hip).  Decoder: one step function
for a position, state in device memory (position, LSTM states, attention state), so that it can be captured once as a HIP graph and replayed
(unast_amd.inference._Generation, config.DECODE_GRAPH).  Teacher-forced decoding is the same step fed from the target buffer with the stop
rule off.  What the kernels read is a derived, cached copy of the parameters (`Pack`), rebuilt when a parameter's or buffer's version counter
moves: eval BatchNorm folded into tap-major conv weights, W_ih of both encoder directions as one matrix, W_hh in MFMA fragment order,
[linear_project | stop_linear] as one head, and beside each GEMM / conv weight the residual the split-bf16 operand preparation drops.
The train packs of unast_amd.train_rnn derive the same operands through the extractors in front of `Pack` and live in the same version-keyed
cache (`contract.cached_operands`, one slot of PACK_SLOTS per pack); each pack adds only what its own kernels read.
Every contraction keeps fp32-level products (greedy trajectories are held to the reference's own fp32 error): unast_rnn_linear for the few rows of a
step, the three-launch split form (unast_amd.contract: linear_rows, conv) around the many-row GEMMs and convs.
"""
import torch

from . import contract, ops
from .contract import buf, detached
from .inference import _Generation, _exit_step
from .utils import SOS_IDX, EOS_IDX, PAD_IDX

_F32 = torch.float32
WINDOW = 7            # prefix positions the last position of three 5-tap convs depends on (src/network.py:573)


# ---- what the eval pack and the train packs (unast_amd.train_rnn) derive alike: each function returns the common part, a pack adds its own --------
LSTM_NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def encoder_layers(enc):
    """RNNEncoder's LSTM, layer by layer (a generator: a pack's own launches for a layer follow that layer's): the four parameters of each
    direction, (W_ih of both directions as one matrix with its residual, W_hh in MFMA fragment order, b_ih, b_hh) as unast_lstm_seq_fwd reads
    them, and the stacked W_hh (the train pack derives the backward's fragment order from it)."""
    for l in range(enc.num_layers):
        dirs = [tuple(getattr(enc.rnn, "%s_l%d%s" % (n, l, s)) for n in LSTM_NAMES) for s in ("", "_reverse")]
        w_ih, w_hh, b_ih, b_hh = zip(*dirs)
        whh = torch.stack(w_hh)
        yield dirs, (contract.resid(torch.cat(w_ih)), ops.lstm_whh_fragments(whh), torch.cat(b_ih).detach().contiguous(), torch.cat(b_hh).detach().contiguous()), whh


def encoder_reduce(enc):
    """reduce_h_W, reduce_c_W as (weight, bias, module)."""
    return [(detached(lin.weight), detached(lin.bias), lin) for lin in (enc.reduce_h_W, enc.reduce_c_W)]


def attention_operands(dec):
    """The attention layer, Luong (anything but 'lsa') or location-sensitive: its operands under the attribute names every pack gives them,
    and the modules they come from (query, memory, v, location conv, location dense; the last two None for Luong)."""
    at = dec.attention_layer
    if dec.attention == "lsa":
        mode, mods = ops.ATTN_LSA, (at.query_layer.linear_layer, at.memory_layer.linear_layer, at.v.linear_layer,
                                    at.location_layer.location_conv.conv, at.location_layer.location_dense.linear_layer)
    else:
        mode, mods = ops.ATTN_LUONG, (at.project_hid, at.project_eo, at.fc2, None, None)
    q, mem, v, conv, dense = mods
    return dict(mode=mode, Wq=detached(q.weight), Wmem=contract.resid(mem.weight), v=detached(v.weight).view(-1), conv_w=detached(conv.weight) if conv is not None else None,
                dense_w=detached(dense.weight) if dense is not None else None), mods


def text_prenet_stages(pn):
    """TextPrenet's three (conv, BatchNorm) stages: folded by the eval pack, kept apart (tap-major weight, batch statistics) by the train packs."""
    return [(getattr(pn, "conv%d" % i).conv, getattr(pn, "batch_norm%d" % i)) for i in (1, 2, 3)]


def speech_postnet_stages(po):
    """SpeechPostnet's four (conv, BatchNorm) stages in front of conv2."""
    return [(po.conv1.conv, po.pre_batchnorm)] + [(c.conv, bn) for c, bn in zip(po.conv_list, po.batch_norm_list)]


def speech_prenet_linears(prenet):
    """SpeechPrenet's fc1, fc2 as (weight with its residual, bias, module)."""
    return [(contract.resid(fc.linear_layer.weight), detached(fc.linear_layer.bias), fc.linear_layer) for fc in (prenet.layer.fc1, prenet.layer.fc2)]


def padded_head(*linears):
    """The given linears' rows as one head, zero rows added up to a multiple of 4 (the pitch the train paths' loss kernels read):
    (((Wh, its residual), bh), ldh)."""
    W, b = (torch.cat([getattr(lin, n).detach() for lin in linears]) for n in ("weight", "bias"))
    pad = -W.shape[0] % 4
    return (contract.resid(torch.nn.functional.pad(W, (0, 0, 0, pad))), torch.nn.functional.pad(b, (0, pad))), W.shape[0] + pad


class Pack:
    """The operands the eval kernels read, derived from one model's parameters (module docstring)."""

    def __init__(self, m, side):
        with torch.no_grad():
            enc, dec = m.encoder, m.decoder
            self.enc = [operands for _, operands, _ in encoder_layers(enc)]
            self.reduce_h, self.reduce_c = ((w, b) for w, b, _ in encoder_reduce(enc))
            self.dec = [tuple(detached(getattr(dec.rnn, n + "_l%d" % l)) for n in LSTM_NAMES) for l in range(dec.num_layers)]
            vars(self).update(attention_operands(dec)[0])              # mode, Wq, Wmem, v, conv_w, dense_w
            self.proj = (detached(dec.linear_projection.linear_layer.weight), detached(dec.linear_projection.linear_layer.bias))
            if side == "text":
                self.emb = detached(m.prenet.embed.weight)
                self.convs = [_fold_resid(conv, bn) for conv, bn in text_prenet_stages(m.prenet)]
                self.head = (detached(m.postnet.fc1.weight), detached(m.postnet.fc1.bias))
                self.head_rows = contract.resid(m.postnet.fc1.weight)
            else:
                po = m.postnet
                (self.fc1_rows, b1, _), (self.fc2_rows, b2, _) = speech_prenet_linears(m.prenet)
                self.fc1, self.fc2 = (self.fc1_rows[0], b1), (self.fc2_rows[0], b2)
                self.head = (torch.cat([po.linear_project.weight, po.stop_linear.weight]).contiguous(),
                             torch.cat([po.linear_project.bias, po.stop_linear.bias]).contiguous())
                self.post = [_fold_resid(conv, bn) for conv, bn in speech_postnet_stages(po)]
                self.post_out = contract.tap_major(po.conv2.conv)


def _fold_resid(conv, bn):
    w, b = contract.fold_bn(conv, bn)
    return contract.resid(w), b


# ---- the version-keyed caches of derived operands: one slot in a model's __dict__ per pack ---------------------------------------------------
EVAL_SLOT, ENCODER_TRAIN_SLOT, DECODER_TRAIN_SLOT = PACK_SLOTS = ("_rnn_pack", "_rnn_train_pack", "_rnn_decoder_train_pack")


def pack_of(m, side):
    return contract.cached_operands(m, EVAL_SLOT, list(m.parameters()) + list(m.buffers()), lambda: Pack(m, side))


def drop_eval_pack(m):
    """For the train-mode forwards: their kernels write the BatchNorm running statistics behind torch's version counters, so the cached eval
    operands (which fold those statistics) are dropped rather than left to the key."""
    m.__dict__.pop(EVAL_SLOT, None)


# ---- encoders ---------------------------------------------------------------------------------------------------------------------------
def text_frontend(P, text, noise=None):
    """TextPrenet over whole sequences (src/module.py:217-230, eval): embedding, three conv + BatchNorm + ReLU stages.  [B,T] -> [B,T,256].
    noise = (p, seed, stream): noise_fn on the embedded ids (src/network.py:519-521; it does not look at model.training, so evaluate() keeps it:
    unast_amd.eval_rnn); None changes nothing."""
    B, T = text.shape
    x = buf(B * T, P.emb.shape[1], dev=text.device)
    if noise is None:
        ops.embed_fwd(text, P.emb, x, T)
    else:
        ops.embed_fwd(text, P.emb, x, T, seed=noise[1], noise_p=noise[0], noise_stream=noise[2])
    x = x.view(B, T, -1)
    for wp, b in P.convs:
        x = contract.relu_(contract.conv(x, wp, b, 2))
    return x


def speech_frontend(P, mel, noise=None):
    """SpeechPrenet (src/module.py:95-110, eval): two linear + ReLU layers per frame.  noise = (p, seed, stream): noise_fn on the input mel
    (src/network.py:306-307), as text_frontend's; None changes nothing."""
    B, T, M = mel.shape
    m2 = mel.reshape(B * T, M)
    if noise is not None:
        mn = torch.empty_like(m2)
        ops.rowmask(m2.contiguous(), mn, noise[0], noise[1], noise[2])
        m2 = mn
    h = contract.linear_rows(m2, P.fc1_rows, P.fc1[1], act=1)
    return contract.linear_rows(h, P.fc2_rows, P.fc2[1], act=1).view(B, T, -1)


def encoder(P, x, lens_i32):
    """RNNEncoder.forward (src/module.py:313-336): the packed bidirectional LSTM stack, then reduce_h_W / reduce_c_W on each layer's
    [forward | backward] final states.  x [B,T,256] -> (enc_output [B,T,512] with zero rows at t >= lens[b], h [L,B,256], c [L,B,256])."""
    B, T, _ = x.shape
    dev = x.device
    x2 = x.reshape(B * T, -1)
    L = len(P.enc)
    h, c = buf(L, B, 256, dev=dev), buf(L, B, 256, dev=dev)
    for l, (w_ih, wfrag, b_ih, b_hh) in enumerate(P.enc):
        xproj = contract.linear_rows(x2, w_ih, None).view(B, T, -1)
        y, hn, cn = buf(B, T, 512, dev=dev), buf(B, 512, dev=dev), buf(B, 512, dev=dev)
        ops.lstm_seq_fwd(xproj, wfrag, b_ih, b_hh, lens_i32, y, hn, cn)
        ops.rnn_linear(hn, P.reduce_h[0], P.reduce_h[1], h[l])
        ops.rnn_linear(cn, P.reduce_c[0], P.reduce_c[1], c[l])
        x2 = y.view(B * T, 512)
    return y, h, c


# ---- decoders ---------------------------------------------------------------------------------------------------------------------------
class _Core:
    """What the text and the speech step share: attention, the two LSTM layers, the tanh projection (RNNDecoder.forward, src/module.py:362-374)."""

    def __init__(self, P, enc, lens_k, h0, c0, lsa_state=None):
        B, Tk, _ = enc.shape
        dev = enc.device
        self.P, self.enc, self.lens_k, self.B = P, enc, lens_k, B
        A = P.Wmem[0].shape[0]
        self.mem = contract.linear_rows(enc.view(B * Tk, -1), P.Wmem, None).view(B, Tk, A)  # memory-side projection, once per generation
        self.h0, self.c0 = h0, c0
        self.h, self.c = h0.clone(), c0.clone()
        self.ctx = buf(B, 512, dev=dev)
        self.ga, self.gb = buf(B, 1024, dev=dev), buf(B, 1024, dev=dev)
        self.pa, self.out = buf(B, 256, dev=dev), buf(B, 256, dev=dev)
        if P.mode == ops.ATTN_LSA:
            self.prev, self.cum = lsa_state if lsa_state is not None else (torch.zeros(B, Tk, dtype=_F32, device=dev), torch.zeros(B, Tk, dtype=_F32, device=dev))
        else:
            self.prev = self.cum = None

    def reset(self):
        self.h.copy_(self.h0)
        self.c.copy_(self.c0)
        if self.prev is not None:
            self.prev.zero_()
            self.cum.zero_()

    def step(self, pre):
        """pre [B,256] (any row stride): the prenet output of this position.  Returns the decoder output [B,256]."""
        P, h, c, ctx, ga, gb = self.P, self.h, self.c, self.ctx, self.ga, self.gb
        # the query is the top layer's h from BEFORE this step's LSTM (src/module.py:365)
        ops.rnn_attn_step(P.mode, h[1], P.Wq, self.mem, P.v, self.enc, self.lens_k, ctx, prev=self.prev, cum=self.cum, conv_w=P.conv_w, dense_w=P.dense_w)
        w_ih, w_hh, b_ih, b_hh = P.dec[0]                                                  # LSTM input = [prenet | context] (src/module.py:367)
        ops.rnn_linear(pre, w_ih[:, :256], b_ih, ga)
        ops.rnn_linear(ctx, w_ih[:, 256:], None, gb, R=ga)
        ops.rnn_linear(h[0], w_hh, b_hh, ga, R=gb)
        ops.lstm_cell(ga, c[0], h[0])
        w_ih, w_hh, b_ih, b_hh = P.dec[1]
        ops.rnn_linear(h[0], w_ih, b_ih, gb)
        ops.rnn_linear(h[1], w_hh, b_hh, ga, R=gb)
        ops.lstm_cell(ga, c[1], h[1])
        Wp, bp = P.proj                                                                    # tanh(linear_projection([lstm_out | context]))
        ops.rnn_linear(h[1], Wp[:, :256], bp, self.pa)
        ops.rnn_linear(ctx, Wp[:, 256:], None, self.out, R=self.pa)
        ops.tanh_rows(self.out)
        return self.out


def _prep(enc_outputs, lens_k):
    (h0, c0), enc = enc_outputs
    return enc.detach().to(_F32).contiguous(), h0.detach().to(_F32).contiguous(), c0.detach().to(_F32).contiguous(), lens_k


def window_bufs(P, B, dev):
    """What text_prenet_last writes: the embedded window, the three conv outputs, and the convs' four temporaries (all [B,7,256], allocated
    once per generation like the rest of the step's state)."""
    return tuple(buf(B, WINDOW, P.emb.shape[1], dev=dev) for _ in range(8))


def text_prenet_last(P, tokens, pos_t, teacher_forced, bufs):
    """TextPrenet over the prefix at device position pos, last position only: a window recompute (csrc/rnn.hip unast_text_window).  The three
    convs run over the same 7-row window; rows that would need positions left of the window are never read by the row that is kept.
    `bufs` = window_bufs(...); token ids index the embedding table unchecked (callers check given ids, TextRNN._ids)."""
    x0, a1, a2, a3 = bufs[:4]
    work = bufs[4:]
    ops.text_window(tokens, P.emb, x0, pos_t, teacher_forced, SOS_IDX)
    contract.relu_(contract.conv(x0, P.convs[0][0], P.convs[0][1], 2, out=a1, work=work))
    ops.window_mask(a1, pos_t, teacher_forced)
    contract.relu_(contract.conv(a1, P.convs[1][0], P.convs[1][1], 2, out=a2, work=work))
    ops.window_mask(a2, pos_t, teacher_forced)
    contract.relu_(contract.conv(a2, P.convs[2][0], P.convs[2][1], 2, out=a3, work=work))
    return a3[:, WINDOW - 1, :]


@torch.no_grad()
def text_generation(P, enc_outputs, lens_k, max_len, target=None, tokens=None, pos0=0, lsa_state=None):
    """TextRNN.infer_sequence (src/network.py:586-617; target None) or decode_sequence (src/network.py:539-560; target [B,T] int64, max_len = T)
    as a _Generation.  `tokens` / `pos0`: a given prefix and its last index (TextRNN.decode, one step)."""
    enc, h0, c0, lens_k = _prep(enc_outputs, lens_k)
    B = enc.shape[0]
    dev = enc.device
    core = _Core(P, enc, lens_k, h0, c0, lsa_state)
    tf = target is not None
    V = P.head[0].shape[0]
    ldl = (V + 3) // 4 * 4
    if tf:
        src = target.contiguous()
        logits_all = torch.zeros(B, max_len, ldl, dtype=_F32, device=dev)
    elif tokens is not None:
        src = tokens.contiguous()
    else:
        src = torch.full((B, max_len + 1), PAD_IDX, dtype=torch.int64, device=dev)
        src[:, 0] = SOS_IDX
    logits = torch.zeros(B, ldl, dtype=_F32, device=dev)
    stop_lens = torch.full((B,), max_len, dtype=torch.int64, device=dev)
    pos_t = torch.full((1,), pos0, dtype=torch.int64, device=dev)
    bufs = window_bufs(P, B, dev)

    def reset():
        pos_t.fill_(pos0)
        stop_lens.fill_(max_len)
        core.reset()

    def step(epoch):
        out = core.step(text_prenet_last(P, src, pos_t, tf, bufs))
        if tf:
            ops.rnn_linear(out, P.head[0], P.head[1], None, pos=pos_t, y_frames=logits_all)              # logits -> logits_all[:, pos]
            ops.pos_advance(pos_t, epoch)
        else:
            ops.rnn_linear(out, P.head[0], P.head[1], logits)
            if tokens is None:
                ops.decode_end_text(logits, V, src, stop_lens, max_len, EOS_IDX, pos_t, epoch)             # argmax -> tokens[:, pos+1]; stop rule; pos += 1

    def finish(steps):
        if tf:
            return logits_all[:, :, :V]
        T = min(_exit_step(stop_lens, max_len), steps)
        res = src[:, 1:T + 1].contiguous()
        keep = torch.arange(T, device=dev)[None, :] < stop_lens[:, None]
        return res * keep, stop_lens

    g = _Generation(step, reset, finish, pos_t, stop_lens, max_len)
    g.core, g.logits, g.V = core, logits, V
    return g


def speech_postnet_sum(P, outs):
    """outputs + SpeechPostnet(outputs) (src/module.py:155-168, eval; src/network.py:344, 376): five causal 5-tap convs, BatchNorm folded, tanh."""
    B, T, M = outs.shape
    dev = outs.device
    x = outs
    for wp, b in P.post:
        x = contract.conv(x, wp, b, 4)
        ops.tanh_rows(x.view(B * T, -1))
    y = contract.conv(x, P.post_out[0], P.post_out[1], 4)
    ops.add_inplace(y, outs.contiguous())
    return y


@torch.no_grad()
def speech_generation(P, enc_outputs, lens_k, max_len, target=None, frame=None, lsa_state=None):
    """SpeechRNN.infer_sequence (src/network.py:312-349; target None) or decode_sequence (src/network.py:352-377; target [B,T,M], max_len = T)
    as a _Generation.  `frame` [B,1,M]: a given input frame (SpeechRNN.decode, one step)."""
    enc, h0, c0, lens_k = _prep(enc_outputs, lens_k)
    B = enc.shape[0]
    dev = enc.device
    core = _Core(P, enc, lens_k, h0, c0, lsa_state)
    tf = target is not None
    M = P.head[0].shape[0] - 1
    ldh = (M + 1 + 3) // 4 * 4
    outputs = torch.zeros(B, max_len + 1, M, dtype=_F32, device=dev)                       # position 0 = the all-zero go frame
    stops = torch.zeros(B, max_len + 1, dtype=_F32, device=dev)
    if tf:
        feed = torch.zeros(B, max_len + 1, M, dtype=_F32, device=dev)                      # step i reads target[:, i-1]; step 0 the zero frame
        feed[:, 1:].copy_(target)
    elif frame is not None:
        feed = frame.detach().to(_F32).contiguous()
    else:
        feed = outputs
    stop_lens = torch.full((B,), max_len, dtype=torch.int64, device=dev)                   # never moves when teacher-forced: the stop rule is off
    rule_lens = torch.full((B,), max_len, dtype=torch.int64, device=dev) if tf else stop_lens
    pos_t = torch.zeros(1, dtype=torch.int64, device=dev)
    head = torch.zeros(B, ldh, dtype=_F32, device=dev)
    p1, pre = buf(B, P.fc1[0].shape[0], dev=dev), buf(B, 256, dev=dev)

    def reset():
        pos_t.zero_()
        stop_lens.fill_(max_len)
        rule_lens.fill_(max_len)
        core.reset()

    def step(epoch):
        ops.rnn_linear(None, P.fc1[0], P.fc1[1], p1, act=1, pos=pos_t, x_frames=feed)                       # SpeechPrenet on the frame at pos
        ops.rnn_linear(p1, P.fc2[0], P.fc2[1], pre, act=1)
        out = core.step(pre)
        ops.rnn_linear(out, P.head[0], P.head[1], head)
        if frame is None:
            ops.decode_end_speech(head, M, outputs, stops, rule_lens, max_len, pos_t, epoch)              # frame / stop -> pos+1; stop rule; pos += 1

    def finish(steps):
        if tf:
            post = speech_postnet_sum(P, outputs)
            return outputs[:, 1:], post[:, 1:], stops[:, 1:]
        T = min(_exit_step(stop_lens, max_len), steps)
        outs = outputs[:, :T + 1].contiguous()
        post = speech_postnet_sum(P, outs)
        pre_res, res = outs[:, 1:].contiguous(), post[:, 1:].contiguous()
        res_stop = stops[:, 1:T + 1].contiguous().unsqueeze(-1)
        ops.mask_by_len(pre_res, stop_lens)
        ops.mask_by_len(res, stop_lens)
        ops.mask_by_len(res_stop, stop_lens)
        return pre_res, res, res_stop.squeeze(-1), stop_lens

    g = _Generation(step, reset, finish, pos_t, stop_lens, max_len)
    g.core, g.head, g.M = core, head, M
    return g
