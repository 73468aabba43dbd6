"""fp64 torch restatement of the RNN model family's eval arithmetic (TextRNN / SpeechRNN: LSTM encoder, additive attention, one decoder
step), written from the formulas, as the yardstick of the HIP kernels in unast_amd/csrc/rnn.hip.  CPU only, no package import.

Conventions: lens are python ints or an int tensor [B]; padding is a suffix; weights keep torch's nn.LSTM / nn.Linear / nn.Conv1d layouts."""
import torch
import torch.nn.functional as F

F64 = torch.float64


def lstm_cell(gates, c, order="ifgo"):
    """(h, c) from summed gate pre-activations [B, 4H] laid out in `order` (torch: i, f, g, o)."""
    H = gates.shape[1] // 4
    part = {name: gates[:, k * H:(k + 1) * H] for k, name in enumerate(order)}
    i, f, g, o = torch.sigmoid(part["i"]), torch.sigmoid(part["f"]), torch.tanh(part["g"]), torch.sigmoid(part["o"])
    c = f * c + i * g
    return o * torch.tanh(c), c


def lstm_direction(x, lens, w_ih, w_hh, b_ih, b_hh, reverse=False, order="ifgo"):
    """One direction of a packed LSTM layer over x [B,T,D]: (y [B,T,H] with zero rows at t >= lens[b], h_n [B,H], c_n [B,H]).
    The reverse direction starts at lens[b] - 1 with a zero state."""
    B, T, _ = x.shape
    H = w_hh.shape[1]
    y = torch.zeros(B, T, H, dtype=x.dtype)
    hn, cn = torch.zeros(B, H, dtype=x.dtype), torch.zeros(B, H, dtype=x.dtype)
    for b in range(B):
        n = int(lens[b])
        h, c = torch.zeros(1, H, dtype=x.dtype), torch.zeros(1, H, dtype=x.dtype)
        for s in range(n):
            t = n - 1 - s if reverse else s
            gates = x[b, t:t + 1] @ w_ih.T + h @ w_hh.T + (b_ih + b_hh if b_hh is not None else b_ih)
            h, c = lstm_cell(gates, c, order)
            y[b, t] = h[0]
        hn[b], cn[b] = h[0], c[0]
    return y, hn, cn


def attn_step(mode, h, Wq, mem, v, enc, lens, prev=None, cum=None, conv_w=None, dense_w=None, mask_extra=0, conv_shift=0):
    """One additive-attention step.  mode 'luong': e = v . tanh(Wq h + mem); mode 'lsa': e = v . tanh(Wq h + dense(conv([prev; cum])) + mem)
    with conv = Conv1d(2 -> 32, k = 31, pad 15, no bias).  Keys t >= lens[b] get -inf before the softmax.  Returns (ctx [B,D], weights [B,Tk],
    new cum or None).  mask_extra / conv_shift plant faults for the tests (one key too many; the conv shifted by one tap)."""
    B, Tk, A = mem.shape
    x = (h @ Wq.T)[:, None, :]
    if mode == "lsa":
        cat = torch.stack([prev, cum], dim=1)                               # [B, 2, Tk]
        loc = F.conv1d(F.pad(cat, (15 + conv_shift, 15 - conv_shift)), conv_w)   # [B, 32, Tk]
        x = x + loc.transpose(1, 2) @ dense_w.T
    e = torch.tanh(x + mem) @ v                                               # [B, Tk]
    lens_t = torch.as_tensor([int(n) for n in lens]) + mask_extra
    masked = torch.arange(Tk)[None, :] >= lens_t[:, None]
    w = torch.softmax(e.masked_fill(masked, float("-inf")), dim=1)
    ctx = torch.bmm(w[:, None, :], enc)[:, 0]
    return ctx, w, (cum + w if mode == "lsa" else None)


# ---- whole models ---------------------------------------------------------------------------------------------------------------------
PAD, SOS, EOS = 0, 1, 2
FAULTS = ("gate_order", "no_b_hh", "mask_plus_one", "query_after", "no_cum", "conv_shift", "causal_prenet", "keep_sos", "c_not_reduced")


def _bn(x, sd, pre, eps=1e-5):
    """Eval BatchNorm1d over [B,C,T]."""
    s = sd[pre + "weight"] / torch.sqrt(sd[pre + "running_var"] + eps)
    return (x - sd[pre + "running_mean"][None, :, None]) * s[None, :, None] + sd[pre + "bias"][None, :, None]


class RNNModel:
    """TextRNN or SpeechRNN in eval mode from a state_dict (fp64).  `fault`: one of FAULTS, a planted deviation the tests must see."""

    def __init__(self, side, sd, attn, fault=None):
        assert fault is None or fault in FAULTS
        self.side, self.attn, self.fault = side, attn, fault
        self.sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        self.order = "ifog" if fault == "gate_order" else "ifgo"

    # front ends
    def text_prenet(self, ids):
        sd = self.sd
        x = sd["prenet.embed.weight"][ids].transpose(1, 2)                        # [B,E,T]
        for i in (1, 2, 3):
            pad = (4, 0) if self.fault == "causal_prenet" else (2, 2)
            x = F.conv1d(F.pad(x, pad), sd["prenet.conv%d.conv.weight" % i], sd["prenet.conv%d.conv.bias" % i])
            x = torch.relu(_bn(x, sd, "prenet.batch_norm%d." % i))
        return x.transpose(1, 2)

    def speech_prenet(self, mel):
        sd = self.sd
        h = torch.relu(mel @ sd["prenet.layer.fc1.linear_layer.weight"].T + sd["prenet.layer.fc1.linear_layer.bias"])
        return torch.relu(h @ sd["prenet.layer.fc2.linear_layer.weight"].T + sd["prenet.layer.fc2.linear_layer.bias"])

    def speech_postnet(self, x):
        """SpeechPostnet.forward on [B,T,M]: five causal 5-tap convs (pad 4, last 4 outputs cut), BatchNorm + tanh behind the first four."""
        sd = self.sd
        x = x.transpose(1, 2)
        stages = [("postnet.conv1.", "postnet.pre_batchnorm.")] + [("postnet.conv_list.%d." % i, "postnet.batch_norm_list.%d." % i) for i in range(3)]
        for cp, bp in stages:
            x = torch.tanh(_bn(F.conv1d(F.pad(x, (4, 0)), sd[cp + "conv.weight"], sd[cp + "conv.bias"]), sd, bp))
        x = F.conv1d(F.pad(x, (4, 0)), sd["postnet.conv2.conv.weight"], sd["postnet.conv2.conv.bias"])
        return x.transpose(1, 2)

    # encoder
    def encode(self, x, lens):
        """x: token ids [B,T] or mel [B,T,M].  Returns ((h, c) each [2,B,H], enc_output [B,T,2H]), pad_mask."""
        sd = self.sd
        if self.side == "text":
            mask = x.eq(PAD)
            feats = self.text_prenet(x)
        else:
            mask = torch.arange(x.shape[1])[None, :] >= torch.as_tensor([int(n) for n in lens])[:, None]
            feats = self.speech_prenet(x.double())
        hs, cs = [], []
        for l in range(2):
            outs, hn, cn = [], [], []
            for sfx, rev in (("_l%d" % l, False), ("_l%d_reverse" % l, True)):
                g = lambda n: sd["encoder.rnn." + n + sfx]                          # noqa: E731
                y, h, c = lstm_direction(feats, lens, g("weight_ih"), g("weight_hh"), g("bias_ih"), None if self.fault == "no_b_hh" else g("bias_hh"),
                                         reverse=rev, order=self.order)
                outs.append(y); hn.append(h); cn.append(c)
            feats = torch.cat(outs, dim=-1)
            hs.append(torch.cat(hn, dim=-1)); cs.append(torch.cat(cn, dim=-1))
        h_, c_ = torch.stack(hs), torch.stack(cs)
        new_h = h_ @ sd["encoder.reduce_h_W.weight"].T + sd["encoder.reduce_h_W.bias"]
        cw = "encoder.reduce_h_W." if self.fault == "c_not_reduced" else "encoder.reduce_c_W."
        new_c = c_ @ sd[cw + "weight"].T + sd[cw + "bias"]
        return ((new_h, new_c), feats), mask

    # decoder
    def _attn_weights(self):
        sd, p = self.sd, "decoder.attention_layer."
        if self.attn == "lsa":
            return (sd[p + "query_layer.linear_layer.weight"], sd[p + "memory_layer.linear_layer.weight"], sd[p + "v.linear_layer.weight"][0],
                    sd[p + "location_layer.location_conv.conv.weight"], sd[p + "location_layer.location_dense.linear_layer.weight"])
        return sd[p + "project_hid.weight"], sd[p + "project_eo.weight"], sd[p + "fc2.weight"][0], None, None

    def start(self, enc_outputs, mask):
        """The state of one generation: LSTM states, the memory-side projection, the LSA weights."""
        (h, c), enc = enc_outputs
        Wq, Wm, v, cw, dw = self._attn_weights()
        B, Tk = enc.shape[:2]
        lens_k = (~mask).sum(1) if mask.dtype == torch.bool else mask
        return dict(h=h.clone(), c=c.clone(), enc=enc, mem=enc @ Wm.T, lens=[int(n) for n in lens_k], prev=torch.zeros(B, Tk, dtype=F64),
                    cum=torch.zeros(B, Tk, dtype=F64), weights=[])

    def _lstm_step(self, l, x, h, c):
        sd = self.sd
        g = lambda n: sd["decoder.rnn.%s_l%d" % (n, l)]                              # noqa: E731
        gates = x @ g("weight_ih").T + h @ g("weight_hh").T + g("bias_ih") + (0 if self.fault == "no_b_hh" else g("bias_hh"))
        return lstm_cell(gates, c, self.order)

    def step(self, st, pre):
        """RNNDecoder.forward on one position: pre [B,256] -> tanh(linear_projection([lstm_out | context])) [B,256]."""
        sd = self.sd
        Wq, Wm, v, cw, dw = self._attn_weights()

        def attend(query):
            ctx, w, cum = attn_step(self.attn, query, Wq, st["mem"], v, st["enc"], st["lens"], st["prev"], st["cum"], cw, dw,
                                    mask_extra=1 if self.fault == "mask_plus_one" else 0, conv_shift=1 if self.fault == "conv_shift" else 0)
            st["weights"].append(w)
            if self.attn == "lsa":
                st["prev"] = w
                if self.fault != "no_cum":
                    st["cum"] = cum
            return ctx
        h, c = st["h"], st["c"]
        if self.fault != "query_after":
            ctx = attend(h[1])                                                       # the top layer's h from before this step's LSTM
            x0 = torch.cat([pre, ctx], dim=-1)
        else:                                                                        # planted: LSTM on the previous context, query taken afterwards
            x0 = torch.cat([pre, st.get("ctx_prev", torch.zeros(pre.shape[0], st["enc"].shape[2], dtype=F64))], dim=-1)
        h0, c0 = self._lstm_step(0, x0, h[0], c[0])
        h1, c1 = self._lstm_step(1, h0, h[1], c[1])
        if self.fault == "query_after":
            ctx = attend(h1)
            st["ctx_prev"] = ctx
        st["h"], st["c"] = torch.stack([h0, h1]), torch.stack([c0, c1])
        W, b = sd["decoder.linear_projection.linear_layer.weight"], sd["decoder.linear_projection.linear_layer.bias"]
        return torch.tanh(torch.cat([h1, ctx], dim=-1) @ W.T + b)

    def _text_head(self, out):
        return out @ self.sd["postnet.fc1.weight"].T + self.sd["postnet.fc1.bias"]

    def _speech_head(self, out):
        sd = self.sd
        return out @ sd["postnet.linear_project.weight"].T + sd["postnet.linear_project.bias"], (out @ sd["postnet.stop_linear.weight"].T + sd["postnet.stop_linear.bias"])[:, 0]

    def decode_sequence(self, target, enc_outputs, mask):
        """Teacher-forced.  Text: logits [B,T,V]; prefixes [SOS], then target[:, :i] with no SOS in front.  Speech: (pre, post, stop); step 0 reads
        the zero frame, step i target[:, i-1]; post = outputs + postnet(outputs) with the go frame included, then cut."""
        st = self.start(enc_outputs, mask)
        B, T = target.shape[:2]
        if self.side == "text":
            outs = []
            sos = torch.full((B, 1), SOS, dtype=torch.long)
            for i in range(T):
                prefix = sos if i == 0 else (torch.cat([sos, target[:, :i]], dim=1) if self.fault == "keep_sos" else target[:, :i])
                pre = self.text_prenet(prefix)[:, -1]
                st.setdefault("pre_rows", []).append(pre)
                outs.append(self._text_head(self.step(st, pre)))
            return torch.stack(outs, dim=1), st
        target = target.double()
        frames, stops = [torch.zeros(B, target.shape[2], dtype=F64)], []
        for i in range(T):
            inp = frames[0] if i == 0 else target[:, i - 1]
            mel, stop = self._speech_head(self.step(st, self.speech_prenet(inp)))
            frames.append(mel); stops.append(stop)
        outputs = torch.stack(frames, dim=1)
        res = outputs + self.speech_postnet(outputs)
        return (outputs[:, 1:], res[:, 1:], torch.stack(stops, dim=1)), st

    def infer_sequence(self, enc_outputs, mask, max_len):
        """Greedy decoding.  Text: (tokens [B,T] zeroed from each stop length on, stop_lens); speech: (pre, post, stop, stop_lens), masked likewise."""
        st = self.start(enc_outputs, mask)
        B = enc_outputs[1].shape[0]
        stop_lens = torch.full((B,), max_len, dtype=torch.long)
        i = 0
        if self.side == "text":
            tokens = torch.full((B, 1), SOS, dtype=torch.long)
            while bool((stop_lens == max_len).any()) and i < max_len:
                choice = self._text_head(self.step(st, self.text_prenet(tokens)[:, -1])).argmax(dim=-1)
                tokens = torch.cat([tokens, choice[:, None]], dim=1)
                i += 1
                stop_lens[(choice == EOS) & (stop_lens == max_len)] = i
            res = tokens[:, 1:]
            return res * (torch.arange(res.shape[1])[None, :] < stop_lens[:, None]), stop_lens
        M = self.sd["postnet.linear_project.weight"].shape[0]
        frames, stops = [torch.zeros(B, M, dtype=F64)], []
        while bool((stop_lens == max_len).any()) and i < max_len:
            mel, stop = self._speech_head(self.step(st, self.speech_prenet(frames[-1])))
            frames.append(mel); stops.append(stop)
            i += 1
            stop_lens[(torch.sigmoid(stop) >= .5) & (stop_lens == max_len)] = i
        outputs = torch.stack(frames, dim=1)
        keep = (torch.arange(i)[None, :] < stop_lens[:, None]).double()
        res = (outputs + self.speech_postnet(outputs))[:, 1:] * keep[..., None]
        return outputs[:, 1:] * keep[..., None], res, torch.stack(stops, dim=1) * keep, stop_lens

    def forward(self, x, lens):
        enc_outputs, mask = self.encode(x, lens)
        return self.decode_sequence(x, enc_outputs, mask)[0]


def value_outputs(text_sd, speech_sd, attn, text, text_len, mel, mel_len, fault=None):
    """Every tensor of a value fixture (tools/gen_golden_rnn.py run_values), by the mirror."""
    tm, sm = RNNModel("text", text_sd, attn, fault), RNNModel("speech", speech_sd, attn, fault)
    out = {}
    with torch.no_grad():
        t_eo, t_mask = tm.encode(text, text_len)
        s_eo, s_mask = sm.encode(mel, mel_len)
        out["text_enc_out"], out["text_h"], out["text_c"] = t_eo[1], t_eo[0][0], t_eo[0][1]
        out["speech_enc_out"], out["speech_h"], out["speech_c"] = s_eo[1], s_eo[0][0], s_eo[0][1]
        out["text_forward"], st = tm.decode_sequence(text, t_eo, t_mask)
        out["text_forward_prenet"] = torch.stack(st["pre_rows"])
        (out["speech_forward_pre"], out["speech_forward_post"], out["speech_forward_stop"]), st = sm.decode_sequence(mel, s_eo, s_mask)
        if attn == "lsa":
            out["lsa_weights"] = torch.stack(st["weights"][:5])
        (out["tts_pre"], out["tts_post"], out["tts_stop"]), _ = sm.decode_sequence(mel, t_eo, t_mask)
        out["asr"], _ = tm.decode_sequence(text, s_eo, s_mask)
        sos = torch.full((text.shape[0], 1), SOS, dtype=torch.long)
        out["prenet_infer"] = torch.stack([tm.text_prenet(torch.cat([sos, text[:, :L - 1]], dim=1))[:, -1] for L in range(1, 10)])
        out["prenet_tf"] = torch.stack([tm.text_prenet(text[:, :L])[:, -1] for L in range(1, 10)])
    return out
