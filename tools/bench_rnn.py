#!/usr/bin/env python3
"""Times the RNN model family's eval path on the GPU (HIP events, warm-up, medians): unast_lstm_seq_fwd per recurrent step, both encoders,
one decoded position eager and replayed for both models and both attention types, and a whole tts(infer) cut to --frames frames (the text
encoder plus SpeechRNN.infer_sequence(max_len=frames); UNAST.tts itself always decodes up to infer_sequence's default of 815).
Sizes: B = 32, T_text = 180, T_mel = 800.  --train: the encoder-training mode instead -- unast_lstm_seq_fwd_train next to unast_lstm_seq_fwd,
unast_lstm_seq_bwd per recurrent step, and train_rnn.encoder_forward + encoder_backward of both models (dropout and noise on).
--train-decoder: SpeechRNN decoder training at B = 32, T = 800, Tk in {180, 800}, both attention types (dropout on) -- decoder_forward,
decoder_forward + decoder_backward, the per-position time of each loop (events recorded through the entry points' `mark` callback), the eval
teacher-forced position of the same session as the yardstick, unast_rnn_attn_step_bwd next to unast_rnn_attn_step, and the saved-state bytes.
--train-text-decoder: TextRNN decoder training at T = 180, B in {4, 16, 32}, Tk in {180, 800}, both attention types (dropout on) --
text_decoder_forward, forward + backward, the prefix prenet's share, the loops' per-position times next to SpeechRNN's at the same shapes, the
saved bytes, and the prefix prenet issued position by position through the uniform-[B,T] entry points as the comparator of the slab form.
--train-step: the whole train step of the family (unast_amd.train_rnn_step through unast_amd.train's entry points, dropout, noise, SpecAugment
and the drawn permutation on) at T_text = 180, T_mel = 800, B in {4, 16}, both attention types -- ms per AE / SP / D sub-step and per
optimizer step of each phase, one warm-up round and medians of 5.  With --ddp the same under a process group of one forced rank (nccl backend,
UNAST_DDP_FORCE=1): the optimizer steps then include the data-parallel exchange of their segments.
--train-cm: the cross-model sub-step (unast_amd.train_rnn_step.train_cm_step) at T_text = 180, T_mel = 800, B in {4, 16}, both attention
types, dropout on, one warm-up and medians of 5.  Generation length depends on the weights, so the stop rule is OFF here (the EOS and stop
biases are set so that no sequence stops) and both generations run a fixed position count: 180 text positions, 800 frames.  Reports the text
prenet per position, fused (csrc/prefix_gen.hip: 4 launches) against the comparator composed from the uniform-[B,L] entry points (unast_embed_fwd,
the three-launch conv with its operand split, train-mode unast_bn_fwd: 23 device operations), averaged over the prefixes L = 1..180, and the
fused form at single prefix lengths L = 1 / 60 / 180 / 300 (its loaders reduce every tile's partial sums again: O(tiles^2) per launch); text and
speech generation per position; and the whole sub-step.
Usage: python tools/bench_rnn.py [--reps 7] [--frames 800] [--train | --train-decoder | --train-text-decoder | --train-step [--ddp] | --train-cm]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--ddp" in sys.argv:
    os.environ.setdefault("UNAST_DDP_FORCE", "1")          # read when unast_amd.ddp is imported: one rank takes the collective path
from tests import rnn_weights  # noqa: E402
from unast_amd import contract, ops, rnn  # noqa: E402
from unast_amd.inference import _capture  # noqa: E402
from unast_amd.network import TextRNN, SpeechRNN  # noqa: E402
from unast_amd.portable import synth_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--frames", type=int, default=800)
ap.add_argument("--train", action="store_true")
ap.add_argument("--train-decoder", action="store_true")
ap.add_argument("--train-text-decoder", action="store_true")
ap.add_argument("--train-step", action="store_true")
ap.add_argument("--train-cm", action="store_true")
ap.add_argument("--ddp", action="store_true")
a = ap.parse_args()
D = torch.device("cuda:0")
B, TT, TM = 32, 180, 800


def median_ms(fn, reps=a.reps, inner=1):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return statistics.median(out)


def models(attn):
    tm, sm = TextRNN(rnn_weights.rnn_args(attn)), SpeechRNN(rnn_weights.rnn_args(attn))
    for side, m in (("text", tm), ("speech", sm)):
        sd = m.state_dict()
        m.load_state_dict(rnn_weights.state_dict(side, list(sd), [list(v.shape) for v in sd.values()], 1234))
    return tm.to(D).eval(), sm.to(D).eval()


def train_mode():
    from unast_amd import train_rnn
    g = torch.Generator().manual_seed(0)
    for T in (TM, TT):
        xproj = torch.randn(B, T, 2048, generator=g).to(D)
        whh = (torch.randn(2, 1024, 256, generator=g) / 16).to(D)
        wfrag, wfrag_t = ops.lstm_whh_fragments(whh), ops.lstm_whh_fragments_bwd(whh)
        bias = torch.zeros(2048, device=D)
        lens = torch.full((B,), T, dtype=torch.int32, device=D)
        y, hn, cn = torch.empty(B, T, 512, device=D), torch.empty(B, 512, device=D), torch.empty(B, 512, device=D)
        saved, hprev = torch.empty(B, T, 2, 5, 256, device=D), torch.empty(B, T, 512, device=D)
        dy, dfin, dxproj = torch.randn(B, T, 512, generator=g).to(D), torch.randn(B, 512, generator=g).to(D), torch.empty(B, T, 2048, device=D)
        ev = median_ms(lambda: ops.lstm_seq_fwd(xproj, wfrag, bias, bias, lens, y, hn, cn))
        tr = median_ms(lambda: ops.lstm_seq_fwd_train(xproj, wfrag, bias, bias, lens, y, hn, cn, saved, hprev))
        bw = median_ms(lambda: ops.lstm_seq_bwd(dy, wfrag_t, saved, lens, dxproj, dhfinal=dfin, dcfinal=dfin))
        print("B=%d T=%d ndir=2: lstm_seq_fwd %.2f ms (%.2f us/step), lstm_seq_fwd_train %.2f ms (%.2f us/step, x %.3f), lstm_seq_bwd %.2f ms "
              "(%.2f us/step, x %.2f of the forward)" % (B, T, ev, ev * 1e3 / T, tr, tr * 1e3 / T, tr / ev, bw, bw * 1e3 / T, bw / ev))
    text, mel, text_len, mel_len = (torch.from_numpy(x) for x in synth_batch(B, TT, TM, seed=3))
    text, mel = text.to(D), mel.to(D)
    tm, sm = models("luong")
    tm.train(), sm.train()
    for name, m, x, ln, T in (("text", tm, text, text_len, TT), ("speech", sm, mel, mel_len, TM)):
        ln = ln.clone()
        ln[0] = T                                                      # encode's rule: max(lens) == T
        cot = (torch.randn(B, T, 512, device=D), torch.randn(2, B, 256, device=D), torch.randn(2, B, 256, device=D))
        tapes = []
        fw = median_ms(lambda: tapes.append(train_rnn.encoder_forward(m, x, ln, noise_in=True, seed=len(tapes))))

        def both():
            train_rnn.encoder_backward(train_rnn.encoder_forward(m, x, ln, noise_in=True, seed=1), *cot)
        del tapes[:]
        fb = median_ms(both)
        print("%s encoder, B=%d T=%d, dropout and noise on: encoder_forward %.2f ms, encoder_forward + encoder_backward %.2f ms" % (name, B, T, fw, fb))


def train_decoder_mode():
    from unast_amd import train_rnn
    g = torch.Generator().manual_seed(0)
    _, mel, _, _ = (torch.from_numpy(x) for x in synth_batch(B, TT, TM, seed=3))
    mel = mel.to(D)
    M = mel.shape[2]
    for attn in ("luong", "lsa"):
        _, sm = models(attn)
        mode = ops.ATTN_LSA if attn == "lsa" else ops.ATTN_LUONG
        for Tk in (TT, TM):
            enc = torch.randn(B, Tk, 512, generator=g).to(D) * 0.5
            hc = (torch.randn(2, B, 256, generator=g).to(D) * 0.5, torch.randn(2, B, 256, generator=g).to(D) * 0.5)
            lens_k = [Tk] * B
            cot = (torch.randn(B, TM, M, device=D), torch.randn(B, TM, M, device=D), torch.randn(B, TM, device=D))
            # the yardstick: the eval path's teacher-forced position, eager, same session
            sm.eval()
            with torch.no_grad():
                gen = rnn.speech_generation(sm._pack(), (hc, enc), torch.tensor(lens_k, dtype=torch.int32, device=D), TM, target=mel)
                gen.step(None)
                gen.reset()
                ev = median_ms(lambda: gen.step(None), inner=20)
            sm.train()
            keep = []
            fw = median_ms(lambda: keep.__setitem__(slice(None), [train_rnn.decoder_forward(sm, mel, (hc, enc), lens_k, seed=3)]))
            saved = keep[0].saved_bytes()
            del keep[:]
            loops = {"forward": [], "backward": []}

            def marker(name):
                def mark(_):
                    e = torch.cuda.Event(enable_timing=True)
                    e.record()
                    loops[name].append(e)
                return mark
            fb = median_ms(lambda: train_rnn.decoder_backward(train_rnn.decoder_forward(sm, mel, (hc, enc), lens_k, seed=3, mark=marker("forward")), *cot,
                                                              mark=marker("backward")))
            per = {n: statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(0, len(ev), 2)) * 1e3 / TM for n, ev in loops.items()}
            print("[%s] B=%d T=%d Tk=%d dropout on: decoder_forward %.1f ms, decoder_forward + decoder_backward %.1f ms; per position: forward loop %.1f us "
                  "(eval teacher-forced position %.1f us, ratio %.2f), backward loop %.1f us; saved state %.1f MiB"
                  % (attn, B, TM, Tk, fw, fb, per["forward"], ev * 1e3, per["forward"] / (ev * 1e3), per["backward"], saved / 2 ** 20))
            # the attention kernels alone
            P = train_rnn.decoder_pack_of(sm)
            A = P.A
            mem = torch.randn(B, Tk, A, generator=g).to(D) * 0.5
            h = hc[0][1]
            z = lambda *s: torch.zeros(*s, device=D)                                            # noqa: E731
            prev, cum, ctx = torch.softmax(torch.randn(B, Tk, generator=g), 1).to(D), z(B, Tk), z(B, 512)
            w, cum2 = z(B, Tk), z(B, Tk)
            f_eval = median_ms(lambda: ops.rnn_attn_step(mode, h, P.Wq, mem, P.v, enc, gen.core.lens_k, ctx, prev=prev.clone(), cum=cum.clone(),
                                                         conv_w=P.conv_w, dense_w=P.dense_w), inner=20)
            f_train = median_ms(lambda: ops.rnn_attn_step_train(mode, h, P.Wq, mem, P.v, enc, gen.core.lens_k, ctx, w, prev_in=prev, cum_in=cum, cum_out=cum2,
                                                                conv_w=P.conv_w, dense_w=P.dense_w), inner=20)
            clone = median_ms(lambda: (prev.clone(), cum.clone()), inner=20)
            ws = ops.rnn_attn_step_bwd_ws(B, Tk, A, D)
            kw = dict(prev=prev, cum=cum, conv_w=P.conv_w, dense_w=P.dense_w, d_w_a=z(B, Tk), d_w_b=z(B, Tk), carry=True, ddense_part=z(B, A, 32),
                      dconv_part=z(B, 32, 2, 31), d_prev=z(B, Tk), d_cum=z(B, Tk)) if attn == "lsa" else {}
            d_h, d_q, d_mem, dv = z(B, 256), z(B, A), z(B, Tk, A), z(B, A)
            bw = median_ms(lambda: ops.rnn_attn_step_bwd(mode, cot[0].new_ones(B, 512), w, h, P.Wq, mem, P.v, enc, gen.core.lens_k, d_h, d_q, d_mem, dv, ws, **kw),
                           inner=20)
            print("[%s] Tk=%d: unast_rnn_attn_step %.1f us (incl. %.1f us of two clones), unast_rnn_attn_step_train %.1f us, unast_rnn_attn_step_bwd %.1f us"
                  % (attn, Tk, f_eval * 1e3, clone * 1e3, f_train * 1e3, bw * 1e3))


def prefix_position_loop(P, ids, p, seed, params):
    """The comparator of --train-text-decoder: the prefix prenet's forward and backward issued position by position through the uniform-[B,T]
    entry points (unast_embed_fwd / _bwd, contract.conv, unast_bn_fwd / _bwd, the conv gradients) -- the same arithmetic as the slab form, about
    100 launches of a few hundred rows per position.  Timing only: the gradients land in the model's .grad."""
    from unast_amd.utils import SOS_IDX
    Bb, T = ids.shape
    E = P.emb.shape[1]
    contract.prepare_grads(params, False)
    sos = torch.full((Bb, 1), SOS_IDX, dtype=torch.int64, device=D)
    bn_ws = torch.empty(512, dtype=torch.float64, device=D)
    saved = []
    for s in range(T):
        tok = (sos if s == 0 else ids[:, :s]).contiguous()
        L = tok.shape[1]
        N = Bb * L
        x0 = torch.empty(N, E, device=D)
        ops.embed_fwd(tok, P.emb, x0, L, drop_p=p, seed=seed, stream_id=40)
        xs, zs, mean, rstd = [x0], [], torch.empty(3, 256, device=D), torch.empty(3, 256, device=D)
        cur = x0.view(Bb, L, E)
        for i, (wp, bias, _, bn) in enumerate(P.convs):
            z = contract.conv(cur, wp, bias, 2).view(N, 256)
            y = torch.empty(N, 256, device=D)
            ops.bn_fwd(z, bn.weight, bn.bias, y, mean[i], rstd[i], bn.running_mean, bn.running_var, bn_ws, 1, drop_p=p, seed=seed, stream_id=41 + i, eps=bn.eps,
                       momentum=bn.momentum, num_batches_tracked=bn.num_batches_tracked)
            zs.append(z)
            xs.append(y)
            cur = y.view(Bb, L, 256)
        saved.append((tok, xs, zs, mean, rstd))
    for s in range(T - 1, -1, -1):
        tok, xs, zs, mean, rstd = saved[s]
        L = tok.shape[1]
        N = Bb * L
        dy = torch.zeros(Bb, L, 256, device=D)
        dy[:, -1] = 1.0                                                                           # d_P: on the prefix's last row only
        dy = dy.view(N, 256)
        for i in (2, 1, 0):
            wpair, _, conv, bn = P.convs[i]
            dz = torch.empty(N, 256, device=D)
            ops.bn_bwd(dy, zs[i], mean[i], rstd[i], bn.weight, bn.bias, dz, bn.weight.grad, bn.bias.grad, bn_ws, 1, drop_p=p, seed=seed, stream_id=41 + i)
            dy = contract.conv_grads(dz, xs[i], Bb, L, wpair, conv, 2)
        ops.embed_bwd(tok, dy, P.emb_grad, L, drop_p=p, seed=seed, stream_id=40, padding_idx=0)


def train_text_decoder_mode():
    """TextRNN decoder training at T = 180 (B in {4, 16, 32}; the RNN configs train at 4 and 16), Tk in {180, 800}, both attention types, dropout
    on: text_decoder_forward, forward + backward, the prefix prenet's share of each, the per-position loop times next to SpeechRNN's at the same
    B / T / Tk in the same session, the saved bytes -- and, once per B (it does not depend on the attention or Tk), the prefix prenet's forward +
    backward in the slab form against the position-by-position comparator."""
    from unast_amd import train_rnn
    g = torch.Generator().manual_seed(0)
    T = TT
    for Bb in (4, 16, 32):
        text, mel, _, _ = (torch.from_numpy(x) for x in synth_batch(Bb, T, T, seed=3))
        text, mel = text.to(D), mel[:, :T].contiguous().to(D)
        for attn in ("luong", "lsa"):
            tm, sm = models(attn)
            tm.train(), sm.train()
            for Tk in (TT, TM):
                enc = torch.randn(Bb, Tk, 512, generator=g).to(D) * 0.5
                hc = (torch.randn(2, Bb, 256, generator=g).to(D) * 0.5, torch.randn(2, Bb, 256, generator=g).to(D) * 0.5)
                lens_k = [Tk] * Bb
                cot = torch.randn(Bb, T, 46, device=D)
                scot = (torch.randn(Bb, T, mel.shape[2], device=D), torch.randn(Bb, T, mel.shape[2], device=D), torch.randn(Bb, T, device=D))
                keep = []
                fw = median_ms(lambda: keep.__setitem__(slice(None), [train_rnn.text_decoder_forward(tm, text, (hc, enc), lens_k, seed=3)]))
                saved = keep[0].saved_bytes()
                del keep[:]
                ev = {}

                def marker(side):
                    def mark(name):
                        e = torch.cuda.Event(enable_timing=True)
                        e.record()
                        ev.setdefault((side, name), []).append(e)
                    return mark

                def span(side, what):
                    b, e = ev[(side, what + "_begin")], ev[(side, what + "_end")]
                    return statistics.median(x.elapsed_time(y) for x, y in zip(b, e))
                fb = median_ms(lambda: train_rnn.text_decoder_backward(train_rnn.text_decoder_forward(tm, text, (hc, enc), lens_k, seed=3, mark=marker("tf")), cot,
                                                                       mark=marker("tb")))
                sfb = median_ms(lambda: train_rnn.decoder_backward(train_rnn.decoder_forward(sm, mel, (hc, enc), lens_k, seed=3, mark=marker("sf")), *scot,
                                                                   mark=marker("sb")))
                pf, pb = span("tf", "prefix"), span("tb", "prefix")
                print("[%s] B=%d T=%d Tk=%d dropout on: text_decoder_forward %.1f ms, forward + backward %.1f ms; prefix prenet %.1f ms forward + %.1f ms backward "
                      "(%.0f %% of forward + backward); per position: forward loop %.1f us (speech %.1f), backward loop %.1f us (speech %.1f); speech forward + "
                      "backward %.1f ms; saved state %.1f MiB"
                      % (attn, Bb, T, Tk, fw, fb, pf, pb, 100 * (pf + pb) / fb, span("tf", "loop") * 1e3 / T, span("sf", "loop") * 1e3 / T,
                         span("tb", "loop") * 1e3 / T, span("sb", "loop") * 1e3 / T, sfb, saved / 2 ** 20))
            if attn == "luong":
                P = train_rnn.decoder_pack_of(tm, train_rnn.TextDecoderPack)
                params = list(tm.prenet.parameters())
                contract.prepare_grads(params, False)
                P.emb_grad = tm.prenet.embed.weight.grad
                p = float(tm.prenet.p)
                loop = median_ms(lambda: prefix_position_loop(P, text, p, 3, params), reps=3)
                lay = train_rnn.prefix_layout(Bb, T)
                print("prefix prenet B=%d T=%d (%d slab rows, %d live): slab form %.1f ms forward + backward (the figures above), position-by-position "
                      "comparator %.1f ms" % (Bb, T, lay.total, lay.total - 2 * Bb * T, pf + pb, loop))


def train_step_mode():
    import json
    from collections import defaultdict
    from types import SimpleNamespace
    from unast_amd import train
    train.DEVICE = D
    if a.ddp:
        import torch.distributed as dist
        from unast_amd import ddp
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29617")
        dist.init_process_group("nccl", rank=0, world_size=1)
        torch.cuda.set_device(D)
        print("--ddp: one forced rank over the nccl backend; data-parallel exchange active: %s; native communicator: %s"
              % (ddp.active(), bool(ddp.native_comm())), flush=True)
    cfgs = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "rnn_configs.json")))
    for attn in ("luong", "lsa"):
        for Bb in (4, 16):
            args = SimpleNamespace(**dict(cfgs["rnn_d_" + attn], load_path=None, ae_steps=1, sp_steps=1, cm_steps=0, d_steps=1, train_batch_size=Bb))
            train.set_seed(0)
            _, _, model, opt, _ = train.initialize_model(args)
            model.train()
            getter = train.SyntheticBatchGetter(args, t_text=TT, t_mel=TM)
            times, losses = defaultdict(list), defaultdict(list)

            def timed(name, fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
            for rep in range(6):                                                                  # one warm-up round, five measured
                if rep == 1:
                    times.clear()
                b_ae, b_sp, b_d = getter._next(), getter._next(), getter._next()
                train.freeze_model_parameters(model.discriminator)
                timed("ae", lambda: train.train_ae_step(losses, model, b_ae, 0, 2, args))
                timed("sp", lambda: train.train_sp_step(losses, model, b_sp, 0, 2, args))
                timed("opt_gen", lambda: train.optimizer_step(model, opt, args))
                train.unfreeze_model_parameters(model.discriminator)
                timed("d", lambda: train.train_discriminator_step(losses, model, b_d, 0, 1, args))
                timed("opt_disc", lambda: train.optimizer_step(model, opt, args))
            med = {k: statistics.median(v) for k, v in times.items()}
            assert all(bool(torch.isfinite(v)) for vs in losses.values() for v in vs)
            print("[%s] B=%d T_text=%d T_mel=%d: AE sub-step %.1f ms, SP sub-step %.1f ms, generator optimizer_step %.2f ms, D sub-step %.1f ms, "
                  "discriminator optimizer_step %.2f ms (the batch's upload included in the sub-steps)"
                  % (attn, Bb, TT, TM, med["ae"], med["sp"], med["opt_gen"], med["d"], med["opt_disc"]), flush=True)
    if a.ddp:
        print("collectives issued through the native communicator: %d" % ddp._Native.issued)
        dist.destroy_process_group()


def train_cm_mode():
    import json
    from collections import defaultdict
    from types import SimpleNamespace
    from unast_amd import train, train_rnn, train_rnn_step
    from unast_amd.utils import SOS_IDX, EOS_IDX
    train.DEVICE = D
    cfgs = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "rnn_configs.json")))
    train_rnn_step.TEXT_MAX_LEN, train_rnn_step.SPEECH_MAX_LEN = TT, TM
    for attn in ("luong", "lsa"):
        for Bb in (4, 16):
            args = SimpleNamespace(**dict(cfgs["rnn_d_" + attn], load_path=None, ae_steps=1, sp_steps=1, cm_steps=1, d_steps=1, train_batch_size=Bb))
            train.set_seed(0)
            _, _, model, opt, _ = train.initialize_model(args)
            model.train()
            tm, sm = model.text_m, model.speech_m
            with torch.no_grad():                                                                 # the stop rule off: a fixed position count
                tm.postnet.fc1.bias[EOS_IDX] = -1e4
                sm.postnet.stop_linear.bias.fill_(-30.0)
            train_rnn_step.drop_cached_operands(model)
            if attn == "luong":
                # ---- the text prenet of one position, averaged over the prefixes L = 1..TT: fused against the comparator
                P = train_rnn.decoder_pack_of(tm, train_rnn.TextDecoderPack)
                bns = [bn for _, _, _, bn in P.convs]
                p = float(tm.prenet.p)
                LMAX = max(TT, 300)                                                               # (300 = infer_sequence's max_len: the longest prefix)
                tokens = torch.randint(3, 46, (Bb, LMAX), device=D)
                ids_sos = torch.cat([torch.full((Bb, 1), SOS_IDX, dtype=torch.int64, device=D), tokens], 1)
                zs = [torch.empty(Bb * LMAX, 256, device=D) for _ in range(3)]
                parts = torch.empty(3 * ops.prefix_gen_tiles(Bb, LMAX) * 512, dtype=torch.float64, device=D)
                pre = torch.empty(Bb, 256, device=D)

                def fused_at(L):
                    row0 = train_rnn.prefix_row0(Bb, L)
                    part = parts[:3 * ops.prefix_gen_tiles(Bb, L) * 512].view(3, -1, 2, 256)
                    ops.prefix_gen_conv(P.convs[0][0][0], P.convs[0][1], zs[0], part[0], Bb, L, tokens=tokens, emb=P.emb, sos=SOS_IDX, drop_p=p, seed=1,
                                        stream_id=21, row0=row0)
                    for k in (1, 2):
                        bn = bns[k - 1]
                        ops.prefix_gen_conv(P.convs[k][0][0], P.convs[k][1], zs[k], part[k], Bb, L, x=zs[k - 1], part_in=part[k - 1],
                                            bn=(bn.weight, bn.bias, bn.eps), drop_p=p, seed=1, stream_id=21 + k, row0=row0)
                    ops.prefix_gen_finish(zs[2], part, bns, pre, Bb, L, drop_p=p, seed=1, stream_id=24, row0=row0)

                def fused():
                    for L in range(1, TT + 1):
                        fused_at(L)

                mean, rstd, bn_ws = torch.empty(256, device=D), torch.empty(256, device=D), torch.empty(512, dtype=torch.float64, device=D)

                def comparator():
                    for L in range(1, TT + 1):
                        ids = ids_sos[:, :L].contiguous()
                        N = Bb * L
                        x = torch.empty(N, P.emb.shape[1], device=D)
                        ops.embed_fwd(ids, P.emb, x, L, drop_p=p, seed=1, stream_id=21)
                        cur = x.view(Bb, L, -1)
                        for k, (wp, bias, _, bn) in enumerate(P.convs):
                            z = contract.conv(cur, wp, bias, 2)
                            y = torch.empty(N, 256, device=D)
                            ops.bn_fwd(z.view(N, 256), bn.weight, bn.bias, y, mean, rstd, bn.running_mean, bn.running_var, bn_ws, 1, drop_p=p, seed=1,
                                       stream_id=22 + k, eps=bn.eps, momentum=bn.momentum, num_batches_tracked=bn.num_batches_tracked)
                            cur = y.view(Bb, L, 256)
                        pre.copy_(cur[:, -1])
                with torch.no_grad():
                    f_ms, c_ms = median_ms(fused, reps=5), median_ms(comparator, reps=5)
                print("text prenet of one position, B=%d, mean over L = 1..%d: fused %.1f us (4 launches), comparator %.1f us (23 device operations + the "
                      "last-row copy) -> x %.2f" % (Bb, TT, f_ms * 1e3 / TT, c_ms * 1e3 / TT, c_ms / f_ms), flush=True)
                # every workgroup of stages 2 and 3 reduces all the tiles' partial sums again (O(tiles^2) per launch): the cost by prefix length
                with torch.no_grad():
                    per_l = [(L, median_ms(lambda: [fused_at(L) for _ in range(20)], reps=5) * 1e3 / 20) for L in (1, 60, 180, 300)]
                print("fused text prenet of one position by prefix length, B=%d: %s" % (Bb, ", ".join("L = %d (%d tiles) %.1f us" % (L, ops.prefix_gen_tiles(Bb, L), us)
                                                                                                   for L, us in per_l)), flush=True)
            # ---- the two generations, fixed position count
            getter = train.SyntheticBatchGetter(args, t_text=TT, t_mel=TM)
            text, mel, tl, ml = train_rnn_step._process(getter._next())[:4]
            with torch.no_grad():
                s_mem = train_rnn.encoder_forward(sm, mel, ml, seed=1)
                t_mem = train_rnn.encoder_forward(tm, text, tl, seed=2)
                got = []
                gt_ms = median_ms(lambda: got.append(train_rnn.text_generate_train(tm, s_mem, ml, max_len=TT, seed=3)), reps=5)
                assert got[-1].lens_host == [TT] * Bb, got[-1].lens_host
                gs_ms = median_ms(lambda: got.append(train_rnn.speech_generate_train(sm, t_mem, tl, max_len=TM, seed=4)), reps=5)
                assert got[-1].lens_host == [TM] * Bb, got[-1].lens_host
            print("[%s] B=%d dropout on, stop rule off: text generation %d positions over a %d-frame memory %.1f ms = %.1f us per position (16 launches); "
                  "speech generation %d frames over a %d-token memory %.1f ms = %.1f us per position (15 launches; the post-net after the loop included)"
                  % (attn, Bb, TT, TM, gt_ms, gt_ms * 1e3 / TT, TM, TT, gs_ms, gs_ms * 1e3 / TM), flush=True)
            # ---- the whole sub-step
            times, losses = [], defaultdict(list)
            train.freeze_model_parameters(model.discriminator)
            for rep in range(6):                                                                  # one warm-up round, five measured
                b = getter._next()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                train_rnn_step.train_cm_step(losses, model, b, 0, 3, args)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
                train_rnn_step.optimizer_step(model, opt, args)
            assert all(bool(torch.isfinite(torch.as_tensor(v))) for vs in losses.values() for v in vs)
            print("[%s] B=%d T_text=%d T_mel=%d: CM sub-step %.1f ms (generated: %d tokens, %d frames; live PAD ids %d)"
                  % (attn, Bb, TT, TM, statistics.median(times[1:]), TT, TM, model._rnn_cm_live_pad), flush=True)


if a.train_cm:
    train_cm_mode()
    sys.exit(0)
if a.train_step:
    train_step_mode()
    sys.exit(0)
if a.train:
    train_mode()
    sys.exit(0)
if a.train_text_decoder:
    train_text_decoder_mode()
    sys.exit(0)
if a.train_decoder:
    train_decoder_mode()
    sys.exit(0)

with torch.no_grad():
    # the recurrence alone
    g = torch.Generator().manual_seed(0)
    for T, Bb in ((TM, B), (TT, B), (TM, 16)):
        xproj = torch.randn(Bb, T, 2048, generator=g).to(D)
        wfrag = ops.lstm_whh_fragments((torch.randn(2, 1024, 256, generator=g) / 16).to(D))
        bias = torch.zeros(2048, device=D)
        lens = torch.full((Bb,), T, dtype=torch.int32, device=D)
        y, hn, cn = torch.empty(Bb, T, 512, device=D), torch.empty(Bb, 512, device=D), torch.empty(Bb, 512, device=D)
        ms = median_ms(lambda: ops.lstm_seq_fwd(xproj, wfrag, bias, bias, lens, y, hn, cn))
        print("lstm_seq_fwd B=%d T=%d ndir=2: %.2f ms = %.2f us per recurrent step" % (Bb, T, ms, ms * 1e3 / T))

    text, mel, text_len, mel_len = (torch.from_numpy(x) for x in synth_batch(B, TT, TM, seed=3))
    text, mel = text.to(D), mel.to(D)
    for attn in ("luong", "lsa"):
        tm, sm = models(attn)
        print("[%s] text encoder %.2f ms, speech encoder %.2f ms" % (attn, median_ms(lambda: tm.encode(text, text_len)), median_ms(lambda: sm.encode(mel, mel_len))))
        t_eo, t_mask = tm.encode(text, text_len)
        s_eo, s_mask = sm.encode(mel, mel_len)
        for name, gen in (("text over speech memory", tm.generation(s_eo, s_mask, 300)), ("speech over text memory", sm.generation(t_eo, t_mask, 815))):
            gen.step(None)
            gen.reset()
            eager = median_ms(lambda: gen.step(None), inner=20)
            gen.reset()
            graph = _capture(lambda: gen.step(None))
            gen.reset()
            replay = median_ms(graph.replay, inner=20)
            print("[%s] one decoded position, %s: eager %.3f ms, replayed %.3f ms" % (attn, name, eager, replay))
        sm.postnet.stop_linear.bias.fill_(-30.0)                     # never stops: all frames are decoded

        def tts():                                                   # UNAST.tts(infer=True), whose infer_sequence runs at its default max_len of 815
            t_enc, t_pad = tm.encode(text, text_len)
            out = sm.infer_sequence(t_enc, t_pad, max_len=a.frames)
            assert out[0].shape[1] == a.frames
            return out
        ms = median_ms(tts, reps=3)
        print("[%s] tts: text encoder + infer_sequence of %d frames, B=%d, T_text=%d: %.1f ms" % (attn, a.frames, B, TT, ms))
