"""unast_amd.eval_rnn on the GPU against the reference's own evaluate() (tests/golden/rnn_eval_{luong,lsa}.npz, tools/gen_golden_rnn_eval.py) and
its invariants.  Bounds: tests/rnn_eval_fixture.py.  Every figure is printed before it is asserted."""
import json
import os

import numpy as np
import pytest
import torch

from tests import rnn_eval_fixture as EF
from tests import rnn_step_fixture as SF

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


@pytest.fixture
def eval_mode(monkeypatch):
    """Parity mode (identity noise, specaugment and permutation, as the fixtures were made) on cuda:0."""
    from unast_amd import config, train, utils
    saved = (utils.is_deterministic(), config.DETERMINISTIC_SUMS)
    utils.set_deterministic(True)
    monkeypatch.setattr(train, "DEVICE", _dev())
    yield
    utils.set_deterministic(saved[0], fixed_sums=saved[1])


def _build(attn, case, **over):
    from unast_amd import train
    args = SF.args_of(attn, None, **over)
    _, _, model, opt, _ = train.initialize_model(args)
    sd = EF.state_dict(attn, case)
    if not args.use_discriminator:
        sd = {k: v for k, v in sd.items() if not k.startswith("discriminator.")}
    assert list(model.state_dict()) == list(sd)
    model.load_state_dict(sd)
    return model, opt, args


def _caps(monkeypatch, attn, case):
    from unast_amd import eval_rnn
    fx = EF.setup(attn, case)
    monkeypatch.setattr(eval_rnn, "TEXT_MAX_LEN", fx["max_text"])
    monkeypatch.setattr(eval_rnn, "SPEECH_MAX_LEN", fx["max_speech"])
    return fx


def _state(model, opt):
    out = {"sd/" + k: v.detach().clone() for k, v in model.state_dict().items()}
    out.update({"grad/" + k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None})
    out["grad_names"] = sorted(k for k, p in model.named_parameters() if p.grad is not None)
    for s in opt.segments:
        out["m/" + s.name], out["v/" + s.name], out["step/" + s.name] = s.m.clone(), s.v.clone(), torch.tensor(s.step)
    out["touched"] = sorted(model.__dict__.get("_rnn_touched", ()))
    return out


def _same_state(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        same = torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k]
        assert same, k


@pytest.mark.parametrize("case", EF.CASES)
@pytest.mark.parametrize("attn", EF.ATTNS)
def test_evaluate_against_the_reference(attn, case, eval_mode, monkeypatch, tmp_path):
    from unast_amd import eval_rnn, train_rnn_step, utils
    fx, ref = _caps(monkeypatch, attn, case), EF.fixture(attn)
    model, opt, args = _build(attn, case, eval_batch_size=EF.setup(attn, case)["B"], out_test_dir=str(tmp_path))
    batch = EF.batch(attn, case)
    fnames = ["utt%d" % b for b in range(fx["B"])]
    before = _state(model, opt)
    per, losses = eval_rnn.evaluate(model, [batch], 0, args)
    per_t, losses_t, d_score = eval_rnn.evaluate(model, [(batch, fnames)], 0, args, is_test=True)
    _same_state(before, _state(model, opt))
    assert not model.training
    assert tuple(losses) == tuple(losses_t) == EF.KEYS_D
    bad = []
    for k in EF.KEYS_D:
        want, got = float(ref["%s/loss/%s" % (case, k)]), losses[k][0]
        tol = EF.LOSS_TOL * max(1.0, abs(want))
        print("%s %s loss %-5s got %.6f ref %.6f err %.2e bound %.2e (reference's own e32 %.1e)" % (attn, case, k, got, want, abs(got - want), tol,
                                                                                                 float(ref["e32/%s/loss/%s" % (case, k)])))
        assert losses_t[k][0] == got, "is_test changes no loss"
        if not abs(got - want) <= tol:
            bad.append(k)
    assert not bad, bad
    # the tokens behind PER, and PER itself against the host function
    content = json.load(open(os.path.join(str(tmp_path), "text_preds.json")))
    assert json.dumps(content, sort_keys=True) == str(ref["%s/json" % case])
    tok, lens = ref["%s/asr/tokens" % case], ref["%s/asr/lens" % case]
    for b, f in enumerate(fnames):
        assert content[f]["pred"] == tok[b, :lens[b]].tolist()
    want_per = utils.compute_per(batch[0], torch.from_numpy(tok), batch[2], torch.from_numpy(lens))
    print("%s %s PER %.6f (host, of the fixture's tokens: %.6f) d_score %.4f (ref %.4f)" % (attn, case, per, want_per, d_score, float(ref["%s/d_score" % case])))
    assert per == per_t == want_per and d_score == float(ref["%s/d_score" % case])
    # the saved frames
    stop_lens = ref["%s/tts/stop_lens" % case]
    for b, f in enumerate(fnames):
        got = np.load(os.path.join(str(tmp_path), "mels", f + ".pt.npy"))
        assert got.shape[0] == stop_lens[b]
        want = ref["%s/mels/%d" % (case, b)]
        err, bound = np.abs(SF.sample(got, EF.meta(attn)["frame_sample"]) - want).max(), EF.frame_bound(ref, "%s/mels" % case, want)
        print("%s %s frames of %s: err %.3g bound %.3g" % (attn, case, f, err, bound))
        assert err <= bound
    # the stop logits of the TTS inference behind the saved frames (evaluate() keeps only frames and lengths: the same generation once more)
    with torch.no_grad():
        text_d, _, tl, _, _, _ = eval_rnn._process(batch)
        t_mem, t_mask, _ = eval_rnn._encode(model.text_m, text_d, tl)
        _, _, tts_stop, tts_lens = model.speech_m.generation(t_mem, t_mask, eval_rnn.SPEECH_MAX_LEN).run()
    want = ref["%s/tts/stop" % case]
    err, bound = np.abs(tts_stop.cpu().double().numpy() - want).max(), EF.frame_bound(ref, "%s/tts/stop" % case, want)
    print("%s %s TTS stop logits: err %.3g bound %.3g" % (attn, case, err, bound))
    assert tts_lens.tolist() == stop_lens.tolist() and err <= bound
    # the cross-model generations
    monkeypatch.setattr(train_rnn_step, "RECORD", True)
    eval_rnn.crossmodel_losses(model, batch, args)
    rec = model._rnn_step_record
    assert torch.equal(rec["gen_text"][0].cpu(), torch.from_numpy(ref["%s/cm/tokens" % case])) and rec["gen_text"][1].tolist() == ref["%s/cm/text_lens" % case].tolist()
    assert rec["gen_speech"][3].tolist() == ref["%s/cm/speech_lens" % case].tolist() and rec["live_pad"] == 0 == model._rnn_cm_live_pad
    for name, got in (("post", rec["gen_speech"][1]), ("stop", rec["gen_speech"][2])):
        want = ref["%s/cm/%s" % (case, name)]
        err, bound = np.abs(got.cpu().double().numpy() - want).max(), EF.frame_bound(ref, "%s/cm/%s" % (case, name), want)
        print("%s %s generated %s: err %.3g bound %.3g" % (attn, case, name, err, bound))
        assert err <= bound


@pytest.mark.parametrize("attn", EF.ATTNS)
def test_two_batches_noise_on_without_discriminator_and_batch_of_one(attn, monkeypatch, tmp_path):
    """evaluate() over two batches with noise and specaugment ON (what a user runs): PER is the host function's of the read-back tokens, the
    record holds the sites, the state stays put; then six losses plus PER (the reference's seven values) without a discriminator, and B = 1."""
    from unast_amd import eval_rnn, train, train_rnn_step, utils
    monkeypatch.setattr(train, "DEVICE", _dev())
    monkeypatch.setitem(utils._RNG, "deterministic", False)            # whatever an earlier test left: noise, specaugment and the permutation are ON here
    _caps(monkeypatch, attn, "a")
    utils.set_seed(3)
    model, opt, args = _build(attn, "a", eval_batch_size=3, out_test_dir=str(tmp_path))
    batches = [EF.batch(attn, "a"), EF.batch(attn, "b")]
    before = _state(model, opt)
    seen = []
    real = utils.compute_per_device
    monkeypatch.setattr(utils, "compute_per_device", lambda gt, hyp, gl, hl: seen.append((gt.cpu(), hyp.cpu(), gl.cpu(), hl.cpu())) or real(gt, hyp, gl, hl))
    per, losses = eval_rnn.evaluate(model, batches, 0, args)
    assert len(seen) == 2 and per == sum(utils.compute_per(*s) for s in seen) / 2
    assert tuple(losses) == EF.KEYS_D and all(len(v) == 2 and all(np.isfinite(x) for x in v) for v in losses.values())
    monkeypatch.setattr(train_rnn_step, "RECORD", True)
    a1 = eval_rnn.autoencoder_losses(model, batches[0], args)
    rec = dict(model._rnn_step_record)
    assert rec["sites"]["text_noise"].kind == "row" and rec["sites"]["text_noise"].rows == 3 * 7 and rec["sites"]["speech_noise"].rows == 3 * 12
    assert rec["seeds"][0] != rec["seeds"][1] and rec["perm"].numel() == 6
    eval_rnn.supervised_losses(model, batches[0], args)
    assert model._rnn_step_record["mel_aug"].shape == (3, 12, 80) and not torch.equal(model._rnn_step_record["mel_aug"].cpu(), batches[0][1])
    utils.set_deterministic(True)
    try:
        a0 = eval_rnn.autoencoder_losses(model, batches[0], args)
        assert model._rnn_step_record["sites"] == dict(text_noise=None, speech_noise=None)
    finally:
        utils.set_deterministic(False)
    print(attn, "t_ae / s_ae with noise", a1[0].item(), a1[1].item(), "without", a0[0].item(), a0[1].item())
    assert a1[0].item() != a0[0].item() and a1[1].item() != a0[1].item()            # the row masks reach both encoders
    d_loss, (d_out, d_target) = eval_rnn.discriminator_eval(model, batches[0], args)
    assert d_out.shape == d_target.shape == (6,) and sorted(set(np.round(d_target.cpu().double().numpy(), 4).tolist())) == [0.1, 0.9]
    monkeypatch.setattr(train_rnn_step, "RECORD", False)
    _same_state(before, _state(model, opt))
    with pytest.raises(ValueError, match="empty"):
        eval_rnn.evaluate(model, [], 0, args)
    # without a discriminator: the reference's seven values (six losses and PER)
    plain, opt_p, args_p = _build(attn, "a", use_discriminator=False)
    per_p, losses_p = eval_rnn.evaluate(plain, batches[:1], 0, args_p)
    assert tuple(losses_p) == EF.KEYS_PLAIN and 0.0 <= per_p
    # B = 1: eval mode has no batch statistics
    one = tuple(x[:1] for x in batches[1])
    per_1, losses_1 = eval_rnn.evaluate(model, [one], 0, args)
    assert all(np.isfinite(v[0]) for v in losses_1.values())
    _same_state(before, _state(model, opt))


def test_a_train_step_after_evaluate_gives_the_same_bits(monkeypatch, tmp_path):
    from collections import defaultdict
    from unast_amd import eval_rnn, train, utils
    monkeypatch.setattr(train, "DEVICE", _dev())
    _caps(monkeypatch, "lsa", "a")
    batch = EF.batch("lsa", "a")
    got = []
    was = utils.is_deterministic()
    utils.set_deterministic(True, fixed_sums=True)
    try:
        for with_eval in (False, True):
            model, opt, args = _build("lsa", "a")
            model.train()
            if with_eval:
                eval_rnn.evaluate(model, [batch], 0, args)
            utils.set_seed(0)                               # the step's dropout seeds (every discriminator forward draws one, evaluate()'s four too)
            losses = defaultdict(list)
            train.freeze_model_parameters(model.discriminator)
            train.train_ae_step(losses, model, batch, 0, 1, args)
            assert model.training
            got.append(({k: v[0].clone() for k, v in losses.items()}, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None},
                        {k: v.clone() for k, v in model.state_dict().items()}))
    finally:
        utils.set_deterministic(was, fixed_sums=False)
    for a, b in zip(got[0], got[1]):
        assert sorted(a) == sorted(b)
        for k in a:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("attn", EF.ATTNS)
def test_noise_on_against_the_mirror(attn, monkeypatch):
    """Noise, specaugment and the permutation ON: every entry point against the fp64 mirror (tests/rnn_eval_mirror.py) fed the row masks rebuilt
    from the recorded sites with tests/dropout_mirror.py, the recorded mel_aug and the recorded permutations.  Bound: the losses' LOSS_TOL x
    max(1, |ref|); the generated tokens and lengths are exact (the entry points return losses only: no frame leaves them under noise)."""
    from tests import rnn_eval_mirror as EM
    from unast_amd import eval_rnn, train, train_rnn_step, utils
    monkeypatch.setattr(train, "DEVICE", _dev())
    monkeypatch.setitem(utils._RNG, "deterministic", False)
    monkeypatch.setattr(train_rnn_step, "RECORD", True)
    fx = _caps(monkeypatch, attn, "a")
    utils.set_seed(5)
    model, opt, args = _build(attn, "a")
    batch = EF.batch(attn, "a")
    B = fx["B"]
    got, noise, perms = {}, {}, {}
    t_ae, s_ae, d_ae = eval_rnn.autoencoder_losses(model, batch, args)
    rec = model._rnn_step_record
    noise = dict(text=EM.site_keep(rec["sites"]["text_noise"], B), speech=EM.site_keep(rec["sites"]["speech_noise"], B))
    perms["ae"] = rec["perm"].tolist()
    print(attn, "rows kept: text", noise["text"].int().tolist(), "speech", noise["speech"].int().tolist(), "perm", perms["ae"])
    assert not noise["text"].all() and not noise["speech"].all(), "choose a seed whose masks drop a row on both sides"
    asr, tts, d_sp = eval_rnn.supervised_losses(model, batch, args)
    mel_aug, perms["sp"] = model._rnn_step_record["mel_aug"].cpu(), model._rnn_step_record["perm"].tolist()
    assert not torch.equal(mel_aug, batch[1])
    t_cm, s_cm, d_cm = eval_rnn.crossmodel_losses(model, batch, args)
    rec = model._rnn_step_record
    perms["cm"], gen_text, gen_speech = rec["perm"].tolist(), rec["gen_text"], rec["gen_speech"]
    dis, (d_out, d_target) = eval_rnn.discriminator_eval(model, batch, args)
    perms["dis"] = model._rnn_step_record["perm"].tolist()
    got = dict(t_ae=t_ae, s_ae=s_ae, d_ae=d_ae, asr=asr, tts=tts, d_sp=d_sp, s_cm=s_cm, t_cm=t_cm, d_cm=d_cm, dis=dis)
    assert len({tuple(p) for p in perms.values()}) > 1, "the permutations are drawn per call"
    mir = EM.evaluate_batch(EF.state_dict(attn, "a"), attn, args, batch, fx["max_text"], fx["max_speech"], noise=noise, mel_aug=mel_aug, perms=perms)
    plain = EM.evaluate_batch(EF.state_dict(attn, "a"), attn, args, batch, fx["max_text"], fx["max_speech"], only=("ae", "sp"))["losses"]
    assert torch.equal(gen_text[0].cpu(), mir["cm_text"][0]) and gen_text[1].tolist() == mir["cm_text"][1].tolist() and gen_speech[3].tolist() == mir["cm_speech"][3].tolist()
    bad = []
    for k in EF.KEYS_D:
        want, g = mir["losses"][k], got[k].item()
        tol = EF.LOSS_TOL * max(1.0, abs(want))
        print("%s noise-on %-5s got %.6f mirror %.6f err %.2e bound %.2e%s" % (attn, k, g, want, abs(g - want), tol,
                                                                              "  (without noise: %.6f)" % plain[k] if k in plain else ""))
        if not abs(g - want) <= tol:
            bad.append(k)
    assert not bad, bad
    for k in ("t_ae", "s_ae", "d_ae", "asr", "d_sp"):             # what the masks and the augmentation must move, far beyond the bound
        assert abs(mir["losses"][k] - plain[k]) > 10 * EF.LOSS_TOL * max(1.0, abs(plain[k])), k
    assert torch.equal(torch.sigmoid(d_out).round().cpu(), torch.sigmoid(mir["d_out"]).round().float()) and torch.allclose(d_target.cpu().double(), mir["d_target"], atol=1e-6)


@pytest.mark.parametrize("attn", EF.ATTNS)
def test_is_test_over_two_batches(attn, eval_mode, monkeypatch, tmp_path):
    """evaluate(is_test=True) over two batches with one weight set: text_preds.json accumulates both batches, every utterance has its mel file,
    PER and d_score are the means of the per-batch values, the losses are the per-batch losses in order."""
    from unast_amd import eval_rnn
    _caps(monkeypatch, attn, "a")
    dirs = [str(tmp_path / n) for n in ("both", "first", "second")]
    batches = [EF.batch(attn, "a"), EF.batch(attn, "b")]
    names = [["a%d" % b for b in range(3)], ["b%d" % b for b in range(2)]]
    model, opt, args = _build(attn, "a", eval_batch_size=3, out_test_dir=dirs[0])
    per, losses, d_score = eval_rnn.evaluate(model, list(zip(batches, names)), 0, args, is_test=True)
    singles = []
    for i in (0, 1):
        args.out_test_dir = dirs[1 + i]
        singles.append(eval_rnn.evaluate(model, [(batches[i], names[i])], 0, args, is_test=True))
    print(attn, "PER", per, [s[0] for s in singles], "d_score", d_score, [s[2] for s in singles])
    assert per == (singles[0][0] + singles[1][0]) / 2 and d_score == (singles[0][2] + singles[1][2]) / 2
    assert round(singles[1][2] * 6, 9) in (0, 1, 2, 3, 4), "the second batch's 4 rows over eval_batch_size = 3, as the reference divides"
    for k in EF.KEYS_D:
        assert losses[k] == singles[0][1][k] + singles[1][1][k], k
    content = [json.load(open(os.path.join(d, "text_preds.json"))) for d in dirs]
    assert sorted(content[0]) == sorted(names[0] + names[1]) and content[0] == {**content[1], **content[2]}
    text, tl = batches[1][0], batches[1][2]
    assert content[0]["b1"]["gt"] == text[1, :tl[1]].tolist()
    for i in (0, 1):
        for f in names[i]:
            a, b = (np.load(os.path.join(d, "mels", f + ".pt.npy")) for d in (dirs[0], dirs[1 + i]))
            assert a.shape == b.shape and a.shape[1] == 80 and np.array_equal(a, b), f
    assert sorted(os.listdir(os.path.join(dirs[0], "mels"))) == sorted(f + ".pt.npy" for f in names[0] + names[1])


def test_conv_taps_fwd_takes_a_single_sequence_with_any_batch_stride():
    """A [1, T, C] slice of a longer buffer (what .contiguous() leaves of a B = 1 generation's frames) gives the bits of a dense copy; with
    B = 2 such a slice is still refused."""
    from unast_amd import ops
    torch.manual_seed(0)
    dev = _dev()
    W, bias = torch.randn(16, 5, 8, device=dev), torch.randn(16, device=dev)
    for B in (1, 2):
        buf = torch.randn(B, 9, 8, device=dev)
        x = buf[:, :6]
        dense, out = torch.empty(B, 6, 16, device=dev), torch.empty(B, 6, 16, device=dev)
        ops.conv_taps_fwd(x.clone(), W, bias, dense, 4)
        if B == 1:
            assert x.stride(0) != 6 * x.stride(1)
            ops.conv_taps_fwd(x, W, bias, out, 4)
            assert torch.equal(out, dense)
        else:
            with pytest.raises(ValueError, match="dense batch strides"):
                ops.conv_taps_fwd(x, W, bias, out, 4)
