"""unast_amd.train_rnn_step on the GPU: the reference's sequence freeze(D); train_ae_step; train_sp_step; optimizer_step; unfreeze(D);
train_discriminator_step; optimizer_step through unast_amd.train's entry points, against the reference's fixtures
(tests/golden/rnn_step_{luong,lsa}.npz).  Bounds: tests/rnn_step_fixture.py.  Every figure is printed before it is asserted."""
from collections import defaultdict

import numpy as np
import pytest
import torch

from tests import rnn_step_fixture as SF

pytestmark = pytest.mark.gpu
GEN = ("text_m.", "speech_m.")


def _dev():
    return torch.device("cuda:0")


def _build(attn, case="a", drops=0.0, **over):
    from unast_amd import train
    args = SF.args_of(attn, drops, **over)
    saved = train.DEVICE
    train.DEVICE = _dev()
    try:
        _, _, model, opt, sched = train.initialize_model(args)
    finally:
        train.DEVICE = saved
    sd = SF.state_dict(attn)
    assert list(model.state_dict()) == list(sd)
    model.load_state_dict(sd)
    if case == "a_eps":
        for i in (1, 2, 3):
            getattr(model.text_m.prenet, "batch_norm%d" % i).eps = SF.meta(attn)["eps_cond"]
    return model.train(), opt, args, sd


def _gen_grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if k.startswith(GEN) and p.grad is not None}


def _disc_grads(model):
    st = model._store()
    return {k: st.gphys[k].detach().clone() for k in st.params if "reduce_c_W" not in k}


def _snapshot(model, opt, prefixes, segments):
    """State-dict entries under `prefixes` plus the moments and step counts of the optimizer segments named in `segments`."""
    out = {k: v.detach().clone() for k, v in model.state_dict().items() if k.startswith(prefixes)}
    for s in opt.segments:
        if s.name in segments:
            out["m/" + s.name], out["v/" + s.name], out["step/" + s.name] = s.m.clone(), s.v.clone(), torch.tensor(s.step)
    return out


def _sequence(model, opt, args, batch, deterministic=True, fixed_sums=None):
    """The fixture's sequence; returns everything the tests look at (device tensors; nothing is read back in between)."""
    from unast_amd import config, train, utils
    saved = (utils.is_deterministic(), config.DETERMINISTIC_SUMS, train.DEVICE)
    utils.set_deterministic(deterministic, fixed_sums=fixed_sums)
    train.DEVICE = _dev()
    r = dict(losses=defaultdict(list))
    try:
        train.freeze_model_parameters(model.discriminator)
        train.train_ae_step(r["losses"], model, batch, 0, 2, args)
        r["ae_grads"] = _gen_grads(model)
        train.train_sp_step(r["losses"], model, batch, 0, 2, args)
        r["gen_grads"] = _gen_grads(model)
        r["disc_before"] = _snapshot(model, opt, ("discriminator.",), ("disc",))
        train.optimizer_step(model, opt, args)
        r["gen_norm"], r["gen_stepped"] = opt.grad_norm(), list(opt.last_stepped)
        r["gen_grads_after"] = _gen_grads(model)
        r["disc_after_gen"] = _snapshot(model, opt, ("discriminator.",), ("disc",))
        r["gen_after_gen"] = _snapshot(model, opt, GEN, ("text_m", "speech_m"))
        train.unfreeze_model_parameters(model.discriminator)
        train.train_discriminator_step(r["losses"], model, batch, 0, 1, args)
        r["disc_grads"] = _disc_grads(model)
        r["gen_touched_in_d"] = set(model.__dict__.get("_rnn_touched", ()))
        train.optimizer_step(model, opt, args)
        r["disc_norm"], r["disc_stepped"] = opt.grad_norm(), list(opt.last_stepped)
        r["gen_after_disc"] = _snapshot(model, opt, GEN, ("text_m", "speech_m"))
        r["disc_after_disc"] = _snapshot(model, opt, ("discriminator.",), ("disc",))
        torch.cuda.synchronize()
    finally:
        utils.set_deterministic(saved[0], fixed_sums=saved[1])
        train.DEVICE = saved[2]
    return r


def _check_grads(tag, got, attn, case, phase):
    ref, gnorm, e32 = SF.reference(attn, case, phase)
    assert sorted(got) == sorted(ref), sorted(set(got) ^ set(ref))
    bounds, common = SF.grad_bounds(e32, case)
    lim = SF.meta(attn)["g_sample"]
    errs = {k: SF.rel(SF.sample(got[k].cpu().double().numpy(), lim), ref[k]) for k in bounds}
    for k in sorted(errs, key=lambda k: errs[k] / bounds[k])[-5:]:
        print("%s grad %-72s %.3g = %.3f of its bound %.3g (own e32 %.2g)" % (tag, k, errs[k], errs[k] / bounds[k], bounds[k], e32[k]))
    print("%s: common e32 %.3g; worst ratio %.3f" % (tag, common, max(errs[k] / bounds[k] for k in errs)))
    for k in SF.ILL:
        if k in errs:
            print("%s ill-conditioned %-40s err %.3g own e32 %.3g bound %.3g" % (tag, k, errs[k], e32[k], bounds[k]))
    bad = {k: "%.2e > %.2e" % (errs[k], bounds[k]) for k in errs if errs[k] > bounds[k]}
    if phase == "gen":
        deg_text = SF.DEG_ABS if case == "a_eps" else max(SF.DEG_ABS, SF.GRAD_MARGIN * e32["text_m.prenet.conv1.conv.weight"])
        for k in SF.DEGENERATE:
            r = got[k].abs().max().item() / got[k[:-4] + "weight"].norm().item()
            lim_k = deg_text if k in SF.DEG_TEXT else SF.DEG_ABS
            print("%s degenerate %-48s max|g| / ||grad W|| %.2e (bound %.2e)" % (tag, k, r, lim_k))
            if r > lim_k:
                bad[k] = "degenerate %.2e > %.2e" % (r, lim_k)
    assert not bad, bad
    return bounds


def _check_moves(tag, after, sd, attn, case, phase, bounds, ref_norm):
    """Post-step parameters against fp64 AdamW from the fixture's gradients, on the sampled elements the gradient bound pins."""
    m = SF.meta(attn)
    ref, gnorm, _ = SF.reference(attn, case, phase)
    slacks, worst = [], (0.0, None)
    for k, b in bounds.items():
        p0 = sd[k].double().numpy().reshape(-1)
        idx = SF.sample_index(p0.size, m["g_sample"])
        want = SF.adamw_first_steps(p0[idx], ref[k], ref_norm, m["lr"], m["weight_decay"], m["grad_clip"])
        got = after[k].cpu().double().numpy().reshape(-1)[idx]
        slack = SF.move_slack(ref[k], gnorm[k], p0.size, b)
        slacks.append(slack)
        tol = m["lr"] * (SF.MOVE_TOL + slack) + 4 * np.spacing(np.abs(p0[idx]).astype(np.float32)).astype(np.float64)
        ratio = float((np.abs(got - want) / tol).max())
        if ratio > worst[0]:
            worst = (ratio, k)
    print("%s post-step: %d sampled elements, %.4f of them allowed more than lr / 2; worst |dp - dp_ref| / allowance %.3g (%s)"
          % (tag, sum(v.size for v in slacks), SF.loose_share(slacks), worst[0], worst[1]))
    assert worst[0] <= 1.0, worst


def _assert_same(a, b, what):
    assert sorted(a) == sorted(b)
    differ = [k for k in a if not torch.equal(a[k], b[k])]
    assert not differ, (what, differ)


# ---- 1. the whole sequence against the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SF.CASES)
@pytest.mark.parametrize("attn", SF.ATTNS)
def test_sequence_matches_the_reference_fixture(attn, case):
    fx = SF.fixture(attn)
    model, opt, args, sd = _build(attn, case)
    assert model.discriminator.rnn.rnn.input_size == 512
    r = _sequence(model, opt, args, SF.batch(attn, case))
    tag = "%s %s" % (attn, case)
    for k in SF.LOSS_KEYS:
        assert len(r["losses"][k]) == 1
        got, want = float(r["losses"][k][0]), float(fx["%s/loss/%s" % (case, k)])
        print("%s loss %-5s %.6f ref %.6f err %.2e (bound %.1e, e32 %.1e)" % (tag, k, got, want, abs(got - want), SF.LOSS_TOL * max(1.0, abs(want)), float(fx["e32/%s/loss/%s" % (case, k)])))
        assert abs(got - want) <= SF.LOSS_TOL * max(1.0, abs(want)), k
    assert r["gen_stepped"] == ["text_m", "speech_m"] and r["disc_stepped"] == ["disc"] and r["gen_touched_in_d"] == set()
    bounds = _check_grads(tag + " gen", r["gen_grads"], attn, case, "gen")
    for ph in ("gen", "disc"):
        want = float(fx["%s/%s/norm" % (case, ph)])
        print("%s %s pre-clip norm %.6f ref %.6f rel %.2e (bound %.2e)" % (tag, ph, r[ph + "_norm"], want, abs(r[ph + "_norm"] - want) / want, SF.norm_bound(fx, case, ph)))
        assert abs(r[ph + "_norm"] - want) <= SF.norm_bound(fx, case, ph) * want
    _check_moves(tag + " gen", r["gen_after_gen"], sd, attn, case, "gen", bounds, float(fx["%s/gen/norm" % case]))
    # the generator phase leaves the frozen discriminator alone: parameters, moments, step count
    _assert_same(r["disc_before"], r["disc_after_gen"], "discriminator after the generator optimizer_step")
    assert int(r["disc_after_gen"]["step/disc"]) == 0
    assert all(float(g.abs().max()) == 0.0 for g in r["gen_grads_after"].values()), "optimizer_step leaves all gradients zero or absent"
    # the discriminator phase: its gradients, its move, and the generators untouched but for the encoders' running statistics
    dbounds = _check_grads(tag + " disc", r["disc_grads"], attn, case, "disc")
    _check_moves(tag + " disc", r["disc_after_disc"], sd, attn, case, "disc", dbounds, float(fx["%s/disc/norm" % case]))
    assert int(r["disc_after_disc"]["step/disc"]) == 1 and int(r["gen_after_disc"]["step/text_m"]) == 1 and int(r["gen_after_disc"]["step/speech_m"]) == 1
    moved = [k for k in r["gen_after_gen"] if not torch.equal(r["gen_after_gen"][k], r["gen_after_disc"][k])]
    want_moved = [k for k in SF.group(fx, "%s/disc/state" % case) if k.startswith(GEN)] + ["text_m.prenet.batch_norm%d.num_batches_tracked" % i for i in (1, 2, 3)]
    assert sorted(moved) == sorted(want_moved), sorted(set(moved) ^ set(want_moved))
    assert all(k.endswith(SF.BUFFERS) for k in moved)
    final = dict(r["gen_after_disc"], **r["disc_after_disc"])
    for ph, snap in (("gen", r["gen_after_gen"]), ("disc", final)):
        nbt = __import__("json").loads(str(fx["%s/%s/num_batches_tracked" % (case, ph)]))
        assert {k: int(snap[k]) for k in nbt} == nbt
        state = SF.group(fx, "%s/%s/state" % (case, ph))
        e32s = dict(zip(state, fx["e32/%s/%s/state" % (case, ph)].tolist()))
        for k, want in state.items():
            if k.endswith(("running_mean", "running_var")):
                got = SF.sample(snap[k].cpu().double().numpy(), SF.meta(attn)["p_sample"])
                err, lim = np.abs(got - want).max(), SF.buffer_bound(k, want, case, ph)
                print("%s after %-4s %-46s err %.3g (bound %.3g, the reference's own fp32 run %.3g)" % (tag, ph, k, err, lim, e32s[k]))
                assert err <= lim, (ph, k, err, lim)


# ---- 2. accumulation, what optimizer_step leaves behind, padded rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("attn", SF.ATTNS)
def test_two_identical_substeps_accumulate_and_padded_rows_get_exact_zeros(attn):
    from unast_amd import train, train_rnn_step, utils
    model, opt, args, sd = _build(attn, "b")
    buffers = {k: v.clone() for k, v in model.state_dict().items() if k.endswith(SF.BUFFERS)}
    batch = SF.batch(attn, "b")
    saved = (utils.is_deterministic(), train.DEVICE)
    utils.set_deterministic(True)
    train.DEVICE, train_rnn_step.RECORD = _dev(), True
    try:
        train.freeze_model_parameters(model.discriminator)
        losses = defaultdict(list)
        train.train_ae_step(losses, model, batch, 0, 2, args)
        rec = model._rnn_step_record
        for d, lens in ((rec["d_t_enc"], batch[2]), (rec["d_s_enc"], batch[3])):
            assert d.abs().max().item() > 0.0
            for b, n in enumerate(lens.tolist()):
                assert d[b, n:].abs().sum().item() == 0.0, "d_enc_output rows past a sequence's length must get exact zeros from the discriminator"
        first = _gen_grads(model)
        model.load_state_dict(buffers, strict=False)                                             # the same running statistics for the second sub-step
        train.train_ae_step(losses, model, batch, 0, 2, args)
        second = _gen_grads(model)
    finally:
        utils.set_deterministic(saved[0])
        train.DEVICE, train_rnn_step.RECORD = saved[1], False
        model.__dict__.pop("_rnn_step_record", None)
    worst = max(SF.rel(second[k].cpu().double().numpy(), 2 * first[k].cpu().double().numpy()) for k in first if k not in SF.DEGENERATE)
    print("%s two identical sub-steps against twice the first: %.2e" % (attn, worst))
    assert worst <= 1e-5
    assert abs(float(losses["t_ae"][0]) - float(losses["t_ae"][1])) <= 1e-6 * float(losses["t_ae"][0])
    assert model._store().touched == set(), "the frozen discriminator must not produce gradients"
    train.optimizer_step(model, opt, args)
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in model.parameters())
    assert model.__dict__["_rnn_touched"] == set()
    for m in (model.text_m, model.speech_m):
        assert not {"_rnn_pack", "_rnn_train_pack", "_rnn_decoder_train_pack"} & set(m.__dict__), "cached operands must be dropped after a step"


# ---- 3. bit-equality of two runs with fixed sums -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attn", SF.ATTNS)
def test_two_runs_with_fixed_sums_agree_to_the_bit(attn):
    runs = []
    for _ in range(2):
        model, opt, args, sd = _build(attn, "a")
        runs.append(_sequence(model, opt, args, SF.batch(attn, "a"), fixed_sums=True))
    a, b = runs
    for k in SF.LOSS_KEYS:
        assert torch.equal(a["losses"][k][0], b["losses"][k][0]), k
    for part in ("gen_grads", "disc_grads", "gen_after_gen", "gen_after_disc", "disc_after_disc"):
        _assert_same(a[part], b[part], part)


# ---- 4. the configs' dropout rates, noise, SpecAugment and a drawn permutation, against the mirror under the kernels' own masks ------------------------
def _tape_masks(tape):
    from tests import dropout_mirror as DM
    masks = {}
    for s in tape.sites:
        epoch = int(s.epoch.item())
        if s.kind == "row":
            masks[s.name] = torch.from_numpy(DM.row_keep(s.seed, s.stream, s.rows, s.p, epoch).astype(np.float64))
        else:
            masks[s.name] = torch.from_numpy(DM.drop_factor(s.seed, s.stream, s.rows, s.cols, s.p, epoch))
    return masks


def _record_masks(rec):
    return {name: _tape_masks(t) for name, t in rec["tapes"].items()}, [int(v) for v in rec["perm"].tolist()]


@pytest.mark.parametrize("attn", SF.ATTNS)
def test_dropout_noise_and_permutation_match_the_mirror_under_the_kernels_masks(attn):
    """Non-deterministic mode with a fixed seed on case a_eps at the configs' rates 0.5 / 0.3 / 0.1.  The discriminator's own dropout (0.2,
    seeded inside its forward) is switched off: its sites are not on a tape."""
    from tests import rnn_step_mirror as SM
    from unast_amd import train, train_rnn_step, utils
    case = "a_eps"
    model, opt, args, sd = _build(attn, case, drops=None)
    assert (args.t_pre_drop, args.d_drop, args.t_post_drop) == (0.5, 0.3, 0.1)
    model.discriminator.dropout_p = 0.0
    batch = SF.batch(attn, case)
    saved = (utils.is_deterministic(), train.DEVICE)
    utils.set_seed(20241)
    utils.set_deterministic(False)
    train.DEVICE, train_rnn_step.RECORD = _dev(), True
    masks, perms, losses = {}, {}, defaultdict(list)
    try:
        train.freeze_model_parameters(model.discriminator)
        train.train_ae_step(losses, model, batch, 0, 2, args)
        masks["ae"], perms["ae"] = _record_masks(model._rnn_step_record)
        assert [s.name for s in model._rnn_step_record["tapes"]["text_enc"].sites][:2] == ["emb_dropout", "noise"]
        train.train_sp_step(losses, model, batch, 0, 2, args)
        masks["sp"], perms["sp"] = _record_masks(model._rnn_step_record)
        mel_aug = model._rnn_step_record["mel_aug"].cpu().double()
        gen_grads = _gen_grads(model)
        train.optimizer_step(model, opt, args)
        gen_norm = opt.grad_norm()
        train.unfreeze_model_parameters(model.discriminator)
        train.train_discriminator_step(losses, model, batch, 0, 1, args)
        masks["d"], perms["d"] = _record_masks(model._rnn_step_record)
        assert len(model._rnn_step_record["tapes"]["text_enc"].sites) >= 4, "the D step's encoders run with dropout on"
        disc_grads = _disc_grads(model)
        train.optimizer_step(model, opt, args)
        disc_norm = opt.grad_norm()
        torch.cuda.synchronize()
    finally:
        utils.set_deterministic(saved[0])
        train.DEVICE, train_rnn_step.RECORD = saved[1], False
        model.__dict__.pop("_rnn_step_record", None)
    assert any(p != list(range(len(p))) for p in perms.values()), perms
    print("%s permutations %s" % (attn, perms))
    text, mel, tl, ml = batch
    eps = SF.meta(attn)["eps_cond"]
    r64 = SM.run_sequence(sd, attn, args, (text, mel.double(), tl, ml), eps_text=eps, masks=masks, perms=perms, mel_aug=mel_aug)
    r32 = SM.run_sequence(sd, attn, args, (text, mel, tl, ml), dtype=torch.float32, eps_text=eps, masks=masks, perms=perms, mel_aug=mel_aug.float())
    tag = attn + " dropout"
    for k in SF.LOSS_KEYS:
        got, want = float(losses[k][0]), r64["losses"][k]
        print("%s loss %-5s %.6f mirror %.6f err %.2e" % (tag, k, got, want, abs(got - want)))
        assert abs(got - want) <= SF.LOSS_TOL * max(1.0, abs(want)), k
    for ph, got, norm in (("gen", gen_grads, gen_norm), ("disc", disc_grads, disc_norm)):
        want, w32 = r64[ph + "_grads"], r32[ph + "_grads"]
        assert sorted(got) == sorted(want)
        e32 = {k: SF.rel(w32[k].numpy(), want[k].numpy()) for k in want}
        bounds, common = SF.grad_bounds(e32, case)
        errs = {k: SF.rel(got[k].cpu().double().numpy(), want[k].numpy()) for k in bounds}
        for k in sorted(errs, key=lambda k: errs[k] / bounds[k])[-4:]:
            print("%s %s grad %-72s %.3g = %.3f of its bound %.3g (mirror's own e32 %.2g)" % (tag, ph, k, errs[k], errs[k] / bounds[k], bounds[k], e32[k]))
        bad = {k: "%.2e > %.2e" % (errs[k], bounds[k]) for k in errs if errs[k] > bounds[k]}
        assert not bad, bad
        print("%s %s pre-clip norm %.6f mirror %.6f" % (tag, ph, norm, r64[ph + "_norm"]))
        assert abs(norm - r64[ph + "_norm"]) <= SF.NORM_TOL * r64[ph + "_norm"]


# ---- 5. the loops ---------------------------------------------------------------------------------------------------------------------------------------
def test_train_and_train_step_run_an_rnn_config_without_cross_model_steps():
    from unast_amd import train
    args = SF.args_of("lsa", drops=None, epochs=1, epoch_steps=2, train_batch_size=2, seed=5, checkpoint_path=None, d_steps=2)
    saved = train.DEVICE
    train.DEVICE = _dev()
    try:
        getter = train.SyntheticBatchGetter(args, t_text=6, t_mel=10)
        model, history = train.train(args, batch_getter=getter)
        assert len(history) == 1 and sorted(history[0]) == sorted(SF.LOSS_KEYS)
        assert all(np.isfinite(v) for v in history[0].values()), history
        _, _, model, opt, sched = train.initialize_model(args)
        losses = defaultdict(list)
        b = getter._next
        train.train_step(losses, model, opt, sched, dict(unsup=[b()], sup=[b()], cm=[], disc=[b(), b()]), 0, args)
        torch.cuda.synchronize()
        assert sorted(losses) == sorted(SF.LOSS_KEYS) and len(losses["d"]) == 2
        assert all(bool(torch.isfinite(v)) for vs in losses.values() for v in vs)
        assert [s.step for s in opt.segments] == [1, 1, 1] and sched.last_epoch == 1
    finally:
        train.DEVICE = saved
