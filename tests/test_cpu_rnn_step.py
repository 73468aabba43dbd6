"""CPU side of unast_amd.train_rnn_step: the fp64 mirror (tests/rnn_step_mirror.py) against the reference's fixtures
(tests/golden/rnn_step_{luong,lsa}.npz), planted faults in the mirror against the GPU bounds (tests/rnn_step_fixture.py), initialize_model
for every RNN config of the reference, the refusals that remain, and the optimizer's state_dict format.

Mirror agreement (fp64 against the reference's fp64 run; the label-smoothed targets are float32 constants on both sides): losses 1e-6, gradients
1e-6 in relative L2 norm on the fixture's samples, pre-clip norm 1e-7 relative, post-step parameters and running statistics 1e-7 absolute --
30 times below the tightest GPU bound.  A planted fault has to move some checked quantity by at least 100 x its GPU bound."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import rnn_step_fixture as SF
from tests import rnn_step_mirror as SM

LOSS_AGREE, GRAD_AGREE, NORM_AGREE, STATE_AGREE = 1e-6, 1e-6, 1e-7, 1e-7
FAULT_FACTOR = 100.0
_RUNS = {}


def _mirror(attn, case, fault=None):
    key = (attn, case, fault)
    if key not in _RUNS:
        eps = SF.meta(attn)["eps_cond"] if case == "a_eps" else 1e-5
        text, mel, tl, ml = SF.batch(attn, case)
        mel = torch.from_numpy(SF.fixture(attn)[("a" if case == "a_eps" else case) + "/mel"])    # fp64, as the reference's fp64 run read it
        _RUNS[key] = SM.run_sequence(SF.state_dict(attn), attn, SF.args_of(attn), (text, mel, tl, ml), eps_text=eps, fault=fault)
    return _RUNS[key]


def _grad_errs(r, attn, case, phase):
    ref, _, _ = SF.reference(attn, case, phase)
    got = r[phase + "_grads"]
    assert sorted(got) == sorted(ref), sorted(set(got) ^ set(ref))
    lim = SF.meta(attn)["g_sample"]
    return {k: SF.rel(SF.sample(got[k].numpy(), lim), ref[k]) for k in ref if k not in SF.DEGENERATE}


@pytest.mark.parametrize("case", SF.CASES)
@pytest.mark.parametrize("attn", SF.ATTNS)
def test_mirror_reproduces_the_fixture(attn, case):
    fx, r = SF.fixture(attn), _mirror(attn, case)
    worst_loss = max(abs(r["losses"][k] - float(fx["%s/loss/%s" % (case, k)])) for k in SF.LOSS_KEYS)
    assert sorted(r["losses"]) == sorted(SF.LOSS_KEYS) and worst_loss <= LOSS_AGREE
    report = ["losses %.2e" % worst_loss]
    for ph in ("gen", "disc"):
        errs = _grad_errs(r, attn, case, ph)
        worst = max(errs, key=errs.get)
        nerr = abs(r[ph + "_norm"] - float(fx["%s/%s/norm" % (case, ph)])) / float(fx["%s/%s/norm" % (case, ph)])
        state = SF.group(fx, "%s/%s/state" % (case, ph))
        serr = max(np.abs(SF.sample(r[ph + "_state"][k].numpy(), SF.meta(attn)["p_sample"]) - v).max() for k, v in state.items() if k not in SF.DEGENERATE)
        report.append("%s: grads %.2e (%s) norm %.2e state %.2e" % (ph, errs[worst], worst, nerr, serr))
        assert errs[worst] <= GRAD_AGREE and nerr <= NORM_AGREE and serr <= STATE_AGREE, report
        nbt = json.loads(str(fx["%s/%s/num_batches_tracked" % (case, ph)]))
        assert {k: int(r[ph + "_state"][k]) for k in nbt} == nbt
    steps = json.loads(str(fx["%s/opt_steps" % case]))
    assert {k: r["steps"].get(k, 0) for k in steps} == steps
    print("%s %s mirror vs fixture: %s" % (attn, case, "; ".join(report)))


def _ratios(attn, case, fault):
    """{checked quantity: how far the fault moves it, in units of its GPU bound}."""
    fx, base, bad = SF.fixture(attn), _mirror(attn, case), _mirror(attn, case, fault)
    m = SF.meta(attn)
    out = {}
    for k in SF.LOSS_KEYS:
        want = float(fx["%s/loss/%s" % (case, k)])
        out["loss/" + k] = abs(bad["losses"][k] - base["losses"][k]) / (SF.LOSS_TOL * max(1.0, abs(want)))
    for ph in ("gen", "disc"):
        _, _, e32 = SF.reference(attn, case, ph)
        bounds, _ = SF.grad_bounds(e32, case)
        for k, b in bounds.items():
            if k in bad[ph + "_grads"] and k in base[ph + "_grads"]:
                out["grad/%s/%s" % (ph, k)] = SF.rel(bad[ph + "_grads"][k].numpy(), base[ph + "_grads"][k].numpy()) / b
        out["norm/" + ph] = abs(bad[ph + "_norm"] - base[ph + "_norm"]) / base[ph + "_norm"] / SF.norm_bound(fx, case, ph)
    # the frozen discriminator after the generator step: bit-identical on the GPU; here, its move against the post-step allowance of an element
    # whose gradient is pinned (1e-3 x lr)
    out["frozen/discriminator"] = max(float((bad["gen_state"][k] - base["gen_state"][k]).abs().max()) for k in base["gen_state"] if k.startswith("discriminator.")) \
        / (SF.MOVE_TOL * m["lr"])
    for k, v in base["disc_state"].items():
        if k.endswith(("running_mean", "running_var")) and k.startswith("text_m."):
            out["buffer/" + k] = float((bad["disc_state"][k] - v).abs().max()) / SF.buffer_bound(k, v.numpy(), case, "disc")
    return out


@pytest.mark.parametrize("fault", SM.FAULTS)
def test_planted_faults_move_a_checked_quantity_far_beyond_its_gpu_bound(fault):
    attn, case = "lsa", "a_eps"                                                                  # the conditioned case carries the weight of the check
    ratios = _ratios(attn, case, fault)
    top = sorted(ratios, key=ratios.get)[-3:]
    print("%s: %s" % (fault, ", ".join("%s x%.3g" % (k, ratios[k]) for k in reversed(top))))
    assert ratios[top[-1]] >= FAULT_FACTOR, (fault, top[-1], ratios[top[-1]])
    if fault == "frozen_disc_live":
        bad = _mirror(attn, case, fault)
        assert all(bad["steps"][k] == 2 for k in bad["steps"] if k.startswith("discriminator.") and "reduce_c_W" not in k), "stepped in both phases"


def test_share_of_elements_the_post_step_check_cannot_pin():
    """From the fixture alone: how many sampled elements the post-step check allows more than lr / 2 (their reference gradient is below what the
    gradient bound lets an element be wrong by).  DESIGN 5l records the figures; none may exceed 30 %."""
    for attn in SF.ATTNS:
        sd = SF.state_dict(attn)
        for case in SF.CASES:
            for ph in ("gen", "disc"):
                ref, gnorm, e32 = SF.reference(attn, case, ph)
                bounds, _ = SF.grad_bounds(e32, case)
                share = SF.loose_share([SF.move_slack(ref[k], gnorm[k], sd[k].numel(), b) for k, b in bounds.items()])
                print("%s %s %s: %.4f of the sampled elements are allowed more than lr / 2" % (attn, case, ph, share))
                assert share <= 0.30


# ---- initialize_model, refusals, optimizer state ---------------------------------------------------------------------------------------------------
def _config_args(name):
    cfgs = SF.configs()
    cfg = dict(cfgs["rnn_d_lsa"])                       # rnn_d, rnn_d_b16 and rnn_no_discrim leave some keys (disc_*, sched_type, ..) to defaults
    cfg.update(cfgs[name])
    cfg["load_path"] = None
    return SimpleNamespace(**cfg)


@pytest.fixture()
def cpu_device():
    from unast_amd import train
    saved = train.DEVICE
    train.DEVICE = torch.device("cpu")
    yield
    train.DEVICE = saved


@pytest.mark.parametrize("name", ["rnn_d", "rnn_d_b16", "rnn_d_lsa", "rnn_d_luong", "rnn_d_test", "rnn_lsa", "rnn_luong", "rnn_no_discrim"])
def test_initialize_model_for_every_hidden_256_config(name, cpu_device):
    from unast_amd import train, train_rnn_step
    from unast_amd.network import TextRNN, SpeechRNN, UNAST
    args = _config_args(name)
    s_epoch, best, model, opt, sched = train.initialize_model(args)
    assert (s_epoch, best) == (0, 300) and isinstance(model, UNAST) and isinstance(model.text_m, TextRNN) and isinstance(model.speech_m, SpeechRNN)
    m = SF.meta(args.d_attn)
    want = {k: tuple(s) for k, s in zip(m["keys"], m["shapes"])}
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    if not args.use_discriminator:
        want = {k: s for k, s in want.items() if not k.startswith("discriminator.")}
        assert model.discriminator is None
    else:
        assert model.discriminator.rnn.rnn.input_size == 2 * args.hidden == 512
        if args.disc_hid != m["disc_hid"]:
            assert model.discriminator.rnn.rnn.hidden_size == args.disc_hid == 128
            got = {k: s for k, s in got.items() if not k.startswith("discriminator.")} | {k: want[k] for k in got if k.startswith("discriminator.")}
    assert list(got) == [k for k in m["keys"] if k in want] and got == want
    assert isinstance(opt, train_rnn_step.RNNFlatAdamW) and opt.decoupled == (args.optim_type == "adamw")
    assert opt.param_groups[0]["lr"] == args.lr and opt.param_groups[0]["weight_decay"] == args.weight_decay
    assert isinstance(sched, torch.optim.lr_scheduler.MultiStepLR)
    assert [s.name for s in opt.segments] == ["text_m", "speech_m"] + (["disc"] if args.use_discriminator else [])


def test_the_small_config_still_raises(cpu_device):
    from unast_amd import train
    with pytest.raises(NotImplementedError, match="hidden"):
        train.initialize_model(_config_args("rnn_small_no_discrim"))


def test_unknown_model_type_unstated_configuration_and_the_joint_steps_out_buffer_are_refused(cpu_device):
    from unast_amd import train
    with pytest.raises(NotImplementedError, match="'transformer' or 'rnn'"):
        train.initialize_model(SimpleNamespace(model_type="gru"))
    with pytest.raises(NotImplementedError, match="args does not set hidden"):
        train.initialize_model(SimpleNamespace(model_type="rnn"))
    wide = lambda T: torch.zeros(2, T, 512)                                                      # noqa: E731
    with pytest.raises(NotImplementedError, match="out="):
        train.discriminator_shuffle_batch(wide(3), torch.tensor([3, 3]), wide(4), torch.tensor([4, 4]), "rnn", out=torch.zeros(4, 4, 512))
    with pytest.raises(NotImplementedError, match="512 wide"):
        train.discriminator_shuffle_batch(torch.zeros(2, 3, 256), torch.tensor([3, 3]), torch.zeros(2, 4, 256), torch.tensor([4, 4]), "rnn")


def test_what_stays_refused_says_why(cpu_device):
    from unast_amd import train
    args = _config_args("rnn_d_lsa")
    assert args.cm_steps > 0
    with pytest.raises(NotImplementedError, match="generate in train mode"):
        train.train(args)                                   # before any model is built or kernel launched
    batch = ((None,) * 4, (None,) * 3)
    for fn in (train.crossmodel_step, ):
        with pytest.raises(NotImplementedError, match="generate in train mode"):
            fn(None, batch, args)
    with pytest.raises(NotImplementedError, match="generate in train mode"):
        train.train_cm_step({}, None, None, 0, 1, args)
    with pytest.raises(NotImplementedError, match="train_ae_step"):
        train.autoencoder_step(None, batch, args)
    with pytest.raises(NotImplementedError, match="train_sp_step"):
        train.supervised_step(None, batch, args)
    args.cm_steps = 0
    args.use_hip_graphs = True
    with pytest.raises(NotImplementedError, match="graph capture"):
        train.train(args)


def test_optimizer_state_dict_round_trips_through_torch_adamw(cpu_device):
    from unast_amd import train
    args = _config_args("rnn_d_lsa")
    _, _, model, opt, _ = train.initialize_model(args)
    assert opt.state_dict()["state"] == {}
    ref = torch.optim.AdamW(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    ref.load_state_dict(opt.state_dict())                                                        # the empty state, torch's format
    gen = torch.Generator().manual_seed(3)
    for k, p in model.named_parameters():
        p.grad = None if k.startswith("discriminator.") else torch.randn(p.shape, generator=gen) * 1e-3     # the generator phase: D has no gradients
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    ref.step()
    for k, p in model.named_parameters():
        p.data.copy_(before[k])
    sd = ref.state_dict()
    n_gen = sum(1 for k, _ in model.named_parameters() if not k.startswith("discriminator."))
    assert len(sd["state"]) == n_gen
    opt.load_state_dict(sd)
    assert [s.step for s in opt.segments] == [1, 1, 0]
    back = opt.state_dict()
    assert sorted(back["state"]) == sorted(sd["state"])
    for i, ent in sd["state"].items():
        assert float(back["state"][i]["step"]) == float(ent["step"]) == 1.0
        assert torch.equal(back["state"][i]["exp_avg"], ent["exp_avg"]) and torch.equal(back["state"][i]["exp_avg_sq"], ent["exp_avg_sq"])
    assert back["param_groups"][0]["params"] == sd["param_groups"][0]["params"]
    again = torch.optim.AdamW(model.parameters(), lr=1.0)
    again.load_state_dict(back)
    assert again.param_groups[0]["lr"] == args.lr and len(again.state) == n_gen
