"""The serialiser the three optimizers share (unast_amd.flat_adam.FlatAdam.state_dict / load_state_dict) over segments built by hand from
small CPU tensors: an adopted segment whose parameters need padding, a segment with a tap-major parameter, a segment that never stepped.
No GPU and no kernel.
"""
import pytest
import torch

from unast_amd import flat_adam

HYPER = dict(lr=1e-3, weight_decay=0.02, betas=(0.8, 0.95), eps=1e-6)


def build(lr=HYPER["lr"], known=True):
    """(optimizer, [adopted, tap-major, never stepped]); torch's parameter order interleaves the segments.  known: the moments and step
    counts the checks expect; otherwise junk everywhere that a load has to clear."""
    g = torch.Generator().manual_seed(5)
    p7, p12, pc = (torch.nn.Parameter(torch.randn(*s, generator=g)) for s in ((7,), (3, 4), (2, 2)))
    adopted = flat_adam.adopt("adopted", [p7, p12])
    assert adopted.offsets == [0, 8] and adopted.flat.numel() == 20                    # 7 -> 8: one element of padding
    never = flat_adam.adopt("never", [pc])
    conv = torch.nn.Parameter(torch.zeros(3, 2, 5))                                    # torch: [Cout, Cin, k]; stored [Cout, k, Cin]
    cflat, cgrad = torch.randn(30, generator=g), torch.zeros(30)
    conv.data = cflat.view(3, 5, 2).permute(0, 2, 1)
    tap = flat_adam.Segment("tap", [conv], [0], cflat, cgrad, tap_major=[True])
    segs = [adopted, tap, never]
    for i, s in enumerate(segs):
        n = s.m.numel()
        if known:
            s.m.copy_(torch.arange(n) * 0.5 - 3.0 + 100 * i)
            s.v.copy_(torch.arange(n) * 0.25 + 1.0 + 100 * i)
        else:
            s.m.fill_(7.0); s.v.fill_(7.0)
    if known:
        adopted.m[7] = adopted.v[7] = 0.0                                              # padding never receives a moment
        never.m.zero_(); never.v.zero_()
    adopted.step, tap.step, never.step = (3, 5, 0) if known else (8, 8, 8)
    opt = flat_adam.FlatAdam([p7, conv, p12, pc], segs, lr, HYPER["weight_decay"], HYPER["betas"], HYPER["eps"])
    return opt, segs


def expected(segs):
    """{torch index: (step, exp_avg, exp_avg_sq)} in torch's shapes, indexed out of the buffers element by element."""
    adopted, tap, _ = segs
    out = {0: (3, adopted.m[0:7].clone(), adopted.v[0:7].clone()), 2: (3, adopted.m[8:20].view(3, 4).clone(), adopted.v[8:20].view(3, 4).clone())}
    m, v = torch.empty(3, 2, 5), torch.empty(3, 2, 5)
    for co in range(3):
        for ci in range(2):
            for k in range(5):
                m[co, ci, k], v[co, ci, k] = tap.m[co * 10 + k * 2 + ci], tap.v[co * 10 + k * 2 + ci]
    out[1] = (5, m, v)
    return out


def test_state_dict_is_torch_adamw_format():
    opt, segs = build()
    want = expected(segs)
    sd = opt.state_dict()
    params = opt.param_groups[0]["params"]
    assert list(sd["state"]) == [0, 1, 2]                                              # the never-stepped segment (index 3) has no entry
    topt = torch.optim.AdamW(params, lr=0.5)
    topt.load_state_dict(sd)
    tsd = topt.state_dict()
    assert sorted(tsd["state"]) == [0, 1, 2] and tsd["param_groups"][0]["params"] == [0, 1, 2, 3]
    for key, val in HYPER.items():
        assert topt.param_groups[0][key] == val
    buffers = {t.untyped_storage().data_ptr() for s in segs for t in (s.m, s.v, s.flat, s.grad)}
    for i, (step, m, v) in want.items():
        for d in (sd, tsd):
            ent = d["state"][i]
            assert float(ent["step"]) == step
            assert ent["exp_avg"].shape == params[i].shape and ent["exp_avg_sq"].shape == params[i].shape
            assert torch.equal(ent["exp_avg"], m) and torch.equal(ent["exp_avg_sq"], v), i
        for t in (sd["state"][i]["exp_avg"], sd["state"][i]["exp_avg_sq"]):
            assert t.is_contiguous() and t.untyped_storage().data_ptr() not in buffers
    before = [s.m.clone() for s in segs]
    for ent in sd["state"].values():
        ent["exp_avg"].add_(1.0)
    assert all(torch.equal(s.m, b) for s, b in zip(segs, before))


@pytest.mark.parametrize("string_keys", [False, True])
def test_load_state_dict_restores_moments_steps_and_hyper_parameters(string_keys):
    opt, segs = build()
    opt.param_groups[0]["initial_lr"] = 0.25                                           # what a torch LR scheduler leaves behind
    sd = opt.state_dict()
    sd["param_groups"][0]["betas"] = list(sd["param_groups"][0]["betas"])              # as a checkpoint that went through JSON carries them
    if string_keys:
        sd["state"] = {str(k): v for k, v in sd["state"].items()}
    opt2, segs2 = build(lr=0.5, known=False)
    assert opt2.param_groups[0]["lr"] == 0.5
    opt2.load_state_dict(sd)
    assert [s.step for s in segs2] == [3, 5, 0]
    for s, s2 in zip(segs, segs2):
        assert torch.equal(s2.m, s.m) and torch.equal(s2.v, s.v), s.name               # junk cleared, padding and the unstepped segment zero
    g2 = opt2.param_groups[0]
    assert {k: g2[k] for k in ("lr", "weight_decay", "betas", "eps", "initial_lr")} == dict(HYPER, initial_lr=0.25)
    assert isinstance(g2["betas"], tuple)
    assert opt2.state_dict()["state"].keys() == opt.state_dict()["state"].keys()
