"""Child program of tests/test_gpu_rnn_ddp.py: one rank of a data-parallel run of the RNN family on cuda:0 (two ranks share the one GPU over gloo,
or over the test communicator tests/native/fake_rccl.cpp; one rank runs real RCCL under UNAST_DDP_FORCE=1).  Shapes and weights:
tests/rnn_step_fixture.py -- rank 0 gets batch(attn, 'a') (B = 3, T_text = 7, T_mel = 12), rank 1 batch(attn, 'b') (B = 2, 9, 6), so the ranks
differ in batch size, lengths and launch counts; generation is cut at 7 tokens / 12 frames.  Everything runs under
set_deterministic(True, fixed_sums=True).  The worker asserts nothing about the results: it writes what it found (flags, digests, losses) to
<out>.<rank> and the test decides.

Modes
  gen    without a process group: the generator sub-steps AE, CM, SP (accum_steps = 3) on each of the two batches from fresh weights, the two
         segments' flat gradients read back; their fp32 average put into a fresh optimizer's gradient buffers and stepped (the expectation).
         Then the process group is initialised and the same sub-steps run on the rank's own batch, followed by optimizer_step.  After that
         sync_buffers and one eval encode on a common input.
  disc   the same construction with train_discriminator_step, then one frozen-discriminator forward on a common input.
  step   one train_step with ae = cm = sp = d = 1, with (--dist 1) or without a process group.
  loop   three train_step iterations under a process group; digests after each."""
import argparse
import hashlib
import os
import sys
from collections import defaultdict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import rnn_step_fixture as SF  # noqa: E402
from unast_amd import ddp, train, utils  # noqa: E402
from unast_amd import train_rnn_step as RS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("gen", "disc", "step", "loop"), required=True)
ap.add_argument("--attn", choices=SF.ATTNS, default="luong")
ap.add_argument("--drops", choices=("0", "config"), default="0")
ap.add_argument("--backend", default="gloo")
ap.add_argument("--dist", type=int, default=1)
ap.add_argument("--seed", type=int, default=11)
ap.add_argument("--out", required=True)
a = ap.parse_args()
rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
DEV = torch.device("cuda:0")
torch.cuda.set_device(DEV)
train.DEVICE = DEV
RS.TEXT_MAX_LEN, RS.SPEECH_MAX_LEN = 7, 12
utils.set_deterministic(True, fixed_sums=True)
CASE = ("a", "b")
GEN = RS.GEN_SEGMENTS
res = dict(rank=rank, mode=a.mode)


def build():
    args = SF.args_of(a.attn, 0.0 if a.drops == "0" else None, cm_steps=1)
    _, _, model, opt, _ = train.initialize_model(args)
    model.load_state_dict(SF.state_dict(a.attn))
    return model.train(), opt, args, {s.name: s for s in opt.segments}


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def state_of(segs, names):
    """Parameters, both moment buffers and the step count of the named segments (clones)."""
    return {n: (segs[n].flat.clone(), segs[n].m.clone(), segs[n].v.clone(), segs[n].step) for n in names}


def same_state(x, y):
    return {n: [bool(torch.equal(p, q)) for p, q in zip(x[n][:3], y[n][:3])] + [x[n][3] == y[n][3]] for n in x}


def state_digest(segs, names=GEN + ("disc",)):
    return {n: (digest(segs[n].flat), digest(segs[n].m), digest(segs[n].v), segs[n].step) for n in names}


def buffers(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items() if k.endswith(SF.BUFFERS) and k.startswith(("text_m.", "speech_m."))}


def gen_substeps(model, args, batch):
    utils.set_seed(a.seed)
    losses = defaultdict(list)
    train.freeze_model_parameters(model.discriminator)
    RS.train_ae_step(losses, model, batch, 0, 3, args)
    RS.train_cm_step(losses, model, batch, 0, 3, args)
    RS.train_sp_step(losses, model, batch, 0, 3, args)
    return losses


def disc_substep(model, args, batch):
    utils.set_seed(a.seed)
    losses = defaultdict(list)
    train.unfreeze_model_parameters(model.discriminator)
    RS.train_discriminator_step(losses, model, batch, 0, 1, args)
    return losses


def init_group():
    import torch.distributed as dist
    dist.init_process_group(a.backend, rank=rank, world_size=world)
    res["active"] = ddp.active()
    return dist


def finish(dist=None):
    torch.cuda.synchronize()
    res["native_handle"], res["native_issued"] = bool(ddp._Native.handle), ddp._Native.issued
    res["log"] = [l[0] for l in ddp._State.log]
    res["left_behind"] = (len(ddp._State.issued), len(ddp._State.pending))
    torch.save(res, "%s.%d" % (a.out, rank))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    print("rank", rank, "ok")


def flat_grads(opt, segs, names):
    for n in names:
        if n != "disc":
            opt._adopt_grads(segs[n])
    return {n: segs[n].grad.clone() for n in names}


def phase(names, substep, touch):
    """The three parts the gen and disc modes share.  Returns (model, opt, args, segs, dist) of the data-parallel run."""
    others = tuple(n for n in GEN + ("disc",) if n not in names)
    # -- without a process group: each batch's gradients from fresh weights
    assert not ddp.active()
    g = {}
    for c in CASE:
        model, opt, args, segs = build()
        substep(model, args, SF.batch(a.attn, c))
        g[c] = flat_grads(opt, segs, names)
    if a.mode == "gen":                                     # sync_buffers without a process group changes nothing
        before = buffers(model)
        res["sync_without_group"] = (RS.sync_buffers(model), all(torch.equal(v, before[k]) for k, v in buffers(model).items()))
    # -- the expectation: one optimizer step on the fp32 average of the two
    model_e, opt_e, args, segs_e = build()
    for n in names:
        segs_e[n].grad.copy_((g["a"][n] + g["b"][n]) * 0.5)
    touch(model_e)
    RS.optimizer_step(model_e, opt_e, args)
    want = state_of(segs_e, names)
    res["expected_stepped"] = list(opt_e.last_stepped)
    # -- the data-parallel run on the rank's own batch
    dist = init_group()
    model, opt, args, segs = build()
    start = state_of(segs, GEN + ("disc",))
    res["losses"] = {k: [float(x) for x in v] for k, v in substep(model, args, SF.batch(a.attn, CASE[rank % 2])).items()}
    own = flat_grads(opt, segs, names)
    res["own_grads_reproduced"] = {n: bool(torch.equal(own[n], g[CASE[rank % 2]][n])) for n in names}
    res["ranks_grads_differ"] = {n: not torch.equal(g["a"][n], g["b"][n]) for n in names}
    RS.optimizer_step(model, opt, args)
    torch.cuda.synchronize()
    res["stepped"] = list(opt.last_stepped)
    got = state_of(segs, names)
    res["equals_expected"] = same_state(got, want)
    res["max_abs_diff"] = {n: float((got[n][0] - want[n][0]).abs().max()) for n in names}
    res["moved"] = {n: not torch.equal(got[n][0], start[n][0]) for n in names}
    res["others_unchanged"] = same_state(state_of(segs, others), {n: start[n] for n in others})
    res["grads_left"] = {n: float(segs[n].grad.abs().max()) for n in names}
    res["state"] = state_digest(segs)
    res["buffers"] = {k: digest(v) for k, v in buffers(model).items()}
    return model, model_e, args, segs, dist


def mode_gen():
    model, model_e, args, segs, dist = phase(GEN, gen_substeps, lambda m: RS._touched(m).update(GEN))
    res["disc_params_unchanged"] = all(torch.equal(p, q) for p, q in zip(model.discriminator.parameters(), model_e.discriminator.parameters()))
    # sync_buffers: every buffer becomes rank 0's; an eval encode on one common input then agrees across the ranks
    res["synced"] = RS.sync_buffers(model)
    res["buffers_synced"] = {k: digest(v) for k, v in buffers(model).items()}
    text, _, text_len, _ = SF.batch(a.attn, "a")
    model.eval()
    with torch.no_grad():
        out = model.text_m.encode(text.to(DEV), text_len)
    flat = []

    def walk(o):
        if torch.is_tensor(o):
            flat.append(o.float())
        elif isinstance(o, (tuple, list)):
            for x in o:
                walk(x)
    walk(out)
    res["encode"] = (len(flat), digest(*flat), bool(all(torch.isfinite(t).all() for t in flat)))
    finish(dist)


def _disc_forward(model):
    g = torch.Generator().manual_seed(5)
    d_hid = (torch.randn(4, 9, RS.ENC_WIDTH, generator=g) * 0.5).to(DEV)
    d_len = torch.tensor([9, 7, 4, 2], dtype=torch.int32, device=DEV)
    for b, n in enumerate(d_len.tolist()):
        d_hid[b, n:] = 0.0
    train.freeze_model_parameters(model.discriminator)
    utils.set_seed(99)                                      # the discriminator's own dropout: the same masks on every rank
    with torch.no_grad():
        return model.discriminator(d_hid, d_len).detach().clone()


def mode_disc():
    model, model_e, args, segs, dist = phase(("disc",), disc_substep, lambda m: m._store().touched.add("disc"))
    # the store's W^T copies and tiled planes are what the frozen discriminator's forward reads
    fresh = _disc_forward(build()[0])
    out, out_e = _disc_forward(model), _disc_forward(model_e)
    res["forward"] = digest(out)
    res["forward_equals_expected"] = bool(torch.equal(out, out_e))
    res["forward_moved"] = not torch.equal(out, fresh)
    res["forward_finite"] = bool(torch.isfinite(out).all())
    finish(dist)


def _train_steps(n):
    dist = init_group() if a.dist else None
    model, opt, args, segs = build()
    utils.set_seed(a.seed)
    batch = SF.batch(a.attn, CASE[rank % 2])
    losses = defaultdict(list)
    res["iterations"] = []
    for it in range(n):
        RS.train_step(losses, model, opt, None, dict(unsup=[batch], cm=[batch], sup=[batch], disc=[batch]), it, args)
        torch.cuda.synchronize()
        res["iterations"].append(dict(state=state_digest(segs), stepped=list(opt.last_stepped)))
    res["losses"] = {k: [float(x) for x in v] for k, v in losses.items()}
    res["buffers"] = {k: digest(v) for k, v in buffers(model).items()}
    finish(dist)


{"gen": mode_gen, "disc": mode_disc, "step": lambda: _train_steps(1), "loop": lambda: _train_steps(3)}[a.mode]()
