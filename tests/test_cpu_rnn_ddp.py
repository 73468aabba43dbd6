"""The RNN family's data-parallel exchange on the host (gloo, CPU tensors): unast_amd.ddp.finish_segments over flat_adam.Segment gradient buffers,
the local phase check of RNNFlatAdamW.step, and train_rnn_step.sync_buffers.  DESIGN 5p.  The GPU side is tests/test_gpu_rnn_ddp.py."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HEAD = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
from unast_amd import ddp, flat_adam
rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
"""

_SEGMENTS_WORKER = _HEAD + r"""
ddp._State.scale_fn = lambda buf, a: buf.mul_(a)
def own(n, r):                                            # small integers and quarters: sums and the mean are exact in fp32
    return torch.arange(n, dtype=torch.float32) * (r + 1) + 0.25 * r
segs = [flat_adam.Segment(name, [], [], torch.zeros(n), own(n, rank)) for name, n in (("text_m", 10), ("speech_m", 7), ("disc", 4))]
assert ddp.active() and ddp._State.log == []
n = ddp.finish_segments([segs[0].grad, segs[1].grad], ["text_m", "speech_m"])
assert n == 2
for s in segs[:2]:
    mean = sum(own(s.grad.numel(), r) for r in range(world)) / world
    assert torch.equal(s.grad, mean), (s.name, s.grad, mean)
assert torch.equal(segs[2].grad, own(4, rank)), "a segment that does not step must not travel"
assert ddp._State.log == [("text_m", 0, 10), ("speech_m", 0, 7)], ddp._State.log
assert ddp._State.issued == [] and ddp._State.pending == [] and not ddp._State.armed
# the D phase after it: the third buffer alone; without labels the log names the position in the list
n = ddp.finish_segments([segs[2].grad])
assert n == 1 and ddp._State.log[-1] == ("segment0", 0, 4) and torch.equal(segs[2].grad, sum(own(4, r) for r in range(world)) / world)
assert ddp._State.issued == [] and ddp._State.pending == []

# sync_buffers: every buffer of both sides becomes rank 0's (int64 counters included), cached operand packs are dropped
from types import SimpleNamespace
from unast_amd import train_rnn_step as RS
from unast_amd.rnn import PACK_SLOTS
model = SimpleNamespace(text_m=torch.nn.BatchNorm1d(3), speech_m=torch.nn.BatchNorm1d(5))
for m in (model.text_m, model.speech_m):
    m.running_mean.fill_(1.0 + rank); m.running_var.fill_(2.0 + rank); m.num_batches_tracked.fill_(7 + rank)
    m.__dict__[PACK_SLOTS[0]] = "stale"
assert RS.sync_buffers(model) == 6
for m in (model.text_m, model.speech_m):
    assert float(m.running_mean[0]) == 1.0 and float(m.running_var[-1]) == 2.0 and int(m.num_batches_tracked) == 7
    assert PACK_SLOTS[0] not in m.__dict__
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""

_PHASE_WORKER = _HEAD + r"""
from types import SimpleNamespace
from unast_amd import train_rnn_step as RS
assert world == 1 and ddp.FORCE and ddp.active()
ddp._State.scale_fn = lambda buf, a: buf.mul_(a)
# a stand-in optimizer: the three segments over tiny parameters, and a model whose sub-steps touched text_m alone
opt = RS.RNNFlatAdamW.__new__(RS.RNNFlatAdamW)
opt.segments = [flat_adam.adopt(n, [torch.nn.Parameter(torch.ones(k))]) for n, k in (("text_m", 10), ("speech_m", 7), ("disc", 4))]
opt.model, opt._store, opt.last_stepped = SimpleNamespace(_rnn_touched={"text_m"}), None, []
for s in opt.segments:
    s.grad.fill_(3.0)
try:
    opt.step(max_norm=1.0)
except RuntimeError as e:
    msg = str(e)
else:
    raise AssertionError("a step over text_m alone must be refused under a process group")
assert "(text_m)" in msg and "text_m, speech_m" in msg and "disc" in msg, msg
assert ddp._State.log == [] and ddp._State.issued == [], "refused before any collective"
assert all(float(s.grad[0]) == 3.0 and s.step == 0 for s in opt.segments), "nothing was scaled or stepped"
# generator and discriminator segments mixed in one phase are refused too
opt.model._rnn_touched = {"text_m", "speech_m"}
opt._has_grads = lambda seg: True
try:
    opt.step(max_norm=1.0)
except RuntimeError as e:
    assert "text_m, speech_m, disc" in str(e), e
else:
    raise AssertionError("all three segments in one phase must be refused")
assert ddp._State.log == []
# a phase without gradients steps nothing and exchanges nothing
opt._has_grads = lambda seg: False
opt.step(max_norm=1.0)
assert opt.last_stepped == [] and ddp._State.log == []
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def _run(tmp_path, worker, world, port, **extra):
    script = tmp_path / "w.py"
    script.write_text(worker % ROOT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), **extra)
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    outs = [p.communicate(timeout=180)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert all("rank %d ok" % r in outs[r] for r in range(world)), outs


def test_segment_buffers_are_exchanged_in_list_order_two_ranks_gloo(tmp_path):
    """finish_segments on two of three odd-sized segment buffers: the exact mean in both, the third bit-unchanged, the log in list order, no
    issued range or pending handle left behind; and sync_buffers makes the buffers of both sides rank 0's."""
    _run(tmp_path, _SEGMENTS_WORKER, 2, 29611)


def test_a_step_over_other_segments_than_a_phase_is_refused_before_any_collective(tmp_path):
    """RNNFlatAdamW.step under a (forced, one-rank) process group: a touched set of {text_m} alone, or of all three segments, raises a
    RuntimeError that names the sets, before anything is exchanged, scaled or stepped."""
    _run(tmp_path, _PHASE_WORKER, 1, 29613, UNAST_DDP_FORCE="1")


def test_sync_buffers_changes_nothing_without_a_process_group():
    import torch
    from types import SimpleNamespace
    from unast_amd import train_rnn_step as RS
    from unast_amd.rnn import PACK_SLOTS
    model = SimpleNamespace(text_m=torch.nn.BatchNorm1d(3), speech_m=torch.nn.BatchNorm1d(5))
    model.text_m.running_mean.fill_(4.0)
    model.text_m.__dict__[PACK_SLOTS[0]] = "kept"
    assert RS.sync_buffers(model) == 0
    assert float(model.text_m.running_mean[0]) == 4.0 and model.text_m.__dict__[PACK_SLOTS[0]] == "kept"
