"""The hand-off from a fused head + loss launch (decode_sequence(..., loss_hint=)) to text_loss / speech_loss: the record belongs to the
head buffer and dies with it, the match reads no device memory, and a hint the kernels could misread is ignored.  In every case the loss
call returns what it returns without a hint."""
import gc
from collections import defaultdict

import pytest
import torch

from tests.test_gpu_joint import D, build

pytestmark = pytest.mark.gpu
GS = 0.5            # the upstream gradient of each loss: _sum_and_backward(..., accum_steps=2) hands down a resident 0.5


def _setup():
    """Model, two raw batches of one shape, the same batches processed, and the encoder outputs of the first (computed once, without a
    graph: every decoder call below reads them as they are)."""
    from unast_amd import train
    from unast_amd.portable import synth_batch
    args, model, _ = build(1, 1e-3, use_discriminator=False)
    model.train()
    raw = [tuple(torch.from_numpy(x) for x in synth_batch(3, 24, 64, seed=s, ragged=True)) for s in (1, 2)]
    xy = [train.process_batch(b) for b in raw]
    text, mel, tl, ml = xy[0][0]
    with torch.no_grad():
        mem = model.text_m.encode(text, tl), model.speech_m.encode(mel, ml)
    return args, model, raw, xy, mem


def _text(model, x, mem, hint=None):
    return model.text_m.decode_sequence(x[0], x[2], *mem[0], loss_hint=hint)                 # [B, T, V], a view of the logits buffer


def _speech(model, x, mem, hint=None):
    return model.speech_m.decode_sequence(x[1], x[3], *mem[1], loss_hint=hint)[:3]           # pre, post, stop: views of the head / post buffers


def _text_loss(args, y, logits):
    from unast_amd import train
    return train.text_loss(y[0], logits.permute(0, 2, 1), args.t_eos_weight)


def _speech_loss(args, y, ml, out):
    from unast_amd import train
    pre, post, stop = out
    return train.speech_loss(y[1], y[2], pre, post, ml, stop, args.s_eos_weight)


def _another_loss(model, out):
    """A backward of some other function of a decoder call's outputs; its gradients are discarded."""
    sum(t.sum() for t in out).backward()
    model._store().zero_grad()


def _backward(model, loss):
    """(loss, parameter gradients) after the train step's backward of this one loss; leaves the gradients zero."""
    from unast_amd import train
    train._sum_and_backward([loss], 2)
    model.expose_grads()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    model._store().zero_grad()
    for p in model.parameters():
        p.grad = None
    return float(loss.detach()), grads


def _assert_same(a, b):
    """The tolerances of test_gpu_joint.test_joint_generator_step_equals_the_two_substeps."""
    (la, ga), (lb, gb) = a, b
    assert abs(la - lb) <= 2e-6 * max(1.0, abs(la)), (la, lb)
    assert set(ga) == set(gb) and ga
    tot = float(torch.sqrt(sum((g.double() ** 2).sum() for g in ga.values())))
    for n in ga:
        d = (ga[n].double() - gb[n].double()).norm().item()
        assert d <= 2e-5 * ga[n].double().norm().item() + 2e-7 * tot, (n, d, ga[n].double().norm().item())


def _records():
    return sum(1 for o in gc.get_objects() if issubclass(type(o), torch.Tensor) and "fused_loss" in vars(o))


@pytest.mark.parametrize("side", ["text", "speech"])
def test_a_dropped_record_never_reaches_a_later_buffer_at_its_address(side):
    """A hinted decoder call whose loss never comes, its outputs dropped; then an unhinted call of the same shape on other targets, whose
    head buffer the allocator places at the dropped one's address, and its loss with the same gold tensor: the loss and the gradients
    are those of a fresh unhinted run, not the dropped call's.  (The speech call's outputs go through another backward first: a call
    with several outputs that is dropped before any backward keeps its buffers, so no later buffer could take its address.)"""
    from unast_amd import functional as F, train
    args, model, _, ((x1, y1), (x2, _)), mem = _setup()
    if side == "text":
        hint = (y1[0], args.t_eos_weight, GS, train._loss_ws(D))
        run, loss = (lambda x, h=None: (_text(model, x, mem, h),)), (lambda out: _text_loss(args, y1, out[0]))
        drop = lambda out: None
    else:
        hint = (y1[1], x1[3], args.s_eos_weight, GS, train._loss_ws(D))
        run, loss = (lambda x, h=None: _speech(model, x, mem, h)), (lambda out: _speech_loss(args, y1, x1[3], out))
        drop = lambda out: _another_loss(model, out)
    ref = _backward(model, loss(run(x2)))
    for _ in range(4):          # the last call is the one whose address is compared; the first ones make every lazily made buffer
        out = run(x1, hint)
        drop(out)
        dropped = out[0].untyped_storage().data_ptr()
        del out
        gc.collect()
    before = F.FUSED_STATS[side + "_grad_direct"]
    out = run(x2)
    assert out[0].untyped_storage().data_ptr() == dropped
    _assert_same(_backward(model, loss(out)), ref)
    assert F.FUSED_STATS[side + "_grad_direct"] == before


@pytest.mark.parametrize("case", ["text_int32_gold", "speech_int64_lengths"])
def test_a_hint_the_kernels_could_misread_takes_the_general_path(case):
    """int32 gold ids in a text hint are ignored: the head runs unfused.  int64 lengths in a speech hint are converted (utils.lens_i32),
    so the head launch reads the right lengths, and speech_loss, whose own converted lengths are another tensor, computes the loss with
    the general kernels.  Loss and gradients equal the unhinted call's either way."""
    from unast_amd import functional as F, train
    args, model, _, ((x, y), _), mem = _setup()
    if case == "text_int32_gold":
        hinted = lambda: _text_loss(args, y, _text(model, x, mem, (y[0].int(), args.t_eos_weight, GS, train._loss_ws(D))))
        plain = lambda: _text_loss(args, y, _text(model, x, mem))
        expect = {"text_head": 0}
    else:
        lens64 = x[3].long()
        hinted = lambda: _speech_loss(args, y, lens64, _speech(model, x, mem, (y[1], lens64, args.s_eos_weight, GS, train._loss_ws(D))))
        plain = lambda: _speech_loss(args, y, x[3], _speech(model, x, mem))
        expect = {"speech_head": 1, "speech_grad_direct": 0}
    before = dict(F.FUSED_STATS)
    got = _backward(model, hinted())
    used = {k: F.FUSED_STATS[k] - before[k] for k in expect}
    _assert_same(got, _backward(model, plain()))
    assert used == expect


def test_no_record_outlives_its_step_or_its_dropped_outputs():
    """train_gen_joint_step consumes every record it makes; a hinted call whose loss never comes leaves nothing allocated once its
    outputs are dropped (the speech call's after another backward, see test_a_dropped_record_never_reaches_a_later_buffer_at_its_address)."""
    from unast_amd import train
    args, model, (ae, sp), ((x, y), _), mem = _setup()
    n = _records()
    train.train_gen_joint_step(defaultdict(list), model, ae, sp, 0, 2, args)
    torch.cuda.synchronize()
    gc.collect()
    assert _records() == n
    model._store().zero_grad()

    th, sh = (y[0], args.t_eos_weight, GS, train._loss_ws(D)), (y[1], x[3], args.s_eos_weight, GS, train._loss_ws(D))
    for hinted in (False, True):        # (the unhinted round makes every lazily made buffer before the baseline)
        _text(model, x, mem, th if hinted else None)
        _another_loss(model, _speech(model, x, mem, sh if hinted else None))
        gc.collect()
        if not hinted:
            base = torch.cuda.memory_allocated(D)
    assert _records() == n
    assert torch.cuda.memory_allocated(D) <= base


def test_the_match_reads_no_device_memory(monkeypatch):
    """A loss call whose gold is an equal-valued copy of the announced one does not match (addresses only, no torch.equal) and completes
    on the general kernels with the unhinted result."""
    from unast_amd import functional as F, train
    args, model, _, ((x, y), _), mem = _setup()
    ref_t = _backward(model, _text_loss(args, y, _text(model, x, mem)))
    ref_s = _backward(model, _speech_loss(args, y, x[3], _speech(model, x, mem)))
    logits = _text(model, x, mem, (y[0], args.t_eos_weight, GS, train._loss_ws(D)))
    out = _speech(model, x, mem, (y[1], x[3], args.s_eos_weight, GS, train._loss_ws(D)))

    def no_host_read(*a, **k):
        raise AssertionError("torch.equal in the fused-loss match")
    monkeypatch.setattr(torch, "equal", no_host_read)
    before = dict(F.FUSED_STATS)
    copy = (y[0].clone(), y[1].clone(), y[2])
    got_t = _backward(model, _text_loss(args, copy, logits))
    got_s = _backward(model, _speech_loss(args, copy, x[3], out))
    assert all(F.FUSED_STATS[k] == before[k] for k in before), (before, F.FUSED_STATS)
    monkeypatch.undo()
    _assert_same(got_t, ref_t)
    _assert_same(got_s, ref_s)
