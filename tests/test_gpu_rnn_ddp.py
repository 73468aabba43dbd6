"""Data-parallel training of the RNN family (unast_amd.train_rnn_step under torch.distributed) on ONE GPU: two child processes
(tests/rnn_ddp_worker.py) share cuda:0 and exchange the optimizer's flat gradient segments over gloo or over the test communicator
(tests/native/fake_rccl.cpp behind the C ABI); one forced rank runs real RCCL.  Rank 0 trains on the step fixture's batch a (B = 3, T_text = 7,
T_mel = 12), rank 1 on batch b (B = 2, 9, 6); generation is cut at 7 tokens / 12 frames.

The bound is bit equality throughout.  With two ranks the fp32 sum of two addends rounds once in either order and the factor 0.5 is exact, so the
exchanged gradient is (g0 + g1) * 0.5 computed in fp32; under set_deterministic(True, fixed_sums=True) a rank's own gradients reproduce to the
bit (tests/test_gpu_rnn_step.py, tests/test_gpu_rnn_cm.py pin that), and the clip norm is an fp64 sum rounded to fp32 before use.  A worker
run is made once per (mode, attention, dropout, transport) and shared by the tests that read it."""
import functools
import os
import subprocess
import sys
import tempfile
import time

import pytest

from tests import rnn_step_fixture as SF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "rnn_ddp_worker.py")
SHIM = os.path.join(ROOT, "tests", "native", "libfake_rccl.so")
GEN = ["text_m", "speech_m"]
LIMIT = 180.0                                               # seconds per run; the children of one run share it
_PORT = [29620]
_TMP = []
_ABNORMAL = []                                              # set by a run that hung, aborted or died of a signal: no later run is started


def _need_shim():
    if not os.path.exists(SHIM):
        subprocess.run(["make", "-C", os.path.join(ROOT, "unast_amd", "csrc"), "../../tests/native/libfake_rccl.so"], check=True)


def _launch(world, worker_args, **extra):
    """Starts `world` children (at most two: with this process three hold the GPU), collects them under one deadline, and on the first
    non-zero or abnormal exit kills the other one and fails without starting anything else.  Returns what each rank saved."""
    import torch
    if _ABNORMAL:
        pytest.fail("not started: an earlier run of this module ended abnormally (%s)" % _ABNORMAL[0], pytrace=False)
    if not _TMP:
        _TMP.append(tempfile.TemporaryDirectory(prefix="rnn_ddp_"))
    _PORT[0] += 2
    out = os.path.join(_TMP[0].name, "run%d" % _PORT[0])
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_PORT[0]), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0", **extra)
    cmd = [sys.executable, WORKER, "--out", out] + list(worker_args)
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    outs, deadline, failed = [None] * world, time.monotonic() + LIMIT, None
    while failed is None and any(o is None for o in outs):
        for r, p in enumerate(procs):
            if outs[r] is not None:
                continue
            left = deadline - time.monotonic()
            if left <= 0:
                failed = "rank %d did not finish within %d s" % (r, LIMIT)
                _ABNORMAL.append(failed)
                break
            try:
                outs[r] = p.communicate(timeout=min(0.5, left))[0].decode()
            except subprocess.TimeoutExpired:
                continue
            if p.returncode != 0:
                failed = "rank %d exited with %s" % (r, p.returncode)
                if p.returncode != 1:                      # a signal or an abort, not a Python exception
                    _ABNORMAL.append(failed)
                break
    if failed is not None:
        for r, p in enumerate(procs):
            if p.poll() is None:
                p.kill()
            if outs[r] is None:
                outs[r] = p.communicate(timeout=30)[0].decode()
        pytest.fail("%s\n%s" % (failed, "\n".join("---- rank %d ----\n%s" % (r, o[-4000:]) for r, o in enumerate(outs))), pytrace=False)
    assert all("rank %d ok" % r in outs[r] for r in range(world)), outs
    return [torch.load("%s.%d" % (out, r)) for r in range(world)]


@functools.lru_cache(maxsize=None)
def _run(mode, attn="luong", drops="0", transport="gloo", dist=1, repeat=0):
    """transport: 'gloo' (two ranks, torch.distributed's all_reduce), 'shim' (two ranks, unast_allreduce over the test communicator) or 'rccl'
    (one forced rank over the nccl backend: the native communicator on real RCCL).  `repeat` only tells two runs of one setting apart."""
    args = ["--mode", mode, "--attn", attn, "--drops", drops, "--dist", str(dist)]
    if transport == "rccl":
        if not dist:
            return _launch(1, args)
        return _launch(1, args + ["--backend", "nccl"], UNAST_DDP_FORCE="1")
    if transport == "shim":
        _need_shim()
        return _launch(2, args, UNAST_COMM_LIB=SHIM)
    return _launch(2, args)


def _all(flags):
    return all(all(v) for v in flags.values())


def _check_phase(runs, names, others):
    """What the generator-phase and the D-phase tests share: every rank's stepped segments equal the step on the averaged gradient to the bit,
    the other segments are bit-unchanged, and the ranks agree with each other."""
    assert len(runs) == 2
    for r in runs:
        print("rank %d: losses %s; max |p - p_expected| %s; log %s" % (r["rank"], r["losses"], r["max_abs_diff"], r["log"]))
        assert r["active"] and r["expected_stepped"] == names
        assert all(r["own_grads_reproduced"].values()), ("a rank's own gradients did not reproduce to the bit", r["own_grads_reproduced"])
        assert all(r["ranks_grads_differ"].values()), "the two batches must give different gradients"
        assert r["stepped"] == names
        assert _all(r["equals_expected"]), ("parameters / exp_avg / exp_avg_sq / step against the averaged-gradient step", r["equals_expected"], r["max_abs_diff"])
        assert all(r["moved"].values()) and all(r["state"][n][3] == 1 for n in names)
        assert sorted(r["others_unchanged"]) == sorted(others) and _all(r["others_unchanged"]), r["others_unchanged"]
        assert all(r["state"][n][3] == 0 for n in others)
        assert all(v == 0.0 for v in r["grads_left"].values()), "optimizer_step leaves the gradients zero"
        assert r["log"] == names and r["left_behind"] == (0, 0)
    assert runs[0]["state"] == runs[1]["state"], "the ranks' parameters and optimizer state diverged"
    assert runs[0]["losses"] != runs[1]["losses"], "the ranks should have seen different batches"


# ---- 1. the generator phase equals the step on the averaged gradient, to the bit ------------------------------------------------------------------
@pytest.mark.parametrize("drops", ["0", "config"])
@pytest.mark.parametrize("attn", SF.ATTNS)
def test_generator_phase_equals_the_step_on_the_averaged_gradient(attn, drops):
    """AE, CM and SP sub-steps (accum_steps = 3) on each rank's own batch, then optimizer_step: parameters, both moments and step counts of
    text_m and speech_m equal one step on (g0 + g1) * 0.5; the discriminator is bit-unchanged; the ranks' parameters are bit-identical; their
    BatchNorm statistics are not (they stay per rank)."""
    runs = _run("gen", attn, drops)
    _check_phase(runs, GEN, ["disc"])
    assert all(r["disc_params_unchanged"] for r in runs)
    assert all(sorted(r["losses"]) == sorted(("t_ae", "s_ae", "d_ae", "t_cm", "s_cm", "d_cm", "asr_", "tts_", "sp_d")) for r in runs)
    b0, b1 = runs[0]["buffers"], runs[1]["buffers"]
    differ = [k for k in b0 if b0[k] != b1[k]]
    print("%s drops=%s: %d of %d buffers differ between the ranks" % (attn, drops, len(differ), len(b0)))
    assert any(k.endswith("running_mean") for k in differ) and any(k.endswith("running_var") for k in differ), differ


# ---- 2. the D phase ------------------------------------------------------------------------------------------------------------------------------------
def test_discriminator_phase_equals_the_step_on_the_averaged_gradient():
    """train_discriminator_step on each rank's own batch, then optimizer_step: only disc steps, the generators' parameters, moments and step
    counts are bit-unchanged, the discriminator equals the averaged-gradient step, and the store's W^T copies and tiled planes were refreshed:
    one frozen-discriminator forward on a common input agrees to the bit between the ranks and with the expectation's model, and differs from
    the forward on the initial weights."""
    runs = _run("disc", "luong", "config")
    _check_phase(runs, ["disc"], GEN)
    assert all(sorted(r["losses"]) == ["d"] for r in runs)
    for r in runs:
        assert r["forward_finite"] and r["forward_equals_expected"] and r["forward_moved"], (r["forward_finite"], r["forward_equals_expected"], r["forward_moved"])
    assert runs[0]["forward"] == runs[1]["forward"]


# ---- 3. both transports --------------------------------------------------------------------------------------------------------------------------------
def test_generator_phase_over_torch_distributed_and_over_the_native_communicator():
    """Test 1 at dropout 0 over gloo (torch.distributed.all_reduce) and through unast_allreduce with the test communicator bound: the same
    bits, and the native run issued one collective per exchanged segment."""
    gloo, shim = _run("gen", "luong", "0"), _run("gen", "luong", "0", "shim")
    _check_phase(shim, GEN, ["disc"])
    for g, s in zip(gloo, shim):
        assert not g["native_handle"] and g["native_issued"] == 0
        assert s["native_handle"] and s["native_issued"] == 2, (s["native_handle"], s["native_issued"])
        assert g["state"] == s["state"] and g["losses"] == s["losses"] and g["buffers"] == s["buffers"]


# ---- 4. one rank, real RCCL ----------------------------------------------------------------------------------------------------------------------------
def test_one_forced_rank_over_rccl_equals_the_step_without_a_process_group():
    """A full train_step with ae = cm = sp = d = 1 at the configs' dropout over the nccl backend (UNAST_DDP_FORCE=1): the three segments travel
    through the native communicator on real RCCL, and parameters, moments, step counts, the ten losses and the buffers equal the same step of a
    process without a process group, to the bit."""
    (d,), (p,) = _run("step", "lsa", "config", "rccl"), _run("step", "lsa", "config", "rccl", dist=0)
    print("losses %s" % d["losses"])
    assert d["active"] and d["native_handle"] and d["native_issued"] == 3 and d["log"] == GEN + ["disc"], (d["native_handle"], d["native_issued"], d["log"])
    assert p["log"] == [] and p["native_issued"] == 0
    assert len(d["losses"]) == 10 and all(len(v) == 1 for v in d["losses"].values())
    assert d["losses"] == p["losses"], (d["losses"], p["losses"])
    assert d["iterations"] == p["iterations"] and d["iterations"][0]["stepped"] == ["disc"]
    assert all(d["iterations"][0]["state"][n][3] == 1 for n in GEN + ["disc"])
    assert d["buffers"] == p["buffers"]


# ---- 5. sync_buffers -----------------------------------------------------------------------------------------------------------------------------------
def test_sync_buffers_makes_every_buffer_rank_zeros_and_eval_agrees():
    """After test 1's step the ranks differ in running statistics; after sync_buffers(model) every buffer of both sides is bit-identical across
    the ranks and equal to what rank 0 had, and TextRNN.encode under eval() / no_grad on one common input agrees to the bit.  Without a process
    group the call broadcasts nothing and changes nothing."""
    r0, r1 = _run("gen", "luong", "0")
    assert r0["buffers"] != r1["buffers"]
    assert r0["synced"] == r1["synced"] >= len(r0["buffers"]) > 0
    assert r0["buffers_synced"] == r0["buffers"], "rank 0 keeps its own buffers"
    assert r1["buffers_synced"] == r0["buffers"], "rank 1 takes rank 0's"
    assert r0["encode"] == r1["encode"] and r0["encode"][0] >= 3 and r0["encode"][2], (r0["encode"], r1["encode"])
    assert r0["sync_without_group"] == (0, True) and r1["sync_without_group"] == (0, True)


# ---- 6. a loop -------------------------------------------------------------------------------------------------------------------------------------------
def test_three_iterations_stay_in_step_and_repeat_to_the_bit():
    """Three train_step iterations with ae = cm = sp = d = 1 at the configs' dropout on two ranks over gloo: finite losses on both ranks at
    every iteration, parameters and optimizer state bit-identical across the ranks after each, and two runs of the whole thing agree."""
    import math
    first, second = _run("loop", "lsa", "config"), _run("loop", "lsa", "config", repeat=1)
    for runs in (first, second):
        r0, r1 = runs
        for r in runs:
            assert len(r["losses"]) == 10 and all(len(v) == 3 and all(math.isfinite(x) for x in v) for v in r["losses"].values()), r["losses"]
            assert r["log"] == (GEN + ["disc"]) * 3 and r["left_behind"] == (0, 0)
        for it in range(3):
            assert r0["iterations"][it]["state"] == r1["iterations"][it]["state"], "the ranks diverged in iteration %d" % it
            assert all(r0["iterations"][it]["state"][n][3] == it + 1 for n in GEN + ["disc"])
        assert r0["iterations"][0]["state"] != r0["iterations"][2]["state"]
        assert r0["losses"] != r1["losses"] and r0["buffers"] != r1["buffers"]
    for a, b in zip(first, second):
        assert a["losses"] == b["losses"] and a["iterations"] == b["iterations"] and a["buffers"] == b["buffers"]
