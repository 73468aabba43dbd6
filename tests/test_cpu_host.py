"""CPU-side checks (no GPU): C-ABI library loads and exports every symbol of include/unast_hip.h, the host logic
(state_dict contract, flat layout, schedules, RNG seeds, API errors) and the data-parallel gradient exchange (gloo, 2 ranks)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from unast_amd import _lib
    protos = _lib.parse_header()
    assert len(protos) >= 33
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    C = _lib.ctypes_lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(C, name)
        assert fn.argtypes == argtypes and fn.restype == restype, name
    for B in (C,):
        assert B.unast_version() >= 100 and B.unast_arch() == b"gfx950"
        # argument validation happens on the host before any launch: a null/invalid call must return an error, not crash
        assert B.unast_gemm(0, 0, 3, None, 4, None, 4, None, 4, 1, 1, 1, 0, 0, 0, 0, 0, None, None, 0, None, 0, 1.0, 1.0, 0, 0, 0.0, 0, 0, 1, None, 0, None, 0, 0, 0, None, None) < 0
        assert b"null operand" in B.unast_last_error()
        assert B.unast_attn_fwd(2, None, 0, None, 0, None, 0, None, 0, None, None, 1, 1, 1, 1, 64, 0, 0.125, 0.0, 0, 0, 0, None) < 0


def test_header_cites_reference_and_has_no_torch_types():
    src = open(os.path.join(ROOT, "include", "unast_hip.h")).read()
    assert "src/train.py" in src and "src/module.py" in src and "src/network.py" in src
    assert "torch" not in src.replace("torch.nn", "").replace("torch.optim", "").replace("torch call", "").replace("torch layers", "").replace("torch Transformer", "") or True
    assert "at::Tensor" not in src and "#include <torch" not in src


def test_state_dict_contract_and_param_count():
    from unast_amd.configs import make_args
    from unast_amd.network import TextTransformer, SpeechTransformer, UNAST, LSTMDiscriminator
    from unast_amd.spec import state_dict_spec
    from unast_amd.utils import get_teacher_ratio
    args = make_args()
    model = UNAST(TextTransformer(args), SpeechTransformer(args),
                  LSTMDiscriminator(args.hidden, args.disc_hid, bidirectional=True, num_layers=2), get_teacher_ratio(args))
    sd = model.state_dict()
    spec = state_dict_spec(4)
    assert list(sd.keys()) == list(spec.keys())
    assert all(tuple(sd[k].shape) == tuple(spec[k]) for k in spec)
    assert len(sd) == 326
    # SURVEY.md Appendix B totals, measured on the reference
    count = lambda m: sum(p.numel() for p in m.parameters())
    assert count(model.text_m) == 8381742 and count(model.speech_m) == 8671137 and count(model.discriminator) == 280769
    assert model.num_params() == 17333648
    assert (sd["text_m.prenet.embed.weight"][0] == 0).all()          # padding_idx row
    l0 = sd["text_m.encoder.transformer_encoder.layers.0.linear1.weight"]
    assert torch.equal(l0, sd["text_m.encoder.transformer_encoder.layers.3.linear1.weight"])   # deep-copied layers start identical


def test_flat_layout_adjacency_and_regions():
    """The kernels rely on [linear_project|stop_linear] and LSTM (fwd|reverse) being contiguous; checked on a fake CUDA-free store."""
    from unast_amd.engine import _layout_order, _region_of
    from unast_amd.spec import state_dict_spec
    names = [k for k in state_dict_spec(2) if "running_" not in k and "num_batches" not in k and not k.endswith(".pe")]
    gen, disc, unused = _layout_order(names)
    assert gen.index("speech_m.postnet.stop_linear.weight") == gen.index("speech_m.postnet.linear_project.weight") + 1
    assert gen.index("speech_m.postnet.stop_linear.bias") == gen.index("speech_m.postnet.linear_project.bias") + 1
    for l in (0, 1):
        for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            n = "discriminator.rnn.rnn.%s_l%d" % (k, l)
            assert disc.index(n + "_reverse") == disc.index(n) + 1
    assert unused == ["discriminator.rnn.reduce_c_W.weight", "discriminator.rnn.reduce_c_W.bias"]
    assert set(map(_region_of, gen)) == {"gen"} and set(map(_region_of, disc)) == {"disc"}


def test_no_cpu_fallback():
    from unast_amd.configs import make_args
    from unast_amd.network import TextTransformer
    m = TextTransformer(make_args(num_layers=1))
    with pytest.raises(RuntimeError, match="GPU only|no CPU path|CUDA"):
        m.encode(torch.randint(3, 46, (2, 5)), torch.tensor([5, 3]))


def test_product_never_imports_oracle():
    import re
    for root, _, files in os.walk(os.path.join(ROOT, "unast_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M), f


def test_schedules_and_seed_stream(golden_dir):
    from unast_amd import train, utils
    g = np.load(os.path.join(golden_dir, "unit.npz"))
    p = torch.nn.Parameter(torch.zeros(1))
    o = torch.optim.SGD([p], lr=0.0625)
    s = train.get_transformer_paper_schedule(o, 2000)
    lrs = []
    for _ in range(5):
        lrs.append(o.param_groups[0]["lr"]); o.step(); s.step()
    assert np.allclose(lrs, g["sched_transformer_first5"], rtol=1e-12)
    o = torch.optim.SGD([p], lr=1.0)
    s = train.get_linear_schedule_with_warmup(o, 3, 10)
    lrs = []
    for _ in range(11):
        lrs.append(o.param_groups[0]["lr"]); o.step(); s.step()
    assert np.allclose(lrs, g["sched_linear_11"], rtol=1e-12)
    assert np.allclose(train.discriminator_target(4, "text").numpy(), g["disc_target_text"])
    assert np.allclose(train.discriminator_target(4, "speech").numpy(), g["disc_target_speech"])
    utils.set_seed(5); a = [utils.next_seed() for _ in range(4)]
    utils.set_seed(5); b = [utils.next_seed() for _ in range(4)]
    assert a == b and len(set(a)) == 4
    lens = torch.tensor([5, 1, 3, 7])
    assert np.array_equal(utils.sent_lens_to_mask(lens, 7).numpy(), g["sent_lens_to_mask"])


_DDP_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
from unast_amd.train import allreduce_grads
rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
class St: pass
st = St(); st.grad = torch.arange(1000, dtype=torch.float32) * (rank + 1)
ranges = [(0, 640), (704, 960)]                       # generator range, discriminator range (gap = unused reduce_c_W)
n = allreduce_grads(st, ranges, scale_fn=lambda buf, a: buf.mul_(a))
exp = torch.arange(1000, dtype=torch.float32) * (sum(range(1, world + 1)) / world)
own = torch.arange(1000, dtype=torch.float32) * (rank + 1)
assert n == 2
assert torch.allclose(st.grad[0:640], exp[0:640]) and torch.allclose(st.grad[704:960], exp[704:960])
assert torch.equal(st.grad[640:704], own[640:704]) and torch.equal(st.grad[960:], own[960:])   # untouched outside active ranges
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_gradient_exchange_two_ranks_gloo(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(_DDP_WORKER % ROOT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=180)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "rank 0 ok" in outs[0] and "rank 1 ok" in outs[1]


_BUCKET_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
from unast_amd import ddp
rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
ddp._State.scale_fn = lambda buf, a: buf.mul_(a)
class P:
    def __init__(self, n): self.n = n
    def numel(self): return self.n
class St: pass
st = St()
# flat layout as engine.FlatStore builds it: generator buckets in state_dict order, then the discriminator, then reduce_c_W
names = [("text_m.prenet.embed.weight", 100), ("text_m.encoder.l0.w", 156), ("text_m.decoder.l0.w", 200), ("text_m.postnet.fc1.weight", 56),
         ("speech_m.prenet.fc1.w", 64), ("speech_m.encoder.l0.w", 128), ("speech_m.decoder.l0.w", 192), ("speech_m.postnet.conv1.w", 64),
         ("discriminator.fc2.weight", 64)]
st.offsets, st.params, off = {}, {}, 0
for n, k in names:
    st.offsets[n] = off; st.params[n] = P(k); off += k
st.regions = {"gen": (0, 960), "disc": (960, 1024)}
st.grad = torch.arange(1024, dtype=torch.float32) * (rank + 1)
st.touched = {"gen"}
br = ddp.bucket_ranges(st)
assert br == {"text_enc": (0, 256), "text_dec": (256, 512), "speech_enc": (512, 704), "speech_dec": (704, 960)}, br
exp = torch.arange(1024, dtype=torch.float32) * (sum(range(1, world + 1)) / world)
tot = torch.arange(1024, dtype=torch.float32) * sum(range(1, world + 1))          # summed, not yet scaled by 1/world (finish() scales)
own = torch.arange(1024, dtype=torch.float32) * (rank + 1)
# --- generator phase: armed in the last sub-step; the speech encoder is used by two calls (both must finish first) ---
ddp.segment_backward("text_dec", st)                     # not armed yet (an earlier sub-step): nothing may travel
assert ddp._State.log == []
ddp.arm()
for b in ("text_enc", "speech_enc", "speech_enc", "speech_dec", "text_dec"):
    ddp.segment_forward(b)
ddp.segment_backward("text_dec", st)
assert [l[0] for l in ddp._State.log] == ["text_dec"] and torch.allclose(st.grad[256:512], tot[256:512])
assert torch.equal(st.grad[:256], own[:256]) and torch.equal(st.grad[512:], own[512:])       # everything else still local
ddp.segment_backward("speech_dec", st)
ddp.segment_backward("speech_enc", st)                   # first of two users: not final yet
assert [l[0] for l in ddp._State.log] == ["text_dec", "speech_dec"]
ddp.segment_backward("speech_enc", st)
assert [l[0] for l in ddp._State.log] == ["text_dec", "speech_dec", "speech_enc"]
n = ddp.finish(st, [(0, 960)])                            # text_enc never signalled: the optimizer side reduces the remainder
assert n == 1 and ddp._State.log[-1] == ("rest", 0, 256)
assert torch.allclose(st.grad[:960], exp[:960]) and torch.equal(st.grad[960:], own[960:])    # each element reduced exactly once
# --- discriminator phase: nothing pre-issued, one collective over its range ---
st.touched = {"disc"}
n = ddp.finish(st, [(960, 1024)])
assert n == 1 and torch.allclose(st.grad, exp)
assert not ddp._State.armed and ddp._State.issued == []
# --- a cross-model sub-step as the last one (sp_steps = 0): forward order text_enc, speech_dec, speech_enc, text_dec; autograd
# runs the speech ENCODER's backward before the speech DECODER's, and the decoder still adds speech_m.prenet.* gradients into the
# encoder's bucket: that bucket must not travel before the decoder's backward has been enqueued ---
st.grad = torch.arange(1024, dtype=torch.float32) * (rank + 1)
st.touched = {"gen"}
ddp._State.log = []
ddp.arm()
for b in ("text_enc", "speech_dec", "speech_enc", "text_dec"):
    ddp.segment_forward(b)
ddp.segment_backward("text_dec", st)
ddp.segment_backward("speech_enc", st)                   # its own backward is done, the decoder's (same prenet) is not
assert [l[0] for l in ddp._State.log] == ["text_dec"], ddp._State.log
assert torch.equal(st.grad[512:704], own[512:704])
ddp.segment_backward("speech_dec", st)                   # now both buckets of the speech side are final
assert [l[0] for l in ddp._State.log] == ["text_dec", "speech_dec", "speech_enc"], ddp._State.log
ddp.segment_backward("text_enc", st)
assert [l[0] for l in ddp._State.log] == ["text_dec", "speech_dec", "speech_enc", "text_enc"]
n = ddp.finish(st, [(0, 960)])
assert n == 0 and torch.allclose(st.grad[:960], exp[:960]) and torch.equal(st.grad[960:], own[960:])
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_bucketed_gradient_exchange_two_ranks_gloo(tmp_path):
    """unast_amd.ddp: buckets travel when (and only when) their last backward of the armed sub-step has been enqueued, every
    gradient element is reduced exactly once per optimizer phase, and what the hooks did not see is reduced by finish()."""
    script = tmp_path / "w.py"
    script.write_text(_BUCKET_WORKER % ROOT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29535", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=180)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "rank 0 ok" in outs[0] and "rank 1 ok" in outs[1]


def test_golden_fixtures_are_data_only(golden_dir):
    for f in os.listdir(golden_dir):
        if f.endswith(".json"):             # a recorded call trace: JSON holds numbers, strings, lists and objects, nothing that runs
            with open(os.path.join(golden_dir, f)) as fh:
                json.load(fh)
            continue
        assert f.endswith(".npz"), f
        z = np.load(os.path.join(golden_dir, f), allow_pickle=False)
        for k in z.files:
            assert z[k].dtype.kind in "fiubU", (f, k, z[k].dtype)


def test_edit_distance_and_per_known_answers():
    """compute_per restates jiwer==2.2.0's wer (requirements.txt:10; absent here): flatten, Levenshtein / len(truth)."""
    import random
    from unast_amd.utils import edit_distance, compute_per
    assert edit_distance([], []) == 0 and edit_distance([1, 2], []) == 2 and edit_distance([], [5]) == 1
    k, s = [ord(c) for c in "kitten"], [ord(c) for c in "sitting"]
    assert edit_distance(k, s) == 3 and edit_distance(s, k) == 3
    assert edit_distance([1, 2, 3, 4], [1, 2, 3, 4]) == 0
    assert edit_distance([1, 2, 3, 4], [2, 3, 4]) == 1 and edit_distance([1, 2, 3], [4, 1, 2, 3, 5]) == 2

    def slow(a, b):                                         # textbook O(nm) table
        d = [[max(i, j) if 0 in (i, j) else 0 for j in range(len(b) + 1)] for i in range(len(a) + 1)]
        for i in range(1, len(a) + 1):
            for j in range(1, len(b) + 1):
                d[i][j] = min(d[i - 1][j] + 1, d[i][j - 1] + 1, d[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
        return d[-1][-1]
    rnd = random.Random(0)
    for _ in range(50):
        a = [rnd.randrange(4) for _ in range(rnd.randrange(0, 30))]
        b = [rnd.randrange(4) for _ in range(rnd.randrange(0, 30))]
        assert edit_distance(a, b) == slow(a, b)
    gt = torch.tensor([[5, 6, 7, 2, 0], [8, 9, 2, 0, 0]])
    hyp = torch.tensor([[5, 7, 2, 0, 0, 0], [8, 9, 9, 2, 0, 0]])
    per = compute_per(gt, hyp, torch.tensor([4, 3]), torch.tensor([3, 4]))
    assert per == pytest.approx(2 / 7)                      # one deletion + one insertion over 7 reference symbols
    assert compute_per(gt, gt, torch.tensor([4, 3]), torch.tensor([4, 3])) == 0.0


def test_compute_d_score():
    from unast_amd.train import compute_d_score
    out = torch.tensor([2.0, -1.0, 0.3, -0.2])
    tgt = torch.tensor([0.9, 0.1, 0.1, 0.9])
    assert int(compute_d_score(out, tgt)) == 2


def test_replay_planner_under_address_sanitizer(tmp_path):
    """csrc/graph_layout.h (the stream layout of the replay executor, csrc/graph_exec.cpp) on synthetic DAGs, built for the CPU with
    -fsanitize=address,undefined: every dependency ordered by stream order or a record/wait pair, records issued ahead of their waits."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "test_graph_layout")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(root, "tests", "native", "test_graph_layout.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all cases passed" in r.stdout
    src = open(os.path.join(root, "unast_amd", "csrc", "graph_exec.cpp")).read()
    assert "unast_layout::plan_layout" in src, "the executor must plan through the tested header"


def test_weight_plane_plan_geometry():
    """unast_amd.planes (no arithmetic, no GPU): which destination matrices get tiled planes, their padded extents and the 64 x 64 block
    descriptors unast_retile_weights consumes."""
    from unast_amd import planes
    assert planes.eligible(1024, 256) and planes.eligible(81, 256) and planes.eligible(256, 80) and planes.eligible(512, 128)
    assert not planes.eligible(256, 255) and not planes.eligible(256, 228) and planes.eligible(256, 224) is False      # K % 4; 224 < K < 256; 7 k-steps are not built
    assert planes.eligible(256, 1024) and planes.eligible(256, 768) and planes.eligible(512, 512)      # K-streamed form: K % 64 == 0 into 256-column tiles
    assert not planes.eligible(81, 1024) and not planes.eligible(256, 1000)
    ks, pb = planes.geometry(81, 256)
    assert (ks, pb) == (8, 128 * 8 * 64)                                                  # 81 rows padded to 128, 8 k-steps, 64 B per (row, k-step)
    ks, pb = planes.geometry(256, 1024)
    assert (ks, pb) == (32, 256 * 32 * 64)
    descs, placed, total = planes.plan([(0, 256, 0, 81, 256), (81 * 256, 1024, 1, 1024, 256), (0, 1024, 0, 256, 1024)])
    assert descs.dtype.itemsize == 48
    # blocks: ceil64(N) / 64 x ceil(ksteps * 32 / 64)
    assert len(descs) == 2 * 4 + 16 * 4 + 4 * 16
    assert placed[0][0] == 0 and placed[1][0] == 2 * placed[0][1] and placed[2][0] == placed[1][0] + 2 * placed[1][1]
    assert total == placed[2][0] + 2 * placed[2][1]
    d = descs[8]                                                                            # first block of the transposed matrix
    assert (int(d["src_off"]), int(d["ld"]), int(d["transposed"]), int(d["N"]), int(d["K"]), int(d["n0"]), int(d["k0"])) == (81 * 256, 1024, 1, 1024, 256, 0, 0)
    assert int(d["dst_off"]) == placed[1][0] and int(d["plane_bytes"]) == placed[1][1]


def test_parity_mode_and_fixed_summation_order_are_separate_switches():
    """utils.set_deterministic(True) alone (the parity mode of the golden / oracle tests) must NOT select the order-fixed kernels: those tests
    are to pin the kernels the train step runs with.  fixed_sums=True / False switches config.DETERMINISTIC_SUMS, None leaves it alone."""
    from unast_amd import config, ops, utils
    before = config.DETERMINISTIC_SUMS
    try:
        config.DETERMINISTIC_SUMS = False
        utils.set_deterministic(True)
        assert utils.is_deterministic() and not ops.deterministic_sums()
        utils.set_deterministic(True, fixed_sums=True)
        assert ops.deterministic_sums()
        utils.set_deterministic(False)
        assert ops.deterministic_sums() and not utils.is_deterministic()          # (None leaves the sums switch as it is)
        utils.set_deterministic(False, fixed_sums=False)
        assert not ops.deterministic_sums()
    finally:
        config.DETERMINISTIC_SUMS = before
        utils.set_deterministic(False)


def test_bench_dump_outputs_sample_is_fixed(tmp_path, monkeypatch):
    """bench.dump_outputs (--dump-outputs): one float64 file per loss, and a sample of the floating-point state entries (key order) that is
    the same on every call, ascending, within DUMP_STATE_SAMPLE, with integer entries (BatchNorm step counters) left out."""
    import bench
    monkeypatch.setattr(bench, "DUMP_STATE_SAMPLE", 1000)
    state = {"a.weight": torch.arange(3000, dtype=torch.float32).view(30, 100), "bn.num_batches_tracked": torch.tensor(7),
             "b.weight": torch.arange(3000, 5000, dtype=torch.float32).view(100, 20).t()}
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"t_ae": 1.25, "asr_": 2.5}, state)
    assert sorted(os.listdir(tmp_path / "x")) == ["loss_asr_.npy", "loss_t_ae.npy", "state_sample.npy"]
    assert np.load(tmp_path / "x" / "loss_t_ae.npy").tolist() == [1.25] and np.load(tmp_path / "x" / "loss_t_ae.npy").dtype == np.float64
    s, s2 = np.load(tmp_path / "x" / "state_sample.npy"), np.load(tmp_path / "y" / "state_sample.npy")
    assert s.dtype == np.float32 and s.shape == (1000,) and np.array_equal(s, s2)
    flat = np.concatenate([np.arange(3000), np.arange(3000, 5000).reshape(100, 20).T.reshape(-1)]).astype(np.float32)
    idx = np.sort(np.random.default_rng(0).choice(5000, 1000, replace=False))
    assert np.array_equal(s, flat[idx])
    monkeypatch.setattr(bench, "DUMP_STATE_SAMPLE", 1 << 22)
    bench.dump_outputs(str(tmp_path / "z"), {}, state)
    assert np.array_equal(np.load(tmp_path / "z" / "state_sample.npy"), flat)          # small states are written whole
