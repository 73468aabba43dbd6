"""A recording stand-in for the HIP library handle, and the one train step whose C-ABI call sequence tests/test_gpu_call_trace.py pins
against tests/golden/call_trace_b4_t24_m64_l2.json (written by tools/gen_call_trace.py).

The recorder replaces every module-level binding of `lib` in unast_amd (`_lib.lib`, `ops.lib`, ...; functions that import it at call
time pick the replacement up from `_lib`).  It forwards each call to the real library and appends one record: the entry point's name, then
its arguments in order -- integers as they are, floats as `repr`, a data pointer as 0 / 1 (null or not), a hipStream_t as the ordinal of that
handle's first appearance in the trace; the `*_ws_floats` queries also record what they returned.  Product code is not touched."""
import ctypes
import json
import re
import sys

import torch

SHAPE = (4, 24, 64)                  # batch, text length, mel length
FIXTURE = "call_trace_b4_t24_m64_l2.json"
VARIANTS = {                         # name -> settings of unast_amd.config; the *_panel ones send the small shape down the headline shape's routes
    "joint_tile": dict(JOINT_GEN=True, PANEL_MIN_ROWS=16384),
    "joint_panel": dict(JOINT_GEN=True, PANEL_MIN_ROWS=1, WGRAD_STREAM_MIN_TOKENS=128),
    "split_tile": dict(JOINT_GEN=False, PANEL_MIN_ROWS=16384),
    "split_panel": dict(JOINT_GEN=False, PANEL_MIN_ROWS=1, WGRAD_STREAM_MIN_TOKENS=128),
}
GRAPHED = ("joint_tile", "split_tile")          # variants whose captured step's node counts are pinned too
GRAPH_KEYS = ("kernels", "memsets", "memcpys")  # compared; cross_stream_edges and streams are reported only


def _param_kinds():
    """{entry point: [kind per argument]}: 'i' integer, 'f' float, 'p' data pointer, 's' hipStream_t.  Types as _lib.parse_header maps them;
    the header's own text tells a stream from a pointer (both are void pointers to ctypes)."""
    from unast_amd import _lib
    src = open(_lib.HEADER_PATH).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\b(unast_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)}
    kinds = {}
    for name, (_, argtypes) in _lib.parse_header().items():
        texts = [a for a in decls[name].split(",")] if argtypes else []
        assert len(texts) == len(argtypes), name
        ks = []
        for t, text in zip(argtypes, texts):
            if t is ctypes.c_void_p:
                ks.append("s" if "hipStream_t" in text else "p")
            else:
                ks.append("f" if t in (ctypes.c_float, ctypes.c_double) else "i")
        kinds[name] = ks
    return kinds


class Recorder:
    """Callable like `_lib.lib` (returns the handle: itself); attribute access gives the recording wrapper of an entry point."""

    def __init__(self, real):
        self._real, self._kinds = real, _param_kinds()
        self.records, self._streams = [], {}

    def __call__(self):
        return self

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        kinds = self._kinds.get(name)
        if kinds is None:
            return fn

        def call(*args):
            ret = fn(*args)
            rec = [name]
            for k, a in zip(kinds, args):
                if k == "i":
                    rec.append(int(a))
                elif k == "f":
                    rec.append(repr(float(a)))
                elif k == "p":
                    rec.append(1 if a else 0)
                else:
                    rec.append(self._streams.setdefault(a or 0, len(self._streams)))
            if name.endswith("_ws_floats"):
                rec.append("=%d" % ret)
            self.records.append(rec)
            return ret
        return call


def install(mp):
    """Puts a Recorder over every module-level `lib` of unast_amd through the MonkeyPatch `mp`; returns it."""
    from unast_amd import _lib
    rec = Recorder(_lib.ctypes_lib())
    real = _lib.lib
    for name, mod in list(sys.modules.items()):
        if (name == "unast_amd" or name.startswith("unast_amd.")) and mod is not None and mod.__dict__.get("lib") is real:
            mp.setattr(mod, "lib", rec)
    return rec


def _setup(mp, settings):
    from unast_amd import config, train, utils
    from unast_amd.configs import make_args
    from unast_amd.portable import synth_batch
    for k, v in settings.items():
        mp.setattr(config, k, v)
    dev = torch.device("cuda:0")
    mp.setattr(train, "DEVICE", dev)
    args = make_args(num_layers=2, ae_steps=1, sp_steps=1, d_steps=1, cm_steps=0, use_discriminator=True)
    utils.set_seed(0)
    utils.set_deterministic(False)          # parity mode off: dropout, noise, SpecAugment and the permutation are live
    _, _, model, opt, _ = train.initialize_model(args)
    mk = lambda s: tuple(torch.from_numpy(x).to(dev) for x in synth_batch(*SHAPE, seed=s, ragged=True))
    return args, model, opt, dict(unsup=[mk(1)], sup=[mk(2)], disc=[mk(3)], cm=[])


def record_step(mp, settings):
    """The C-ABI records of the second eager train step under `settings` (the first is the warm-up)."""
    from collections import defaultdict
    from unast_amd import train
    args, model, opt, batches = _setup(mp, settings)
    losses = defaultdict(list)
    train.train_step(losses, model, opt, None, batches, 0, args, defer_d_phase=False)
    torch.cuda.synchronize()
    rec = install(mp)
    train.train_step(losses, model, opt, None, batches, 1, args, defer_d_phase=False)
    torch.cuda.synchronize()
    return rec.records


def captured_counts(mp, settings):
    """plan_info of the step captured by GraphedTrainStep under `settings`: the node counts see the torch-native launches too."""
    from collections import defaultdict
    from unast_amd.graphed import GraphedTrainStep
    args, model, opt, batches = _setup(mp, settings)
    stepper = GraphedTrainStep(model, opt, None, args)
    losses = defaultdict(list)
    for i in range(3):                      # generator phase alone, the shifted body eagerly, then its capture + first replay
        stepper(losses, batches, i)
    assert len(stepper.graphs) == 1
    info = dict(next(iter(stepper.graphs.values())).plan_info)
    stepper.flush(losses)
    torch.cuda.synchronize()
    return info


def first_difference(got, want):
    """(index, got record, wanted record) of the first position at which two record lists differ, or None."""
    for i in range(max(len(got), len(want))):
        g, w = (got[i] if i < len(got) else None), (want[i] if i < len(want) else None)
        if g != w:
            return i, g, w
    return None


def as_multiset(records):
    return sorted(json.dumps(r) for r in records)
