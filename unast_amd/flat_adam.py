"""The Adam(W) core under the package's three optimizers (train.FusedAdamW, train_vocoder.FlatAdamW, train_rnn_step.RNNFlatAdamW): an ordered
list of segments over the two kernels ops.sumsq and ops.adamw.  A segment is a flat parameter range with its gradient range, two moment
ranges, a step count and an optional split-operand output, stepped or skipped as a whole; the segments stepped together share one clip norm.
Nothing here knows a model family: which segments exist, which of them have gradients and what has to be refreshed after an update is the
subclass's business.  state_dict() / load_state_dict() speak torch.optim.AdamW's format (reference checkpoints: src/utils.py:139-195)."""
import math

import torch

from . import ops

_F32 = torch.float32
_TORCH_DEFAULTS = (("amsgrad", False), ("maximize", False), ("foreach", None), ("capturable", False), ("differentiable", False), ("fused", None))
_HYPER_KEYS = ("lr", "weight_decay", "betas", "eps", "initial_lr")


class Segment:
    """One range the optimizer steps or skips as a whole.  `offsets`: element offset of each parameter inside the segment.  `tap_major`: one
    flag per parameter, True where a [Cout, Cin, k] weight is stored [Cout, k, Cin] (the transformer's *.conv.weight).  `m` / `v`: moment
    ranges the caller owns, or None for zeroed buffers of the segment's own."""

    def __init__(self, name, params, offsets, flat, grad, split=None, m=None, v=None, tap_major=None):
        self.name, self.params, self.offsets, self.flat, self.grad, self.split = name, params, offsets, flat, grad, split
        self.m = torch.zeros_like(flat) if m is None else m
        self.v = torch.zeros_like(flat) if v is None else v
        self.tap_major = [False] * len(params) if tap_major is None else tap_major
        self.step = 0

    def moments(self):
        """[(parameter, its exp_avg range, its exp_avg_sq range)], both as views in torch's shape."""
        out = []
        for p, o, tap in zip(self.params, self.offsets, self.tap_major):
            m, v = self.m[o:o + p.numel()], self.v[o:o + p.numel()]
            if tap:
                co, ci, ks = p.shape
                out.append((p, m.view(co, ks, ci).permute(0, 2, 1), v.view(co, ks, ci).permute(0, 2, 1)))
            else:
                out.append((p, m.view(p.shape), v.view(p.shape)))
        return out


def adopt(name, params):
    """A segment over flat buffers of its own: every parameter at a 16-byte boundary, zero padding between; the values are copied in and
    p.data and p.grad become views."""
    offsets, total = [], 0
    for p in params:
        offsets.append(total)
        total += (p.numel() + 3) // 4 * 4
    dev = params[0].device
    flat, grad = torch.zeros(total, dtype=_F32, device=dev), torch.zeros(total, dtype=_F32, device=dev)
    with torch.no_grad():
        for p, o in zip(params, offsets):
            view = flat[o:o + p.numel()].view(p.shape)
            view.copy_(p)
            p.data = view
            p.grad = grad[o:o + p.numel()].view(p.shape)
    return Segment(name, params, offsets, flat, grad)


def _fresh(view):
    """A CPU tensor of the view's shape that shares no storage with it (.cpu() alone returns a CPU tensor itself)."""
    return torch.empty(view.shape, dtype=view.dtype).copy_(view.detach())


class FlatAdam(torch.optim.Optimizer):
    """torch.optim.AdamW (decoupled=True) or torch.optim.Adam with L2 weight decay (decoupled=False) with clip_grad_norm_ folded in, over
    `segments`; `params` in model.parameters() order are torch's parameter indices.  Works with torch LR schedulers (param_groups[0]['lr'])."""

    def __init__(self, params, segments, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, decoupled=True):
        super().__init__(params, dict(lr=lr, weight_decay=weight_decay, betas=betas, eps=eps))
        self.segments, self.decoupled = segments, bool(decoupled)
        self._ss = torch.zeros(1, dtype=torch.float64, device=self.param_groups[0]["params"][0].device)      # squared gradient norm of the last step

    def _launch(self, segs, max_norm, dev_hyper=None, zero_grad=False):
        """One sum-of-squares launch per segment into the zeroed norm scalar, then one clip+AdamW launch per segment, in list order.
        dev_hyper (a step recorded into a HIP graph): one float32 [3] device block per segment from which the launch reads the learning rate
        and the bias corrections at replay time; the step counts then advance per replay, not here.  zero_grad: the update pass also zeroes
        the gradients it consumed."""
        g = self.param_groups[0]
        self._ss.zero_()
        for s in segs:
            ops.sumsq(s.grad, self._ss)
        for i, s in enumerate(segs):
            if dev_hyper is None:
                s.step += 1
                lr, step, hyper = float(g["lr"]), s.step, None
            else:
                lr, step, hyper = 0.0, 0, dev_hyper[i]
            ops.adamw(s.flat, s.grad, s.m, s.v, self._ss, float(max_norm), lr, g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], step,
                      split_out=s.split, decoupled=self.decoupled, dev_hyper=hyper, zero_grad=zero_grad)

    def grad_norm(self):
        """Pre-clip global gradient norm of the last step (one host read; for logging and tests)."""
        return math.sqrt(float(self._ss.item()))

    def state_dict(self):
        params = self.param_groups[0]["params"]
        index = {id(p): i for i, p in enumerate(params)}
        state = {}
        for s in self.segments:
            if s.step == 0:
                continue                                   # never stepped: torch keeps no state either
            for p, m, v in s.moments():
                state[index[id(p)]] = {"step": torch.tensor(float(s.step)), "exp_avg": _fresh(m), "exp_avg_sq": _fresh(v)}
        g = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        g["params"] = list(range(len(params)))
        for key, val in _TORCH_DEFAULTS:
            g.setdefault(key, val)
        return {"state": dict(sorted(state.items())), "param_groups": [g]}

    def load_state_dict(self, sd):
        index = {id(p): i for i, p in enumerate(self.param_groups[0]["params"])}
        for s in self.segments:
            s.m.zero_(); s.v.zero_()
            s.step = 0
            for p, m, v in s.moments():
                i = index[id(p)]
                ent = sd["state"].get(i, sd["state"].get(str(i)))
                if ent is None:
                    continue
                m.copy_(ent["exp_avg"].reshape(p.shape))
                v.copy_(ent["exp_avg_sq"].reshape(p.shape))
                s.step = max(s.step, int(float(ent["step"])))
        g = sd["param_groups"][0]
        for key in _HYPER_KEYS:
            if key in g:
                self.param_groups[0][key] = tuple(g[key]) if key == "betas" else g[key]
