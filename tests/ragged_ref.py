"""fp64 references, the per-sequence error metric and the case table of the ragged-length attention tests (tests/test_gpu_ragged.py runs
the kernels on these cases; tests/test_cpu_ragged_ref.py proves, without the kernels, that the metric sees a length that is off by one).

The metric is taken per sequence: a length-1 sequence has dV[b, 0] = sum_q dO[b, q], of size ~ sqrt(Tq), and a whole-tensor maximum
would hide an error in the long sequences of the same batch behind that one row.

    err[b] = max |got[b] - ref[b]| / max(max |ref[b]|, floor)

The floors start from those of tools/fuzz_attention.py: 1 for O, LSE and dQ (operands are N(0,1); with a single visible key the exact dQ
and dK are zero and what is left is the split products' absolute error), sqrt(Tq) for dK and dV of a one-key sequence (they sum over the
queries) and, per sequence, sqrt(Tq) / klen for a longer one: see floors()."""
import functools
import math

import torch

from tests import dropout_mirror as M

H, E = 4, 256
SEED, STREAM, DROP_P = 0x5EED1234, 7, 0.1

# name -> Tq, Tk, causal, lens_k[, lens_q]      (B is the number of lengths)
CASES = {
    "a": (257, 257, False, [257, 1, 31, 129]),      # single key; under one 32-key chunk; block 1 with one live key and block 2 dead
    "b": (257, 257, True, [257, 1, 33, 64]),        # causal with queries far past klen; kmax from the length; length on the 64-key tile edge
    "c": (33, 300, False, [300, 2, 65, 256]),       # length on the 128-key block edge (block 2 dead); one key into the second tile
    "d": (300, 37, False, [37, 1, 16, 36]),         # many query blocks over a tiny key set
    "e": (1, 130, False, [130, 1, 128]),            # single query
    "f": (5, 5, True, [5, 1, 3]),                   # everything inside one tile
    "g": (40, 40, False, [47, 40]),                 # lens_k > Tk is clamped
    "h": (100, 200, False, [200, 5, 129, 64]),      # lens_q independent of lens_k (see VARIANTS)
}
LENS_Q = {"a": [257, 1, 31, 129], "b": [257, 1, 33, 64], "h": [100, 1, 32, 0]}

# id -> (case, nsplit, dropout rate, lens_q given)
VARIANTS = {}
for _c in "abcdefg":
    VARIANTS[_c] = (_c, 3, 0.0, False)
for _c in "acd":
    VARIANTS[_c + "-drop"] = (_c, 3, DROP_P, False)
for _c in "ab":
    VARIANTS[_c + "-nsplit1"] = (_c, 1, 0.0, False)
for _c in "abh":
    VARIANTS[_c + "-lensq"] = (_c, 3, 0.0, True)

# Operands are N(0,1), except Q of b-nsplit1: under the causal mask one more key among 64 moves O by 0.1 of its size only, below 10 x the
# 2e-2 bound of nsplit = 1 that tests/test_cpu_ragged_ref.py wants; Q x 2 sharpens the softmax (a power of two: the relative rounding error
# of every bf16 / fp32 product stays what it is at N(0,1)).
Q_SCALE = {"b-nsplit1": 2.0}


def tolerance(nsplit, presplit):
    """vs fp64: the bounds of test_attention_fwd_bwd / test_attention_dropout_against_fp64 (5e-5 with three bf16 terms, 2e-2 with one);
    pre-split operands carry 16 mantissa bits: the fuzz tool's 2e-4."""
    if nsplit == 1:
        return 2e-2
    return 2e-4 if presplit else 5e-5


def floors(x):
    """The natural scale of each output of inputs(variant) where its exact value degenerates, per sequence ([B] each).  O, LSE, dQ: 1 (N(0,1)
    operands; with one visible key the exact dQ is zero and the split products' absolute error is what is left).  dK, dV: every element
    sums Tq terms P[q, key] * N(0,1) of random sign, P ~ 1 / klen: sqrt(Tq) / klen.  At klen = 1 that is the fuzz tool's sqrt(Tq) (the
    exact dK is zero there); on a long sequence sqrt(Tq) itself would exceed every element of dK and dV several times, and 2e-2 of it
    would pass a gradient that is wrong altogether."""
    B = x["B"]
    klen = x["lens_k"].clamp(1, x["Tk"]).double()
    one = torch.ones(B, dtype=torch.float64)
    kv = (math.sqrt(x["Tq"]) / klen).clamp_min(1e-30)
    return {"O": one, "LSE": one, "dQ": one, "dK": kv, "dV": kv}


def seq_err(got, ref, floor):
    """float64 [B]: max |got[b] - ref[b]| / max(max |ref[b]|, floor[b])  (floor: a number or [B])."""
    B = ref.shape[0]
    got, ref = got.detach().double().cpu().reshape(B, -1), ref.detach().double().cpu().reshape(B, -1)
    return (got - ref).abs().amax(1) / torch.maximum(ref.abs().amax(1), torch.as_tensor(floor, dtype=torch.float64).expand(B))


def attention_ref(q, k, v, lens_k, causal, H, drop_factor=None):
    """fp64 multi-head attention (head dim E / H) over the first clamp(lens_k[b], 0, Tk) keys, causal or not; drop_factor ([B, H, Tq, Tk],
    0 or 1 / (1 - p)) multiplies the normalised probabilities.  Returns O [B, Tq, E] and the LSE [B, H, Tq] of the undropped scores."""
    B, Tq, E = q.shape
    Tk = k.shape[1]
    hd = E // H
    lens_k = torch.as_tensor(lens_k).clamp(0, Tk)
    qh = q.view(B, Tq, H, hd).transpose(1, 2) / math.sqrt(hd)
    kh = k.view(B, Tk, H, hd).transpose(1, 2)
    vh = v.view(B, Tk, H, hd).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2)
    neg = ~(torch.arange(Tk)[None, :] < lens_k[:, None])[:, None, None, :]
    if causal:
        neg = neg | (torch.arange(Tk)[None, :] > torch.arange(Tq)[:, None])[None, None]
    s = s.masked_fill(neg, float("-inf"))
    p = torch.softmax(s, -1)
    if drop_factor is not None:
        p = p * drop_factor
    return (p @ vh).transpose(1, 2).reshape(B, Tq, E), torch.logsumexp(s, -1)


@functools.lru_cache(maxsize=None)
def inputs(variant):
    """The operands of a variant, fp64 and read-only by convention: q, k, v, dO (zero at queries >= lens_q where lens_q is given), lens_k,
    lens_q (or None), the dropout rate p."""
    case, nsplit, p, with_lens_q = VARIANTS[variant]
    Tq, Tk, causal, lens_k = CASES[case]
    B = len(lens_k)
    g = torch.Generator().manual_seed(1000 * (ord(case) - ord("a") + 1) + Tq + Tk)
    q = torch.randn(B, Tq, E, generator=g, dtype=torch.float64)
    k = torch.randn(B, Tk, E, generator=g, dtype=torch.float64)
    v = torch.randn(B, Tk, E, generator=g, dtype=torch.float64)
    do = torch.randn(B, Tq, E, generator=g, dtype=torch.float64)
    q = q * Q_SCALE.get(variant, 1.0)
    lens_q = None
    if with_lens_q:
        lens_q = torch.tensor(LENS_Q[case])
        do = do * (torch.arange(Tq)[None, :] < lens_q[:, None])[..., None]
    return dict(case=case, nsplit=nsplit, p=p, B=B, Tq=Tq, Tk=Tk, causal=causal, q=q, k=k, v=v, do=do, lens_k=torch.tensor(lens_k),
                lens_q=lens_q)


@functools.lru_cache(maxsize=None)
def drop_factor(variant, epoch=0):
    """[B, H, Tq, Tk] factor on the probabilities, 0 or 1 / (1 - p): the kernels' mask at (SEED, STREAM) and the RNG epoch; None without dropout"""
    x = inputs(variant)
    if x["p"] == 0:
        return None
    return torch.from_numpy(M.attn_keep(SEED, STREAM, x["B"], H, x["Tq"], x["Tk"], x["p"], epoch) * float(M.drop_scale(x["p"])))


def reference(variant, lens_k=None, epoch=0):
    """O, LSE, dQ, dK, dV in fp64 for the variant's operands (lens_k: other key lengths than the variant's own)."""
    x = inputs(variant)
    q, k, v = (x[n].clone().requires_grad_(True) for n in "qkv")
    o, lse = attention_ref(q, k, v, x["lens_k"] if lens_k is None else lens_k, x["causal"], H, drop_factor(variant, epoch))
    o.backward(x["do"])
    return {"O": o.detach(), "LSE": lse.detach(), "dQ": q.grad, "dK": k.grad, "dV": v.grad}


@functools.lru_cache(maxsize=None)
def reference_cached(variant, epoch=0):
    return reference(variant, epoch=epoch)
