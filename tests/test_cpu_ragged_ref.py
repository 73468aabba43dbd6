"""Does the per-sequence metric of tests/ragged_ref.py see a key length that is off by one?  For every case of tests/test_gpu_ragged.py and
every sequence shorter than Tk, the fp64 reference is computed a second time with one more visible key: the metric between the two must
be at least 10 x the tolerance the GPU test applies, for O and for dK or dV of that sequence -- a kernel that masks one key too few would
fail there -- and exactly zero for every other sequence of the batch (the per-sequence property).  No GPU, no code under test."""
import pytest
import torch

from tests import ragged_ref as R


@pytest.mark.parametrize("variant", list(R.VARIANTS))
def test_metric_sees_one_key_too_many(variant):
    x = R.inputs(variant)
    fl = R.floors(x)
    tol = max(R.tolerance(x["nsplit"], False), R.tolerance(x["nsplit"], True))
    ref = R.reference_cached(variant)
    for b in range(x["B"]):
        if int(x["lens_k"][b]) >= x["Tk"]:
            continue
        lens = x["lens_k"].clone()
        lens[b] += 1
        other = R.reference(variant, lens)
        err = {n: R.seq_err(other[n], ref[n], fl[n]) for n in ref}
        rest = [i for i in range(x["B"]) if i != b]
        for n in err:
            assert bool((err[n][rest] == 0).all()), (variant, b, n, "another sequence moved")
        o, g = float(err["O"][b]), max(float(err["dK"][b]), float(err["dV"][b]))
        print("%-10s seq %d lens_k %3d -> %3d: O %.2e (%5.0f x tol)  max(dK, dV) %.2e (%5.0f x tol)" % (
            variant, b, int(x["lens_k"][b]), int(lens[b]), o, o / tol, g, g / tol))
        assert o >= 10 * tol, (variant, b, o)
        if x["lens_q"] is not None and (int(x["lens_q"][b]) == 0 or (x["causal"] and int(x["lens_q"][b]) <= int(x["lens_k"][b]))):
            # No query that carries a gradient sees the added key (lens_q = 0: none carries one; causal with lens_q <= lens_k: key lens_k
            # is visible to queries >= lens_k only, whose dO is zero), so the gradients cannot move: the forward check above is the
            # one that sees this length, and the GPU test's exact zeros of dK / dV at keys >= lens_k see a key too many.
            assert g == 0.0
            continue
        assert g >= 10 * tol, (variant, b, g)


def test_lengths_past_tk_are_clamped_and_the_metric_is_per_sequence():
    x = R.inputs("g")
    a, _ = R.attention_ref(x["q"], x["k"], x["v"], torch.tensor([47, 40]), False, R.H)
    b, _ = R.attention_ref(x["q"], x["k"], x["v"], torch.tensor([40, 40]), False, R.H)
    assert torch.equal(a, b)
    ref = torch.zeros(2, 3, 4)
    ref[0] = 100.0
    got = ref.clone()
    got[1, 0, 0] = 0.5          # invisible to a whole-tensor maximum at 1e-2, plain per sequence
    assert R.seq_err(got, ref, 1.0).tolist() == [0.0, 0.5]
