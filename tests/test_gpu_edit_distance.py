"""unast_edit_distance (csrc/metrics.hip) and utils.compute_per_device against the host functions they restate, utils.edit_distance and
utils.compute_per: everything is integer arithmetic, so every comparison is exact.  Shapes sit on the kernel's edges: a wave (64 columns at one
column per thread), the workgroup (1024 threads: the chunk doubles behind it), one and two thread chunks and 64 chunks (a wave) at every chunk
size -- the larger chunk sizes are forced at small shapes through the `chunk` argument, so that each template instance runs in milliseconds.
Padding behind every len[b] holds poison ids (-1, 2^40) and the rows are strided."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = (-1, 1 << 40)


def _dev():
    return torch.device("cuda:0")


def _split(seq, rng, rows):
    """Cuts a flat sequence into `rows` pieces, some of them empty."""
    cuts = np.sort(rng.randint(0, len(seq) + 1, size=rows - 1)) if rows > 1 else np.zeros(0, dtype=np.int64)
    if rows > 2:
        cuts[1] = cuts[0]                                   # an empty row between non-empty ones
    return [list(p) for p in np.split(np.asarray(seq, dtype=np.int64), cuts)]


def _pack(rows_a, rows_b, pad=3):
    """Two ragged batches as strided int64 device tensors with poison behind every length, and int32 lengths."""
    B = max(len(rows_a), len(rows_b))
    out = []
    for rows in (rows_a, rows_b):
        rows = rows + [[]] * (B - len(rows))
        T = max(len(r) for r in rows)
        full = np.empty((B, T + pad), dtype=np.int64)
        full[:, 0::2], full[:, 1::2] = POISON[0], POISON[1]
        for b, r in enumerate(rows):
            full[b, :len(r)] = r
        t = torch.from_numpy(full).to(_dev())
        out += [t[:, :T], torch.tensor([len(r) for r in rows], dtype=torch.int32, device=_dev())]
    return out


def _mutate(seq, rng, vocab, rate=0.2):
    out = []
    for v in seq:
        u = rng.rand()
        if u < rate / 3:
            continue
        out.append(int(rng.randint(vocab)) if u < 2 * rate / 3 else int(v))
        if u > 1 - rate / 3:
            out.append(int(rng.randint(vocab)))
    return out


def _check(ref_rows, hyp_rows, chunk=0):
    from unast_amd import ops, utils
    ref, rl, hyp, hl = _pack(ref_rows, hyp_rows)
    assert ref.shape[1] == 0 or ref.stride(0) > ref.shape[1]
    got = ops.edit_distance(ref, rl, hyp, hl, chunk=chunk).tolist()
    flat_r = [t for r in ref_rows for t in r]
    flat_h = [t for r in hyp_rows for t in r]
    want = [utils.edit_distance(flat_r, flat_h), len(flat_r)]
    assert got == want, (len(flat_r), len(flat_h), chunk, got, want)
    if flat_r:
        per = utils.compute_per_device(ref, hyp, rl, hl)
        assert per == utils.compute_per(ref.cpu(), hyp.cpu(), rl.cpu(), hl.cpu()) == want[0] / float(want[1])
    return got


def _pair(n, m, seed, vocab=60, rows=3):
    """A reference of n ids and a hypothesis of exactly m ids derived from it, each cut into `rows` ragged rows."""
    rng = np.random.RandomState(seed)
    ref = rng.randint(vocab, size=n).tolist()
    hyp = _mutate(ref, rng, vocab)
    hyp = (hyp + rng.randint(vocab, size=max(m - len(hyp), 0)).tolist())[:m]
    return _split(ref, rng, rows), _split(hyp, rng, rows)


def test_constants_are_the_kernels():
    from unast_amd import ops
    assert ops.edit_distance_limits() == (ops.EDIT_THREADS, ops.EDIT_CHUNK) == (1024, 64) and ops.EDIT_MAX_COLS == 65536


def test_empty_sequences():
    from unast_amd import ops, utils
    assert _check([[], []], [[], []]) == [0, 0]                         # both empty after flattening: distance 0 from ops ...
    ref, rl, hyp, hl = _pack([[], []], [[], []])
    with pytest.raises(ValueError, match="compute_per: empty ground truth"):        # ... and the helper refuses, as compute_per does
        utils.compute_per_device(ref, hyp, rl, hl)
    assert _check([[4, 5], [6]], [[], []]) == [3, 3]                    # hyp empty
    assert _check([[], []], [[7], [8, 9]]) == [3, 0]
    ref, rl, hyp, hl = _pack([[], []], [[7], [8, 9]])
    with pytest.raises(ValueError, match="compute_per: empty ground truth"):
        utils.compute_per_device(ref, hyp, rl, hl)
    z = torch.zeros(2, 0, dtype=torch.int64, device=_dev())             # T = 0 tensors
    zl = torch.zeros(2, dtype=torch.int32, device=_dev())
    assert ops.edit_distance(z, zl, z, zl).tolist() == [0, 0]


def test_short_rows_and_single_ids():
    assert _check([[3]], [[3]]) == [0, 1]                               # B = 1, length 1
    assert _check([[3]], [[4]]) == [1, 1]
    assert _check([[3]], [[4, 3]]) == [1, 1]
    assert _check([[1, 2], [], [3], [], [4, 5, 6]], [[1], [2, 3, 9], [], [4, 6], []])[1] == 6          # rows of length 0 between non-empty rows


@pytest.mark.parametrize("vocab", [2, 60])
def test_identical_swapped_and_vocabularies(vocab):
    ref, hyp = _pair(300, 257, seed=vocab, vocab=vocab, rows=4)
    assert _check(ref, ref)[0] == 0                                     # identical
    a = _check(ref, hyp)                                                # hyp shorter: the direct path
    b = _check(hyp, ref)                                                # ref shorter: the transposed path
    assert a[0] == b[0] and (a[1], b[1]) == (300, 257)


def test_ids_are_compared_as_full_int64():
    hi = 1 << 32
    ref = [[5, 7 + hi, 9], [11 + 2 * hi, 5 - hi]]
    hyp = [[5 + hi, 7 + hi], [9 + hi, 11 + 2 * hi, 5 - hi]]
    assert _check(ref, hyp) == [2, 5]                                   # two ids differ only above bit 32
    assert _check(ref, [[5, 7, 9], [11, 5]])[0] == 3
    rng = np.random.RandomState(3)                                      # a longer one: the same low words everywhere, the high words decide
    r = (rng.randint(3, size=200).astype(np.int64) << 32) + 17
    h = (rng.randint(3, size=170).astype(np.int64) << 32) + 17
    _check(_split(r, rng, 3), _split(h, rng, 3))
    _check(_split(r, rng, 2), _split(h, rng, 2), chunk=64)


@pytest.mark.parametrize("m", [63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049])
def test_wave_and_workgroup_edges(m):
    """One column per thread up to 1024 columns: 64 is the wave's edge, 1024 the workgroup's; behind it two columns per thread up to 2048, then four."""
    _check(*_pair(m + 37, m, seed=m))


@pytest.mark.parametrize("chunk", [2, 4, 8, 16, 32, 64])
def test_every_chunk_size_at_its_edges(chunk):
    """One and two thread chunks and a wave of chunks, each - 1, at it and + 1, with that many columns per thread forced."""
    for m in sorted({chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1, 64 * chunk - 1, 64 * chunk, 64 * chunk + 1}):
        ref, hyp = _pair(m + 21, m, seed=1000 * chunk + m, vocab=2 if m % 2 else 60)
        _check(ref, hyp, chunk=chunk)
        _check(hyp, ref, chunk=chunk)


def test_ragged_batch_and_two_runs_give_the_same_bits():
    from unast_amd import ops
    rng = np.random.RandomState(11)
    ref = rng.randint(45, size=3000).tolist()
    hyp = _mutate(ref, rng, 45)[:2500]
    ref_rows, hyp_rows = _split(ref, rng, 16), _split(hyp, rng, 16)
    _check(ref_rows, hyp_rows)
    a, al, b, bl = _pack(ref_rows, hyp_rows)
    first, second = ops.edit_distance(a, al, b, bl), ops.edit_distance(a, al, b, bl)
    assert torch.equal(first, second)


def test_the_limit_is_checked_before_any_launch():
    from unast_amd import ops
    from unast_amd._lib import lib
    dev = _dev()
    B, T = 64, ops.EDIT_MAX_COLS // 64
    ids = torch.full((B, T), 7, dtype=torch.int64, device=dev)         # at the limit: 65536 ids of capacity on both sides
    lens = torch.zeros(B, dtype=torch.int32, device=dev)
    lens[3], lens[40] = 5, 2
    assert ops.edit_distance(ids, lens, ids, lens).tolist() == [0, 7]
    wide = torch.full((B, T + 1), 7, dtype=torch.int64, device=dev)    # one column more on both sides: refused
    with pytest.raises(ValueError, match="limit"):
        ops.edit_distance(wide, lens, wide, lens)
    assert ops.edit_distance(wide, lens, ids, lens).tolist() == [0, 7]  # only the shorter side is limited
    out = torch.full((2,), -5, dtype=torch.int32, device=dev)           # the C entry point itself: the package's error code, nothing written
    ws = torch.empty(2 * B * (T + 1), dtype=torch.int64, device=dev)
    rc = lib().unast_edit_distance(wide.data_ptr(), T + 1, lens.data_ptr(), T + 1, wide.data_ptr(), T + 1, lens.data_ptr(), T + 1, B, 0,
                                   ws.data_ptr(), ws.numel() * 8, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and b"limit" in lib().unast_last_error() and out.tolist() == [-5, -5]
