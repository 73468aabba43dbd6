"""The host mirror of the kernels' mask RNG (tests/dropout_mirror.py): threshold rounding, keep rates, independence of the halves of a
hash pair, of neighbouring rows, streams and seeds, and the RNG-epoch regression of csrc/common.h (rng_stream_base).  No GPU."""
import math

import numpy as np
import pytest

from tests import dropout_mirror as M


@pytest.mark.parametrize("p,thresh", [(0.1, 6554), (0.25, 16384), (0.5, 32768), (0.0, 0), (1.0, 65535)])
def test_threshold_rounding(p, thresh):
    """drop_threshold: round(p * 2^16) of the fp32 rate, clamped to 16 bits (p = 0.1 in fp32 is 0.100000001..., 6553.6 -> 6554)."""
    assert M.drop_threshold(p) == thresh


def test_scale_is_the_fp32_reciprocal():
    assert M.drop_scale(0.1) == np.float32(1.0) / np.float32(0.9)
    assert M.drop_scale(0.5) == np.float32(2.0)
    assert M.drop_scale(0.0) == np.float32(1.0)


def test_pcg_hash_known_values():
    """Literal values of the kernels' pcg_hash, rng_row_key (epoch 0 and 4) and rng_pair, taken from a C++ build of the functions in
    unast_amd/csrc/common.h: a wrong shift, constant or order of mixing in the mirror changes them.  (The GPU tests then check the
    kernels' masks against the mirror element for element.)"""
    vs = np.array([0, 1, 2, 0xFFFFFFFF, 123456789, 0x80000000], np.uint64)
    assert [int(x) for x in M.pcg_hash(vs)] == [129708002, 2831084092, 2055130248, 3861530882, 4272394698, 566699590]
    assert int(M.rng_row_key(5, 3, 7)) == 1034514340
    assert int(M.rng_row_key(5, 3, 7, epoch=4)) == 266229116
    assert int(M.rng_pair(0x12345678, 10)) == 233568954 == int(M.rng_pair(0x12345678, 11))


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_keep_rate_within_5_sigma(p):
    n_rows, n_cols = 1000, 1000
    keep = M.keep_mask(17, 4, n_rows, n_cols, p)
    n = keep.size
    q = 1.0 - M.drop_threshold(p) / 65536.0
    assert abs(keep.mean() - q) < 5 * math.sqrt(q * (1 - q) / n)
    rows = M.row_keep(17, 4, 10 ** 6, p)
    assert abs(rows.mean() - q) < 5 * math.sqrt(q * (1 - q) / rows.size)


def _corr(a, b):
    a = a.astype(np.float64).ravel(); b = b.astype(np.float64).ravel()
    return float(np.corrcoef(a, b)[0, 1])


def test_no_correlation_between_halves_rows_streams_seeds():
    p, R, C = 0.5, 1000, 1000
    n = R * C // 2
    bound = 5 / math.sqrt(n)
    k = M.keep_mask(1, 2, R, C, p)
    assert abs(_corr(k[:, 0::2], k[:, 1::2])) < bound                      # the two 16-bit halves of one hash
    assert abs(_corr(k[0::2], k[1::2])) < bound                            # adjacent rows
    assert abs(_corr(k, M.keep_mask(1, 3, R, C, p))) < 5 / math.sqrt(R * C)      # adjacent streams
    assert abs(_corr(k, M.keep_mask(2, 2, R, C, p))) < 5 / math.sqrt(R * C)      # adjacent seeds
    r = M.row_keep(1, 2, 10 ** 6, p)
    assert abs(_corr(r[0::2], r[1::2])) < 5 / math.sqrt(r.size // 2)


def test_epoch_is_hashed_apart_from_the_stream():
    """common.h rng_stream_base: with stream + epoch under one hash, site s at epoch e + 1 drew exactly site s + 1's mask at epoch e."""
    for s, e in ((3, 0), (7, 5), (1, 1000)):
        a = M.keep_mask(9, s, 64, 256, 0.5, epoch=e + 1)
        b = M.keep_mask(9, s + 1, 64, 256, 0.5, epoch=e)
        assert abs(float((a == b).mean()) - 0.5) < 0.02
        assert not np.array_equal(M.rng_stream_base(9, s, e + 1), M.rng_stream_base(9, s + 1, e))
    assert np.array_equal(M.keep_mask(9, 3, 8, 8, 0.5, epoch=0), M.keep_mask(9, 3, 8, 8, 0.5))
    assert not np.array_equal(M.keep_mask(9, 3, 64, 64, 0.5, epoch=1), M.keep_mask(9, 3, 64, 64, 0.5))


def test_index_arrays_equal_ranges():
    full = M.keep_mask(4, 5, 50, 70, 0.3)
    rows, cols = np.array([3, 49, 0]), np.array([69, 1, 2, 33])
    assert np.array_equal(M.keep_mask(4, 5, rows, cols, 0.3), full[rows][:, cols])
    assert np.array_equal(M.attn_keep(4, 5, 2, 5, 5, 70, 0.3).reshape(50, 70), full)
    f = M.drop_factor(4, 5, 50, 70, 0.3)
    assert set(np.unique(f)) <= {0.0, float(M.drop_scale(0.3))}
