"""Host mirror, in numpy, of the counter-based mask RNG of the HIP kernels (unast_amd/csrc/common.h): the same uint32 arithmetic, so
that a test can predict bit for bit which elements a kernel drops and compare the kernel with fp64 math under exactly that mask.

Every mask is a function of (seed, stream, row, col) and the RNG epoch only:

    base     = pcg(stream + pcg(epoch + pcg(seed)))       rng_stream_base
    row_key  = pcg(row + base)                             rng_row_key
    h        = ((col >> 1) ^ row_key) * 0x9E3779B1; h ^= h >> 15     rng_pair: one hash serves columns 2j and 2j + 1
    keep     = (col odd ? h >> 16 : h & 0xFFFF) >= thresh  rng_keep
    thresh   = (uint32)(min(p * 65536 + 0.5, 65535))       drop_threshold (p as fp32, the product in double)
    scale    = 1 / (1 - p) in fp32                         the kept elements' factor

What "row" and "col" are at each site:

* element-wise kernels (embed_fwd / embed_bwd, posenc_fwd / posenc_bwd, bn_fwd / bn_bwd, layernorm_bwd's dz_drop, leaky_dropout): row =
  index of the row in the [rows, D] operand as passed to the kernel (token b * T + t of that call), col = feature index;
* GEMM and row-panel epilogues (linear_fwd, panel_gemm, gate_bits, the LayerNorm epilogue, linear_dgrad_lnbwd): row = output row m of
  the view handed to the call, col = output column n within it (a column slice of a wider buffer starts again at 0);
* attention (attn_fwd / attn_bwd): row = (b * H + h) * Tq + q, col = key index within the sequence (0 .. Tk - 1);
* noise_fn (rowmask) and embed_*'s noise: the row form -- row r is kept iff keep(row_key(seed, stream, r), col = 0), no rescale;
* decode_attn: row = b * H + h (one query per sequence), col = key index; decode_linear: epilogue row = m (sequence), col = output
  column n; prologue dropouts row = m, col = input feature k.
"""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def _u32(x):
    return np.asarray(x, dtype=np.uint64) & _M32


def pcg_hash(v):
    v = _u32(v)
    s = (v * np.uint64(747796405) + np.uint64(2891336453)) & _M32
    w = (((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * np.uint64(277803737)) & _M32
    return ((w >> np.uint64(22)) ^ w) & _M32


def rng_stream_base(seed, stream, epoch=0):
    return pcg_hash(_u32(stream) + pcg_hash(_u32(epoch) + pcg_hash(seed)))


def rng_row_key(seed, stream, row, epoch=0):
    return pcg_hash(_u32(row) + rng_stream_base(seed, stream, epoch))


def rng_u32(row_key, col):
    return pcg_hash(_u32(col) ^ _u32(row_key))


def rng_pair(row_key, col):
    h = (((_u32(col) >> np.uint64(1)) ^ _u32(row_key)) * np.uint64(0x9E3779B1)) & _M32
    return h ^ (h >> np.uint64(15))


def rng_keep(row_key, col, thresh):
    col = _u32(col)
    h = rng_pair(row_key, col)
    half = np.where(col & np.uint64(1), h >> np.uint64(16), h & np.uint64(0xFFFF))
    return half >= np.uint64(thresh)


def drop_threshold(p):
    p = float(np.float32(p))
    if p <= 0.0:
        return 0
    t = p * 65536.0 + 0.5
    return int(min(t, 65535.0))


def drop_scale(p):
    p = np.float32(p)
    return np.float32(1.0) / (np.float32(1.0) - p) if p > 0 else np.float32(1.0)


def keep_mask(seed, stream, rows, cols, p, epoch=0):
    """bool [len(rows), len(cols)] (ints are ranges): the keep decisions of dropout at rate p.  rows / cols may be arrays of indices."""
    rows = np.arange(rows) if np.isscalar(rows) else np.asarray(rows)
    cols = np.arange(cols) if np.isscalar(cols) else np.asarray(cols)
    th = drop_threshold(p)
    if th == 0:
        return np.ones((rows.size, cols.size), bool)
    keys = rng_row_key(seed, stream, rows, epoch)[:, None]
    return rng_keep(keys, cols[None, :], th)


def drop_factor(seed, stream, rows, cols, p, epoch=0):
    """float64 [rows, cols]: 0 where dropped, the fp32 scale 1 / (1 - p) where kept -- what a kernel multiplies an element by."""
    return keep_mask(seed, stream, rows, cols, p, epoch) * float(drop_scale(p))


def row_keep(seed, stream, rows, p, epoch=0):
    """bool [rows]: rows that noise_fn (rowmask) / the embedding's noise keep."""
    return keep_mask(seed, stream, rows, [0], p, epoch)[:, 0]


def attn_keep(seed, stream, B, H, Tq, Tk, p, epoch=0):
    """bool [B, H, Tq, Tk]: attention-probability keep decisions, row (b * H + h) * Tq + q, col = key."""
    return keep_mask(seed, stream, B * H * Tq, Tk, p, epoch).reshape(B, H, Tq, Tk)
