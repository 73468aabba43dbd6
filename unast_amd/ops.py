"""Thin Python wrappers over the C ABI (include/unast_hip.h): pointer marshalling only, no arithmetic.

Every function enqueues HIP kernels on torch's current stream.  Tensors are fp32 CUDA tensors owned by torch
(device-memory plumbing); shapes are validated here and again on the C side.
"""
import os as _os

import torch

from . import config
from ._lib import lib, check

OP_KC, OP_KC_CONV, OP_RC, OP_RC_CONV_DGRAD, OP_RC_CONV_WGRAD = 0, 1, 2, 3, 4


def _p(t):
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """hipStream_t of torch's current stream on the current device (raw getter: ~0.3 us instead of ~9 us)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


_F32 = torch.float32
_LN_WS = {}


def deterministic_sums():
    """True with config.DETERMINISTIC_SUMS (utils.set_deterministic(True, fixed_sums=True), or UNAST_DETERMINISTIC_SUMS=1): every fp32 sum
    of the step is then formed in a fixed order -- the two-kernel attention backward instead of the one-pass kernel's dQ atomics, bias
    gradients by unast_colsum_det instead of the weight-gradient GEMM's row-sum atomics, unast_embed_bwd_det, ungrouped weight gradients --
    so that two runs of a step, eager or replayed, agree to the bit.  (fp64 accumulators -- BatchNorm statistics, loss sums, the gradient
    norm -- stay atomic: their order only moves bits far below fp32 resolution.)  Off by default, also in the parity mode: the golden and
    oracle tests are to pin the kernels the train step runs with."""
    return bool(config.DETERMINISTIC_SUMS)


def _f32(t, name):
    if t is None:
        return
    if not (t.is_cuda and t.dtype == torch.float32):
        raise TypeError("%s must be a float32 CUDA tensor (got %s on %s)" % (name, t.dtype, t.device))


# Flat parameter stores whose weights also exist in the pre-split operand format: (base address, bytes, split base).
_WEIGHT_SPANS = []


def register_weight_span(base_ptr, nbytes, split_ptr, transposed_lookup=None, planes_lookup=None):
    _WEIGHT_SPANS[:] = [s for s in _WEIGHT_SPANS if s[0] != base_ptr]
    _WEIGHT_SPANS.append((base_ptr, nbytes, split_ptr, transposed_lookup, planes_lookup))


def unregister_weight_span(base_ptr):
    _WEIGHT_SPANS[:] = [s for s in _WEIGHT_SPANS if s[0] != base_ptr]


def _weight_planes(W, transposed=False):
    """(hi-plane pointer, plane bytes) of the tiled bf16 planes of a stored weight view (engine.FlatStore.planes_of), or None."""
    ptr = W.data_ptr()
    for base, nbytes, split, _, lookup in _WEIGHT_SPANS:
        if lookup is not None and base <= ptr < base + nbytes:
            return lookup(W, transposed)
    return None


def _presplit_ptr(ptr):
    for base, nbytes, split, _, _p in _WEIGHT_SPANS:
        if base <= ptr < base + nbytes:
            return split + (ptr - base)
    return 0


def _transposed_weight(W):
    """(pointer, row stride) of W^T in the pre-split format if W is a stored weight that has one (engine.FlatStore.dgrad_T)."""
    ptr = W.data_ptr()
    for base, nbytes, split, lookup, _p in _WEIGHT_SPANS:
        if lookup is not None and base <= ptr < base + nbytes:
            return lookup(W)
    return None


def gemm(a_mode, b_mode, A, lda, B, ldb, C, ldc, M, N, K, conv=(0, 0, 0, 0), bias=None, R=None, ldr=0, G=None,
         ldg=0, gate_scale=1.0, alpha=1.0, beta=0, act=0, drop_p=0.0, seed=0, stream_id=0, splitk=1, nsplit=None, atomic=False, rowsum_a=None, kb_valid=0, tile_wn=0,
         b_ptr=None, out_split=False, colstats=None):
    """out_split: C is written in the pre-split operand format (for the attention kernels).  b_ptr: B given as a raw device pointer to a PRE-SPLIT operand (a transposed weight copy); `B` is then only a shape/dtype witness."""
    if A.dtype is not _F32 or B.dtype is not _F32 or C.dtype is not _F32 or not C.is_cuda:       # (epilogue operands are produced by this package)
        for t, n in ((A, "A"), (B, "B"), (C, "C"), (bias, "bias"), (R, "R"), (G, "G")):
            _f32(t, n)
    ws, ws_n = None, 0
    if splitk > 1 and not atomic:
        ws_n = splitk * M * ((N + 3) // 4 * 4)
        ws = torch.empty(ws_n, dtype=torch.float32, device=C.device)          # split-K partial slabs (caching allocator)
    bp, presplit = _p(B), 0
    if b_ptr is not None:
        bp, presplit = b_ptr, 1
    elif _WEIGHT_SPANS and a_mode != OP_RC:      # forward / dgrad forms: B may be a stored weight
        sp = _presplit_ptr(bp)
        if sp:
            bp, presplit = sp, 1
    check(lib().unast_gemm(a_mode, b_mode, nsplit or config.NSPLIT, _p(A), lda, bp, ldb, _p(C), ldc, M, N, K, kb_valid,
                           conv[0], conv[1], conv[2], conv[3], _p(bias), _p(R), ldr, _p(G), ldg, gate_scale,
                           alpha, beta, act, drop_p, seed & 0xFFFFFFFF, stream_id, splitk, _p(ws), ws_n, _p(rowsum_a), tile_wn, presplit,
                           int(out_split), _p(colstats), _stream()), "unast_gemm")


SPLITK_TARGET_BLOCKS = 256      # one workgroup per CU: 36.4 vs 36.8 ms/step at 320 (same box)
SPLITK_MIN_KSTEPS = 10


def _splitk_for(M, N, K):
    """Split the long token reduction of a weight gradient so that ~SPLITK_TARGET_BLOCKS workgroups are in flight, each
    with at least SPLITK_MIN_KSTEPS 32-deep k-steps."""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    ksteps = (K + 31) // 32
    # every split writes and re-reads an [M,N] slab: for a small gradient (<= 4 tiles) one workgroup per CU is the optimum, a
    # larger one amortises the slabs over more operand bytes and gains from two per CU (round-1 tools/bench_wgrad.py: 768x256 over
    # 25600 tokens 76 -> 57 us at 42 instead of 21 splits; 256x256 39.7 us at 64 splits, 53.7 at 128)
    target = SPLITK_TARGET_BLOCKS * (2 if tiles >= 8 else 1)
    want = max(1, target // tiles)
    return max(1, min(want, ksteps // SPLITK_MIN_KSTEPS))


def _panel_ok(M, K, *tensors, N=None):
    if not (config.NSPLIT == 3 and M >= config.PANEL_MIN_ROWS and K >= 4 and K % 4 == 0):
        return False
    if K > 256 and not (K % 64 == 0 and N is not None and N % 256 == 0):      # the K-streamed form: 256-column output tiles
        return False
    for t in tensors:
        if t is not None and (t.stride(-1) != 1 or t.data_ptr() % 16 or t.stride(0) % 4):
            return False
        if t is not None and (M + 127) // 128 * 128 * t.stride(0) * 4 >= 0x7FFFFFF0:      # 32-bit buffer offsets (unast_panel_gemm refuses it too)
            return False
    return True


def linear_fwd(x2d, W, bias, out, act=0, drop_p=0.0, seed=0, stream_id=0, R=None, out_split=False, ln=None, gate_bits=None):
    """out[M,N] = epi(x2d[M,K] @ W[N,K]^T + bias).  ln = (gamma, beta, y, mean, rstd, eps): LayerNorm of `out` fused behind the GEMM when
    the row-panel kernel serves the shape (returns True), a separate launch otherwise.  gate_bits: uint8 buffer that receives one
    keep bit per output element (panel kernel only; see linear_dgrad)."""
    M, K = x2d.shape
    N = W.shape[0]
    fuse_ln = ln is not None and N == 256 and not out_split and act == 0
    deep = K > 256                                  # K-streamed form: plain / residual / LayerNorm epilogues (dropout inside the LayerNorm one only)
    if _panel_ok(M, K, x2d, out, R, N=N) and W.stride(1) == 1 and (R is None or fuse_ln or deep) and \
            not (deep and (act or out_split or gate_bits is not None or (drop_p > 0 and not fuse_ln))):       # (K <= 256: a residual operand is served by the LayerNorm epilogue only)
        wp = _weight_planes(W)
        if wp is not None:
            panel_gemm(x2d, wp, out, N, bias=bias, R=R, act=act, drop_p=drop_p, seed=seed, stream_id=stream_id, out_split=out_split,
                       ln=ln if fuse_ln else None, rows_per_wg=config.PANEL_ROWS, gate_bits=gate_bits)
            if ln is not None and not fuse_ln:
                layernorm_fwd(out, ln[0], ln[1], ln[2], ln[3], ln[4], ln[5])
            return out
    if gate_bits is not None:
        raise RuntimeError("linear_fwd: gate_bits needs the row-panel kernel (check ops.panel_serves first)")
    gemm(OP_KC, OP_KC, x2d, x2d.stride(0), W, W.stride(0), out, out.stride(0), M, N, K, bias=bias, act=act,
         drop_p=drop_p, seed=seed, stream_id=stream_id, R=R, ldr=(R.stride(0) if R is not None else 0), out_split=out_split)
    if ln is not None:
        layernorm_fwd(out, ln[0], ln[1], ln[2], ln[3], ln[4], ln[5])
    return out


def gate_bits_bytes(M, N):
    """Bytes of the keep-bit buffer of an [M, N] activation (unast_panel_gemm gate_bits): whole 128-row panels, one bit per element."""
    return (M + 127) // 128 * 128 * ((N + 15) // 16 * 16) // 8


def panel_serves(M, K, W, transposed=False):
    """True when linear_fwd (transposed=False) / linear_dgrad (True) of this shape and stored weight run on the row-panel kernel."""
    return _panel_ok(M, K, N=(W.shape[1] if transposed else W.shape[0])) and W.stride(1) == 1 and _weight_planes(W, transposed) is not None


def linear_dgrad(dy2d, W, dx, R=None, G=None, gate_scale=1.0, beta=0, out_split=False, gate_bits=None):
    """dx[M,K] = (dy2d[M,N] @ W[N,K]) gated by G>0, + R.  gate_bits: the keep bits linear_fwd(..., gate_bits=) wrote for the [M,K]
    activation that G would be (panel kernel only): the gate is read from them with scalar loads instead of from G."""
    M, N = dy2d.shape
    K = W.shape[1]
    deep = N > 256                                  # K-streamed form (contraction over N): residual operand allowed, no gate, no split output
    if N % 4 == 0 and G is None and _panel_ok(M, N, dy2d, dx, R, N=K) and beta == 0 and W.stride(1) == 1 and \
            (R is None if not deep else (gate_bits is None and not out_split)):
        wp = _weight_planes(W, transposed=True)                # dX[M,K] = dY[M,N] (W^T)[K,N]^T: W^T planes, contraction over N
        if wp is not None:
            panel_gemm(dy2d, wp, dx, K, R=R, gate_scale=gate_scale, out_split=out_split, rows_per_wg=config.PANEL_ROWS, gate_bits=gate_bits)
            return dx
    if gate_bits is not None:
        raise RuntimeError("linear_dgrad: gate_bits needs the row-panel kernel (check ops.panel_serves first)")
    Np = (N + 3) // 4 * 4          # dy2d is a view of a zero-padded buffer when N % 4 != 0 (logits 46->48, head 81->84, fc2 1->4)
    if Np != N and dy2d.stride(0) < Np:
        raise ValueError("linear_dgrad: dy must live in a zero-padded buffer with row stride >= %d" % Np)
    wt = _transposed_weight(W) if config.DGRAD_TRANSPOSED else None
    if wt is not None:             # dX = dY (W^T)^T with W^T stored pre-split and K-contiguous: the forward GEMM's operand form
        gemm(OP_KC, OP_KC, dy2d, dy2d.stride(0), W, wt[1], dx, dx.stride(0), M, K, Np, R=R,
             ldr=(R.stride(0) if R is not None else 0), G=G, ldg=(G.stride(0) if G is not None else 0),
             gate_scale=gate_scale, beta=beta, b_ptr=wt[0], out_split=out_split)
        return dx
    gemm(OP_KC, OP_RC, dy2d, dy2d.stride(0), W, W.stride(0), dx, dx.stride(0), M, K, Np, R=R,
         ldr=(R.stride(0) if R is not None else 0), G=G, ldg=(G.stride(0) if G is not None else 0),
         gate_scale=gate_scale, beta=beta, kb_valid=N, out_split=out_split)
    return dx


LNBWD_FUSED = [0]         # launches of the fused form below (tests look at it)


def linear_dgrad_lnbwd(dy2d, W, R, z, mean, rstd, gamma, dz, dz_drop, dgamma, dbeta, drop_p=0.0, seed=0, stream_id=0):
    """The input-gradient GEMM that ends a sub-layer's backward together with the PREVIOUS sub-layer's LayerNorm backward:
    dz = LNbwd(R + dy2d @ W; z, mean, rstd, gamma), dz_drop = dropout(dz), dgamma / dbeta += column sums -- one launch of the K-streamed
    row-panel kernel (csrc/panel.hip kpanel_kernel<2>) instead of linear_dgrad + layernorm_bwd.  Returns False (and does nothing) when the
    kernel does not serve the shape: contraction dy2d.shape[1] > 256 and a multiple of 64, 256 output columns, at least
    config.PANEL_MIN_ROWS rows, tiled planes of W^T, 16-byte operands."""
    M, N = dy2d.shape
    if not (W.shape[1] == 256 and N > 256 and W.stride(1) == 1 and z.shape[1] == 256 and
            _panel_ok(M, N, dy2d, dz, R, z, dz_drop, N=256) and gamma.data_ptr() % 16 == 0):
        return False
    wp = _weight_planes(W, transposed=True)
    if wp is None:
        return False
    part, part_n = None, 0
    if dgamma is not None:
        part_n = lib().unast_panel_gemm_lnbwd_ws_floats(M)
        part = torch.empty(part_n, dtype=torch.float32, device=dy2d.device)
    PANEL_LAUNCHES[1] += 1
    LNBWD_FUSED[0] += 1
    check(lib().unast_panel_gemm_lnbwd(_p(dy2d), dy2d.stride(0), wp[0], wp[1], M, N, _p(R), R.stride(0) if R is not None else 0,
                                       _p(z), z.stride(0), _p(mean), _p(rstd), _p(gamma), _p(dz), dz.stride(0),
                                       _p(dz_drop), dz_drop.stride(0) if dz_drop is not None else 0, _p(part), part_n,
                                       drop_p if dz_drop is not None else 0.0, seed & 0xFFFFFFFF, stream_id, _stream()), "unast_panel_gemm_lnbwd")
    if dgamma is not None:      # the reduction of the parameter-gradient partials is off the backward chain: companion stream
        nblk = (M + 127) // 128
        _on_wgrad_stream(lambda: check(lib().unast_layernorm_partials_finalize(_p(part), nblk, 256, _p(dgamma), _p(dbeta), _stream()),
                                       "unast_layernorm_partials_finalize"), M, dgamma.data_ptr(), part)
    return True


# Set by engine.side_streams: returns the companion stream for weight gradients issued from the current stream, or None.
WGRAD_SIDE = None


# Stream choice per gradient buffer for the current optimizer phase (address of dW -> offloaded?).  The first weight-gradient
# launch into a buffer decides, later ones follow: the token count of a weight's gradient may differ between sub-steps (other
# batch, other memory length) and may straddle the gate, but its accumulations must all be ordered on ONE stream (defensive: the
# sub-step joins also wait for the companion streams).  Cleared by FlatStore.zero_grad.
_WGRAD_CHOICE = {}


def reset_wgrad_choices():
    _WGRAD_CHOICE.clear()


def _on_wgrad_stream(launch, tokens, key, *operands):
    """Runs `launch()` on the weight-gradient companion stream of the current stream (if any): that stream first waits for
    everything enqueued so far on the current one (the producers of dy / x), the operands are handed to the caching allocator
    with record_stream, and nobody waits for the result until the optimizer joins the streams.  All weight / bias gradient
    updates of a module come through here, so their read-modify-writes stay ordered on one stream."""
    w = WGRAD_SIDE() if WGRAD_SIDE is not None else None
    if w is not None:
        off = _WGRAD_CHOICE.get(key)
        if off is None:
            off = _WGRAD_CHOICE[key] = tokens >= config.WGRAD_STREAM_MIN_TOKENS
        if not off:
            w = None
    if w is None:
        return launch()
    from . import engine
    engine.wait(w, torch.cuda.current_stream())
    for t in operands:
        if t is not None:
            t.record_stream(w)
    with torch.cuda.stream(w):
        jitter()
        return launch()


def _linear_wgrad_now(dy2d, x2d, dW, db=None):
    M, N = dy2d.shape
    K = x2d.shape[1]
    sk = _splitk_for(N, K, M)
    if db is not None and deterministic_sums():          # the bias gradient in a fixed order, behind the weight gradient on its stream
        def both():
            gemm(OP_RC, OP_RC, dy2d, dy2d.stride(0), x2d, x2d.stride(0), dW, dW.stride(0), N, K, M, beta=1, splitk=sk)
            colsum(dy2d, db)
        _on_wgrad_stream(both, M, dW.data_ptr(), dy2d, x2d)
        return dW
    _on_wgrad_stream(lambda: gemm(OP_RC, OP_RC, dy2d, dy2d.stride(0), x2d, x2d.stride(0), dW, dW.stride(0), N, K, M, beta=1, splitk=sk,
                                  rowsum_a=db), M, dW.data_ptr(), dy2d, x2d)
    return dW


import ctypes as _ct


class _WgradItem(_ct.Structure):          # include/unast_hip.h: unast_wgrad_item
    _fields_ = [("A", _ct.c_void_p), ("lda", _ct.c_int), ("B", _ct.c_void_p), ("ldb", _ct.c_int), ("C", _ct.c_void_p), ("ldc", _ct.c_int),
                ("rowsum_a", _ct.c_void_p), ("M", _ct.c_int), ("N", _ct.c_int), ("K", _ct.c_int)]


_BATCH = None            # list of pending (dy2d, x2d, dW, db) while inside `wgrad_batch()`
GROUP_MAX = 8
WGRAD_GROUP_TARGET = 256      # workgroups per grouped launch: 29.42 vs 29.65 ms/step at 512 (three alternating runs each, same box; round 2 preferred 512 when one stream bounded the step)


class wgrad_batch:
    """While active, eligible weight gradients (linear_wgrad) are collected and issued as ONE grouped launch at exit
    (unast_wgrad_group): the operands of a backward closure stay alive until it returns, and nobody reads a weight gradient
    before the optimizer, so deferring them to the closure's end changes no result."""

    def __enter__(self):
        global _BATCH
        self.outer = _BATCH is not None
        if not self.outer and config.WGRAD_GROUP:
            _BATCH = []
        return self

    def __exit__(self, *exc):
        global _BATCH
        if self.outer or _BATCH is None:
            return
        items, _BATCH = _BATCH, None
        if exc[0] is None:
            _flush_wgrads(items)


def _groupable(dy2d, x2d, dW, db):
    M, N = dy2d.shape
    K = x2d.shape[1]
    return (N % 128 == 0 and K % 128 == 0 and M % 32 == 0 and dy2d.stride(1) == 1 and x2d.stride(1) == 1 and dW.stride(1) == 1
            and dy2d.stride(0) % 4 == 0 and x2d.stride(0) % 4 == 0 and dW.stride(0) % 4 == 0
            and (dy2d.data_ptr() | x2d.data_ptr() | dW.data_ptr()) % 16 == 0 and M * max(dy2d.stride(0), x2d.stride(0)) < (1 << 29))


def _flush_wgrads(items):
    # the stream choice is per gradient buffer (see _WGRAD_CHOICE): problems bound for the companion stream form one group, the rest another
    w_side = WGRAD_SIDE() if WGRAD_SIDE is not None else None
    groups = {}
    for it in items:
        dy2d, x2d, dW, db = it
        key = dW.data_ptr()
        off = False
        if w_side is not None:
            off = _WGRAD_CHOICE.get(key)
            if off is None:
                off = _WGRAD_CHOICE[key] = dy2d.shape[0] >= config.WGRAD_STREAM_MIN_TOKENS
        groups.setdefault(bool(off), []).append(it)
    for off, its in groups.items():
        for i in range(0, len(its), GROUP_MAX):
            chunk = its[i:i + GROUP_MAX]
            if deterministic_sums():                       # (the grouped kernel takes the bias gradients by atomics)
                for it in chunk:
                    _linear_wgrad_now(*it)
            elif len(chunk) == 1:
                _linear_wgrad_now(*chunk[0])
            else:
                _launch_group(chunk, off)


def _launch_group(chunk, offload):
    n = len(chunk)
    arr = (_WgradItem * n)()
    operands = []
    for j, (dy2d, x2d, dW, db) in enumerate(chunk):
        a = arr[j]
        a.A, a.lda, a.B, a.ldb, a.C, a.ldc = dy2d.data_ptr(), dy2d.stride(0), x2d.data_ptr(), x2d.stride(0), dW.data_ptr(), dW.stride(0)
        a.rowsum_a = db.data_ptr() if db is not None else None
        a.M, a.N, a.K = dy2d.shape[1], x2d.shape[1], dy2d.shape[0]
        operands += [dy2d, x2d]
    ptr = _ct.addressof(arr)              # `arr` stays referenced by the closure below until the launch has been issued
    ws_n = lib().unast_wgrad_group_ws_floats(n, ptr, WGRAD_GROUP_TARGET)
    if ws_n <= 0:
        raise RuntimeError("unast_wgrad_group_ws_floats failed")

    shapes = tuple((int(a.M), int(a.N), int(a.K), int(a.rowsum_a is not None)) for a in arr)

    def launch():
        import sys
        sys.modules[__name__].wgrad_group(shapes, n, ptr, ws_n, chunk[0][0].device)       # looked up at call time: bench.py wraps it with HIP events
    if offload:
        w = WGRAD_SIDE()
        from . import engine
        engine.wait(w, torch.cuda.current_stream())
        for t in operands:
            t.record_stream(w)
        with torch.cuda.stream(w):
            launch()
    else:
        launch()


def wgrad_group(shapes, n, items_ptr, ws_n, device):
    """The grouped launch itself (GEMM + reduction on the current stream); `shapes` = ((out, in, tokens, has_bias), ...) for bookkeeping."""
    ws = torch.empty(ws_n, dtype=torch.float32, device=device)
    check(lib().unast_wgrad_group(config.NSPLIT, n, items_ptr, _p(ws), ws_n, WGRAD_GROUP_TARGET, _stream()), "unast_wgrad_group")


def linear_wgrad(dy2d, x2d, dW, db=None):
    """dW[N,K] += dy2d[M,N]^T @ x2d[M,K]; optionally db[N] += sum_rows dy2d (fused).  Always accumulates.  Inside
    `wgrad_batch()` eligible problems are deferred to the batch's grouped launch."""
    if _BATCH is not None and _groupable(dy2d, x2d, dW, db):
        _BATCH.append((dy2d, x2d, dW, db))
        return dW
    return _linear_wgrad_now(dy2d, x2d, dW, db)


_PANEL_TRACE = _os.environ.get("UNAST_PANEL_TRACE", "0") == "1"       # debugging: print and synchronise every row-panel launch


def retile_weights(src_flat, dst_bytes, descs_dev, ndesc):
    """Tiled bf16 planes (unast_amd.planes) of the matrices the descriptors name, from the fp32 buffer `src_flat`."""
    check(lib().unast_retile_weights(_p(src_flat), _p(dst_bytes), _p(descs_dev), ndesc, _stream()), "unast_retile_weights")


PANEL_LAUNCHES = [0, 0]          # (activation-stationary, K-streamed) launches so far: tests assert which kernel served them


def panel_gemm(A, wplanes, C, N, bias=None, R=None, G=None, gate_scale=1.0, act=0, drop_p=0.0, seed=0, stream_id=0, out_split=False,
               ln=None, rows_per_wg=0, K=None, gate_bits=None):
    """C[M,N] = epi(A[M,K] W[N,K]^T) with W given as tiled planes `wplanes` = (hi-plane pointer, plane bytes).
    ln = (gamma, beta, Y, mean, rstd, eps): LayerNorm epilogue (N = 256): C receives the pre-norm sum z, Y the normalised rows."""
    M = A.shape[0]
    K = A.shape[1] if K is None else K
    g = b = Y = mean = rstd = None
    eps, ldy = 0.0, 0
    if ln is not None:
        g, b, Y, mean, rstd, eps = ln
        ldy = Y.stride(0)
    PANEL_LAUNCHES[0 if K <= 256 else 1] += 1
    if _PANEL_TRACE:
        print("panel_gemm M=%d N=%d K=%d lda=%d ldc=%d bias=%s R=%s G=%s act=%d drop=%.2f split=%d ln=%s bits=%s rows=%d" % (
            M, N, K, A.stride(0), C.stride(0), bias is not None, R is not None, G is not None, act, drop_p, out_split, ln is not None,
            None if gate_bits is None else gate_bits.numel(), rows_per_wg), flush=True)
    check(lib().unast_panel_gemm(_p(A), A.stride(0), wplanes[0], wplanes[1], _p(C), C.stride(0), M, N, K, _p(bias), _p(R),
                                 R.stride(0) if R is not None else 0, _p(G), G.stride(0) if G is not None else 0, gate_scale, act,
                                 drop_p, seed & 0xFFFFFFFF, stream_id, int(out_split), _p(g), _p(b), _p(Y), ldy, _p(mean), _p(rstd), eps,
                                 _p(gate_bits), rows_per_wg, _stream()), "unast_panel_gemm")
    if _PANEL_TRACE:
        torch.cuda.synchronize()
    return C


def conv_fwd(x3d, Wp, bias, out, pad_left, colstats=None):
    """x3d [B,T,Cin], Wp [Cout,5,Cin] (tap-major physical layout), out [B,T,Cout].  colstats: float64 [2*Cout], zeroed by the
    caller, receives the per-channel sum and sum of squares of `out` (the batch statistics of the BatchNorm that follows)."""
    B, T, Cin = x3d.shape
    Cout = Wp.shape[0]
    gemm(OP_KC_CONV, OP_KC, x3d, x3d.stride(1), Wp, 5 * Cin, out, out.stride(1), B * T, Cout, 5 * Cin,
         conv=(T, Cin, 0, pad_left), bias=bias, colstats=colstats)
    return out


def conv_dgrad(dy3d, Wp, dx, pad_left, beta=0):
    B, T, Cout = dy3d.shape
    Cin = Wp.shape[2]
    gemm(OP_KC_CONV, OP_RC_CONV_DGRAD, dy3d, dy3d.stride(1), Wp, 4, dx, dx.stride(1), B * T, Cin, 5 * Cout,
         conv=(T, Cout, Cout, 4 - pad_left), beta=beta)
    return dx


def conv_wgrad(dy3d, x3d, dWp, pad_left, db=None):
    """dWp[Cout,5,Cin] += sum_t dy[t,o] x[t+j-pad_left,c]; optionally db[Cout] += sum_t dy (fused)."""
    B, T, Cout = dy3d.shape
    Cin = x3d.shape[2]
    sk = _splitk_for(Cout, 5 * Cin, B * T)
    if db is not None and deterministic_sums() and dy3d.is_contiguous():
        def both():
            gemm(OP_RC, OP_RC_CONV_WGRAD, dy3d, dy3d.stride(1), x3d, x3d.stride(1), dWp, 5 * Cin, Cout, 5 * Cin, B * T,
                 conv=(T, 0, Cin, pad_left), beta=1, splitk=sk)
            colsum(dy3d.view(B * T, Cout), db)
        _on_wgrad_stream(both, B * T, dWp.data_ptr(), dy3d, x3d)
        return dWp
    _on_wgrad_stream(lambda: gemm(OP_RC, OP_RC_CONV_WGRAD, dy3d, dy3d.stride(1), x3d, x3d.stride(1), dWp, 5 * Cin, Cout, 5 * Cin, B * T,
                                  conv=(T, 0, Cin, pad_left), beta=1, splitk=sk, rowsum_a=db), B * T, dWp.data_ptr(), dy3d, x3d)
    return dWp


# ---- attention ---------------------------------------------------------------------------------------------
def attn_fwd(Q, K, V, O, LSE, lens_k, B, H, Tq, Tk, causal, drop_p=0.0, seed=0, stream_id=0, nsplit=None, qkv_split=False):
    """Q/K/V/O are 2-D views [B*T, >=H*64] (column slices of projection outputs are fine)."""
    check(lib().unast_attn_fwd(nsplit or config.NSPLIT, _p(Q), Q.stride(0), _p(K), K.stride(0), _p(V), V.stride(0), _p(O), O.stride(0),
                               _p(LSE), _p(lens_k), B, H, Tq, Tk, 64, int(causal), 0.125, drop_p, seed & 0xFFFFFFFF, stream_id,
                               int(qkv_split), _stream()), "unast_attn_fwd")


def attn_bwd(Q, K, V, O, dO, LSE, delta_ws, dQ, dK, dV, lens_k, B, H, Tq, Tk, causal, drop_p=0.0, seed=0, stream_id=0, nsplit=None, qkv_split=False, lens_q=None):
    """lens_q (int32 [B], one-pass backward only): queries t >= lens_q[b] have a zero dO by the caller's guarantee; their tiles are skipped."""
    fused = config.ATTN_FUSED_BWD and not deterministic_sums()          # (the one-pass kernel adds dQ with fp32 atomics)
    check(lib().unast_attn_bwd(nsplit or config.NSPLIT, _p(Q), Q.stride(0), _p(K), K.stride(0), _p(V), V.stride(0), _p(O), O.stride(0),
                               _p(dO), dO.stride(0), _p(LSE), _p(delta_ws), _p(dQ), dQ.stride(0), _p(dK), dK.stride(0), _p(dV),
                               dV.stride(0), _p(lens_k), B, H, Tq, Tk, 64, int(causal), 0.125, drop_p, seed & 0xFFFFFFFF, stream_id,
                               (2 if config.ATTN_BWD_TERMS == 2 else 1) if fused else 0, int(qkv_split),
                               _p(lens_q) if fused else None, _stream()), "unast_attn_bwd")


# ---- normalisation -----------------------------------------------------------------------------------------
def layernorm_fwd(z, gamma, beta, y, mean, rstd, eps=1e-5):
    rows, C = z.shape
    check(lib().unast_layernorm_fwd(_p(z), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, C, eps, _stream()), "unast_layernorm_fwd")


def layernorm_bwd(dy, z, gamma, mean, rstd, dz, dz_drop=None, dgamma=None, dbeta=None, drop_p=0.0, seed=0, stream_id=0):
    rows, C = z.shape
    ws, ws_n = None, 0
    if dgamma is not None:
        ws_n = _LN_WS.get((rows, C))
        if ws_n is None:
            ws_n = _LN_WS[(rows, C)] = lib().unast_layernorm_bwd_ws_floats(rows, C)
        ws = torch.empty(ws_n, dtype=torch.float32, device=z.device)
    check(lib().unast_layernorm_bwd(_p(dy), _p(z), _p(gamma), _p(mean), _p(rstd), _p(dz), _p(dz_drop), _p(dgamma), _p(dbeta), _p(ws), ws_n,
                                    rows, C, drop_p, seed & 0xFFFFFFFF, stream_id, 0 if dgamma is not None else 1, _stream()), "unast_layernorm_bwd")
    if dgamma is not None:      # the reduction of the parameter-gradient partials is off the backward chain: companion stream
        _on_wgrad_stream(lambda: check(lib().unast_layernorm_bwd_finalize(_p(ws), ws_n, rows, C, _p(dgamma), _p(dbeta), _stream()),
                                       "unast_layernorm_bwd_finalize"), rows, dgamma.data_ptr(), ws)


def colsum(x2d, out):
    rows, C = x2d.shape
    if deterministic_sums():
        ws_n = lib().unast_colsum_det_ws_floats(rows, C)
        ws = torch.empty(ws_n, dtype=torch.float32, device=x2d.device)
        check(lib().unast_colsum_det(_p(x2d), x2d.stride(0), rows, C, _p(out), _p(ws), ws_n, _stream()), "unast_colsum_det")
        return
    check(lib().unast_colsum_f32(_p(x2d), x2d.stride(0), rows, C, _p(out), _stream()), "unast_colsum_f32")


def bn_fwd(x2d, gamma, beta, y, mean, rstd, running_mean, running_var, ws, act, drop_p=0.0, seed=0, stream_id=0, eps=1e-5, momentum=0.1, have_sums=False,
           num_batches_tracked=None):
    rows, C = x2d.shape
    check(lib().unast_bn_fwd(_p(x2d), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), _p(running_mean), _p(running_var), _p(ws), rows, C,
                             eps, momentum, act, drop_p, seed & 0xFFFFFFFF, stream_id, int(have_sums), _p(num_batches_tracked), _stream()), "unast_bn_fwd")


def bn_eval_fwd(x2d, gamma, beta, running_mean, running_var, y, mean, rstd, act, eps=1e-5):
    rows, C = x2d.shape
    check(lib().unast_bn_eval_fwd(_p(x2d), _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(y), _p(mean), _p(rstd), rows, C,
                                  eps, act, _stream()), "unast_bn_eval_fwd")


def bn_bwd(dy_inout, x2d, mean, rstd, gamma, beta, dx, dgamma, dbeta, ws, act, drop_p=0.0, seed=0, stream_id=0, ws_zeroed=False):
    rows, C = x2d.shape
    check(lib().unast_bn_bwd(_p(dy_inout), _p(x2d), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dx), _p(dgamma), _p(dbeta), _p(ws), rows, C,
                             act, drop_p, seed & 0xFFFFFFFF, stream_id, int(ws_zeroed), _stream()), "unast_bn_bwd")


# ---- embedding / positional encoding / masks ---------------------------------------------------------------
def embed_fwd(ids, E, out, T, shift_sos=-1, drop_p=0.0, seed=0, stream_id=0, noise_p=0.0, noise_stream=0):
    rows = ids.numel()
    check(lib().unast_embed_fwd(_p(ids), _p(E), _p(out), rows, T, E.shape[1], shift_sos, drop_p, seed & 0xFFFFFFFF, stream_id, noise_p,
                                noise_stream, _stream()), "unast_embed_fwd")


def embed_bwd(ids, dout, dE, T, shift_sos=-1, drop_p=0.0, seed=0, stream_id=0, noise_p=0.0, noise_stream=0, padding_idx=0):
    rows = ids.numel()
    fn = lib().unast_embed_bwd_det if deterministic_sums() else lib().unast_embed_bwd
    check(fn(_p(ids), _p(dout), _p(dE), rows, T, dE.shape[1], dE.shape[0], shift_sos, padding_idx, drop_p,
             seed & 0xFFFFFFFF, stream_id, noise_p, noise_stream, _stream()), "unast_embed_bwd")


# ---- the prefix slab of TextRNN's decoder training (csrc/prefix.hip); `lay` = unast_amd.train_rnn.prefix_tables(B, T, device) ---------------
def prefix_bn_ws(lay, C, dev):
    return torch.empty((lay.nchunks + lay.T) * 2 * C, dtype=torch.float64, device=dev)


def prefix_bn_fwd(x2d, lay, gamma, beta, mean, rstd, varu, ws, y=None, p_last=None, running_mean=None, running_var=None, num_batches_tracked=None,
                  eps=1e-5, momentum=0.1, drop_p=0.0, seed=0, stream_id=0):
    rows, C = x2d.shape
    if rows != lay.rows or not x2d.is_contiguous() or tuple(mean.shape) != (lay.T, C) or tuple(rstd.shape) != (lay.T, C) or tuple(varu.shape) != (lay.T, C):
        raise ValueError("prefix_bn_fwd: x [slab rows, C] contiguous, mean / rstd / varu [T, C]")
    if (y is not None and tuple(y.shape) != (rows, C)) or (p_last is not None and tuple(p_last.shape) != (lay.B, lay.T, C)) or ws.numel() < lay.nchunks * 2 * C:
        raise ValueError("prefix_bn_fwd: y [slab rows, C] or p_last [B, T, C]; ws of nchunks*2*C doubles")
    for t, n in ((x2d, "x"), (y, "y"), (p_last, "p_last"), (mean, "mean"), (rstd, "rstd"), (varu, "varu"), (gamma, "gamma"), (beta, "beta")):
        _f32(t, n)
    check(lib().unast_prefix_bn_fwd(_p(x2d), _p(lay.chunks), _p(lay.chunk_start), _p(lay.segoff), lay.nchunks, lay.rows, lay.B, lay.T, C, _p(gamma), _p(beta),
                                    _p(y), _p(p_last), _p(mean), _p(rstd), _p(varu), _p(running_mean), _p(running_var), _p(num_batches_tracked), _p(ws),
                                    eps, momentum, drop_p, seed & 0xFFFFFFFF, stream_id, _stream()), "unast_prefix_bn_fwd")


def prefix_bn_bwd(dy, x2d, lay, mean, rstd, gamma, beta, dz, dgamma, dbeta, ws, last_only=False, drop_p=0.0, seed=0, stream_id=0):
    rows, C = x2d.shape
    want = (lay.B, lay.T, C) if last_only else (rows, C)
    if rows != lay.rows or tuple(dy.shape) != want or tuple(dz.shape) != (rows, C) or not (dy.is_contiguous() and x2d.is_contiguous() and dz.is_contiguous()):
        raise ValueError("prefix_bn_bwd: x, dz [slab rows, C], dy [slab rows, C] or (last_only) [B, T, C], contiguous")
    if ws.numel() < (lay.nchunks + lay.T) * 2 * C or tuple(mean.shape) != (lay.T, C) or tuple(rstd.shape) != (lay.T, C):
        raise ValueError("prefix_bn_bwd: ws of (nchunks + T)*2*C doubles, mean / rstd [T, C]")
    for t, n in ((x2d, "x"), (dy, "dy"), (dz, "dz"), (mean, "mean"), (rstd, "rstd"), (dgamma, "dgamma"), (dbeta, "dbeta")):
        _f32(t, n)
    check(lib().unast_prefix_bn_bwd(_p(dy), int(last_only), _p(x2d), _p(lay.chunks), _p(lay.chunk_start), _p(lay.segoff), lay.nchunks, lay.rows, lay.B, lay.T, C,
                                    _p(mean), _p(rstd), _p(gamma), _p(beta), _p(dz), _p(dgamma), _p(dbeta), _p(ws), drop_p, seed & 0xFFFFFFFF, stream_id,
                                    _stream()), "unast_prefix_bn_bwd")


def prefix_embed_fwd(target, E, lay, out, sos, drop_p=0.0, seed=0, stream_id=0):
    if tuple(target.shape) != (lay.B, lay.T) or target.dtype is not torch.int64 or not target.is_contiguous() or tuple(out.shape) != (lay.rows, E.shape[1]):
        raise ValueError("prefix_embed_fwd: target int64 [B, T] contiguous, out [slab rows, D]")
    _f32(E, "E")
    _f32(out, "out")
    check(lib().unast_prefix_embed_fwd(_p(target), _p(E), _p(lay.chunks), _p(lay.segoff), lay.nchunks, lay.rows, lay.B, lay.T, E.shape[1], E.shape[0], sos,
                                       _p(out), drop_p, seed & 0xFFFFFFFF, stream_id, _stream()), "unast_prefix_embed_fwd")


def prefix_embed_bwd(dx, lay, G, drop_p=0.0, seed=0, stream_id=0):
    D = dx.shape[1]
    if tuple(dx.shape) != (lay.rows, D) or tuple(G.shape) != (lay.B, lay.T + 1, D) or not (dx.is_contiguous() and G.is_contiguous()):
        raise ValueError("prefix_embed_bwd: dx [slab rows, D], G [B, T+1, D], contiguous")
    _f32(dx, "dx")
    _f32(G, "G")
    check(lib().unast_prefix_embed_bwd(_p(dx), _p(lay.segoff), lay.rows, lay.B, lay.T, D, _p(G), drop_p, seed & 0xFFFFFFFF, stream_id, _stream()),
          "unast_prefix_embed_bwd")


# ---- the single-prefix prenet and the position ends of train-mode generation (csrc/prefix_gen.hip) ----------------------------------------------
def prefix_gen_tiles(B, L):
    return lib().unast_prefix_gen_tiles(B, L)


def _pgen_rows(name, B, L, *named):
    if B < 2 or L < 1:
        raise ValueError("%s: 2 <= B, 1 <= L (got B = %d, L = %d)" % (name, B, L))
    for t, n, cols in named:
        _f32(t, n)
        if t.dim() != 2 or t.shape[0] < B * L or t.shape[1] != cols or not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous [>= B*L = %d, %d] (got %s)" % (name, n, B * L, cols, tuple(t.shape)))


def _pgen_part(name, part, tiles, lead=()):
    if not (part.is_cuda and part.dtype is torch.float64 and part.is_contiguous() and part.dim() == len(lead) + 3 and tuple(part.shape[:len(lead)]) == lead and
            part.shape[len(lead)] >= tiles and tuple(part.shape[len(lead) + 1:]) == (2, 256)):
        raise ValueError("%s: partial sums must be contiguous float64 %s[>= %d tiles, 2, 256] (got %s)" % (name, list(lead), tiles, tuple(part.shape)))


def prefix_gen_conv(Wp, bias, z, part_out, B, L, x=None, part_in=None, bn=None, tokens=None, emb=None, sos=0, drop_p=0.0, seed=0, stream_id=0, row0=0):
    """One prenet stage over the prefix [B, L]: z[:B*L] [.,256] = conv5(input) + bias, part_out [tiles,2,256] its column sums.  Wp [256,5,Cin]
    tap-major.  Stage 1: tokens int64 [B, ld] (the generated tokens; SOS is implied at row 0) and emb [V,Cin]; stages 2, 3: x = the previous
    stage's z, part_in its sums, bn = (gamma, beta, eps).  The dropout (on the input rows) draws row row0 + b*L + j."""
    tiles = prefix_gen_tiles(B, L)
    _pgen_rows("prefix_gen_conv", B, L, (z, "z", 256))
    _pgen_part("prefix_gen_conv", part_out, tiles)
    _f32(Wp, "Wp"), _f32(bias, "bias")
    if Wp.dim() != 3 or Wp.shape[0] != 256 or Wp.shape[1] != 5 or not Wp.is_contiguous() or bias.numel() != 256:
        raise ValueError("prefix_gen_conv: Wp contiguous [256,5,Cin], bias [256]")
    Cin = Wp.shape[2]
    if (x is None) == (tokens is None):
        raise ValueError("prefix_gen_conv: give x, part_in and bn (stages 2, 3) or tokens and emb (stage 1)")
    if x is not None:
        _pgen_rows("prefix_gen_conv", B, L, (x, "x", 256))
        _pgen_part("prefix_gen_conv", part_in, tiles)
        gamma, beta, eps = bn
        _f32(gamma, "gamma"), _f32(beta, "beta")
        if Cin != 256 or gamma.numel() != 256 or beta.numel() != 256:
            raise ValueError("prefix_gen_conv: stages 2 and 3 run 256 channels in")
        args = (_p(x), _p(part_in), _p(gamma), _p(beta), float(eps), None, 0, None, 0, 0)
    else:
        _f32(emb, "emb")
        if not (tokens.is_cuda and tokens.dtype is torch.int64 and tokens.dim() == 2 and tokens.shape[0] == B and tokens.stride(1) == 1 and
                tokens.shape[1] >= L - 1):
            raise ValueError("prefix_gen_conv: tokens must be an int64 CUDA tensor [B, >= L - 1] with unit column stride")
        if emb.dim() != 2 or emb.shape[1] != Cin or not emb.is_contiguous():
            raise ValueError("prefix_gen_conv: emb contiguous [V, Cin = %d]" % Cin)
        args = (None, None, None, None, 0.0, _p(tokens), tokens.stride(0), _p(emb), emb.shape[0], sos)
    check(lib().unast_prefix_gen_conv(*args, _p(Wp), _p(bias), _p(z), _p(part_out), B, L, Cin, drop_p, seed & 0xFFFFFFFF, stream_id, row0, _stream()),
          "unast_prefix_gen_conv")
    return z


def prefix_gen_finish(z3, part, bns, pre, B, L, running=None, drop_p=0.0, seed=0, stream_id=0, row0=0):
    """pre [B, 256] = dropout(relu(batchnorm3(z3))) of each sequence's last row; part [3, tiles, 2, 256] = the three stages' sums; bns = the three
    BatchNorm1d modules.  While running (an int32 CUDA scalar, None = always) is non-zero their running statistics take one momentum update and
    num_batches_tracked += 1."""
    tiles = prefix_gen_tiles(B, L)
    _pgen_rows("prefix_gen_finish", B, L, (z3, "z3", 256))
    _pgen_part("prefix_gen_finish", part, tiles, lead=(3,))
    if part.shape[1] != tiles:
        raise ValueError("prefix_gen_finish: part must be [3, tiles = %d, 2, 256] exactly (the stages' sums lie tiles*512 doubles apart)" % tiles)
    ldp = _rows(pre, "pre", B, 256)
    if running is not None and not (running.is_cuda and running.dtype is torch.int32 and running.numel() == 1):
        raise ValueError("prefix_gen_finish: running must be an int32 CUDA scalar")
    if len(bns) != 3:
        raise ValueError("prefix_gen_finish: three BatchNorm1d modules")
    stats = []
    for bn in bns:
        stats += [_p(bn.running_mean), _p(bn.running_var), _p(bn.num_batches_tracked), float(bn.momentum)]
    b3 = bns[2]
    check(lib().unast_prefix_gen_finish(_p(z3), _p(part), _p(b3.weight), _p(b3.bias), float(b3.eps), _p(pre), ldp, *stats, _p(running), B, L, drop_p,
                                        seed & 0xFFFFFFFF, stream_id, row0, _stream()), "unast_prefix_gen_finish")
    return pre


PGEN_NONE, PGEN_TANH, PGEN_RELU = 0, 1, 2


def prefix_gen_act_drop(x, out, act, drop_a=0.0, stream_a=0, drop_b=0.0, stream_b=0, seed=0, row0=0):
    """out = dropout_b(dropout_a(act(x))) over [B, C] rows; the masks' row is row0 + b."""
    B, C = x.shape
    ldx, ldo = _rows(x, "x", B, C), _rows(out, "out", B, C)
    check(lib().unast_prefix_gen_act_drop(_p(x), ldx, _p(out), ldo, B, C, act, drop_a, stream_a, drop_b, stream_b, seed & 0xFFFFFFFF, row0, _stream()),
          "unast_prefix_gen_act_drop")
    return out


def _pgen_state(name, stop_lens, running, B):
    if not (stop_lens.is_cuda and stop_lens.dtype is torch.int64 and stop_lens.is_contiguous() and stop_lens.numel() == B):
        raise ValueError("%s: stop_lens must be a contiguous int64 CUDA tensor [B]" % name)
    if not (running.is_cuda and running.dtype is torch.int32 and running.numel() == 1):
        raise ValueError("%s: running must be an int32 CUDA scalar" % name)


def _pgen_wide(name, t, what, cols):
    _f32(t, what)
    if t.dim() != 2 or t.shape[1] < cols or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        raise ValueError("%s: %s must be [B, >= %d] with unit column stride (got %s)" % (name, what, cols, tuple(t.shape)))
    return t.stride(0)


def prefix_gen_end_text(logits, V, tokens, pos, stop_lens, max_len, eos, running):
    """The end of text position pos, under the running flag: tokens[:, pos] = argmax(logits[:, :V]), first EOS -> stop_lens = pos + 1, running."""
    B = logits.shape[0]
    ld = _pgen_wide("prefix_gen_end_text", logits, "logits", V)
    _pgen_state("prefix_gen_end_text", stop_lens, running, B)
    if not (tokens.is_cuda and tokens.dtype is torch.int64 and tokens.dim() == 2 and tokens.shape[0] == B and tokens.stride(1) == 1 and tokens.shape[1] >= max_len):
        raise ValueError("prefix_gen_end_text: tokens must be an int64 CUDA tensor [B, >= max_len] with unit column stride")
    check(lib().unast_prefix_gen_end_text(_p(logits), ld, V, B, _p(tokens), tokens.stride(0), pos, _p(stop_lens), max_len, eos, _p(running), _stream()),
          "unast_prefix_gen_end_text")


def prefix_gen_end_speech(head, M, frames, stops, pos, stop_lens, max_len, running):
    """The end of speech position pos, under the running flag: frames[:, pos + 1] = head[:, :M], stops[:, pos] = head[:, M], the stop rule."""
    B = head.shape[0]
    ld = _pgen_wide("prefix_gen_end_speech", head, "head", M + 1)
    _pgen_state("prefix_gen_end_speech", stop_lens, running, B)
    _f32(frames, "frames"), _f32(stops, "stops")
    if tuple(frames.shape) != (B, max_len + 1, M) or not frames.is_contiguous() or tuple(stops.shape) != (B, max_len) or not stops.is_contiguous():
        raise ValueError("prefix_gen_end_speech: frames contiguous [B, max_len + 1, M], stops contiguous [B, max_len]")
    check(lib().unast_prefix_gen_end_speech(_p(head), ld, M, B, _p(frames), frames.stride(0), _p(stops), stops.stride(0), pos, _p(stop_lens), max_len,
                                            _p(running), _stream()), "unast_prefix_gen_end_speech")


def posenc_fwd(x2d, pe, y, T, scale, drop_p=0.0, seed=0, stream_id=0):
    rows, D = x2d.shape
    check(lib().unast_posenc_fwd(_p(x2d), _p(pe), _p(y), rows, T, D, scale, drop_p, seed & 0xFFFFFFFF, stream_id, _stream()), "unast_posenc_fwd")


def posenc_bwd(dy, gate, dx, scale, drop_p=0.0, seed=0, stream_id=0):
    rows, D = dy.shape
    check(lib().unast_posenc_bwd(_p(dy), _p(gate), _p(dx), rows, D, scale, drop_p, seed & 0xFFFFFFFF, stream_id, _stream()), "unast_posenc_bwd")


def rowmask(x2d, y, p, seed, stream_id):
    rows, D = x2d.shape
    check(lib().unast_rowmask(_p(x2d), _p(y), rows, D, p, seed & 0xFFFFFFFF, stream_id, _stream()), "unast_rowmask")


def add_inplace(a, b):
    check(lib().unast_add_inplace(_p(a), _p(b), a.numel(), _stream()), "unast_add_inplace")


def sum2(dst, a, b=None):
    """dst = a + b (b None: dst = a), contiguous fp32 tensors of one size."""
    check(lib().unast_sum2(_p(dst), _p(a), _p(b), dst.numel(), _stream()), "unast_sum2")


def argmax_rows(x2d, cols, out_i64):
    check(lib().unast_argmax_rows(_p(x2d), x2d.stride(0), x2d.shape[0], cols, _p(out_i64), _stream()), "unast_argmax_rows")


def mask_by_len(x3d, lens_i64):
    B, T = x3d.shape[0], x3d.shape[1]
    D = x3d.numel() // (B * T)
    check(lib().unast_mask_by_len(_p(x3d), _p(lens_i64), B, T, D, _stream()), "unast_mask_by_len")


PRO_NONE, PRO_LN, PRO_LN_DROP, PRO_EMBED, PRO_POSENC = 0, 1, 2, 3, 4
def decode_linear(X, W, bias, Y, act=0, drop_p=0.0, seed=0, stream_id=0, R=None, ln=None, ln_drop=None, embed=None, posenc=None, xn_out=None,
                  cache=None, split_col=0, pos=None, x_frames=None):
    """Y = epilogue(X' W^T) for the rows of one decoding position (csrc/decode.hip).  X' = X, or
    ln=(gamma, beta): LayerNorm(X);  + ln_drop=(p, stream): dropout of that;
    embed=(tokens [B,T], table, pe, scale, (p1, stream1), (p2, stream2)): dropout(dropout(table[tokens[:, pos]]) * scale + pe[pos]);
    posenc=(pe, scale, (p2, stream2)): dropout(X * scale + pe[pos]).
    x_frames: X is a [B, T, K] buffer and the rows are its slice at the device-resident position `pos`."""
    N, K = W.shape
    assert W.stride(1) == 1
    pro, g, b, tokens, ld_tok, emb, pe, scale, d1, d2 = PRO_NONE, None, None, None, 0, None, None, 1.0, (0.0, 0), (0.0, 0)
    if ln is not None:
        g, b = ln
        pro = PRO_LN
        if ln_drop is not None and ln_drop[0] > 0:
            pro, d2 = PRO_LN_DROP, ln_drop
    elif embed is not None:
        tokens, emb, pe, scale, d1, d2 = embed
        pro, ld_tok = PRO_EMBED, tokens.stride(0)
    elif posenc is not None:
        pe, scale, d2 = posenc
        pro = PRO_POSENC
    if x_frames is not None:
        X, ldx, xps, M = x_frames, x_frames.stride(0), x_frames.stride(1), x_frames.shape[0]
        assert x_frames.stride(2) == 1 and x_frames.shape[2] == K
    elif X is not None:
        assert X.shape[1] == K and X.stride(1) == 1
        ldx, xps, M = X.stride(0), 0, X.shape[0]
    else:
        ldx, xps, M = 0, 0, tokens.shape[0]
    check(lib().unast_decode_linear(_p(X), ldx, xps, _p(W), W.stride(0), _p(bias), _p(Y), Y.stride(0) if Y is not None else 0, M, N, K, act,
                                    float(drop_p), seed, stream_id, _p(R), R.stride(0) if R is not None else 0,
                                    pro, _p(g), _p(b), 1e-5, _p(tokens), ld_tok, _p(emb), _p(pe), float(scale),
                                    float(d1[0]), d1[1], float(d2[0]), d2[1],
                                    _p(xn_out), xn_out.stride(0) if xn_out is not None else 0,
                                    _p(cache), cache.stride(1) if cache is not None else 0, cache.shape[1] if cache is not None else 0, split_col, _p(pos),
                                    _stream()), "unast_decode_linear")


def decode_attn(Q, K, V, rows_per_seq, O, H, lens=None, stop_lens=None, pos=None, drop_p=0.0, seed=0, stream_id=0):
    """Single-query attention over cached K/V rows ([B*rows_per_seq, ld] views), head dim 64; valid keys: lens[b], or
    min(stop_lens[b] + 1, pos + 1) with both on the device."""
    B = Q.shape[0]
    assert K.stride(0) == V.stride(0) and Q.shape[1] == 64 * H
    check(lib().unast_decode_attn(_p(Q), Q.stride(0), _p(K), _p(V), K.stride(0), rows_per_seq, _p(lens), _p(stop_lens), _p(pos), _p(O), O.stride(0), B, H, 0.125,
                                  float(drop_p), seed, stream_id, _stream()), "unast_decode_attn")


def decode_end_text(logits, V, tokens, stop_lens, max_len, eos, pos, epoch):
    check(lib().unast_decode_end_text(_p(logits), logits.stride(0), V, logits.shape[0], _p(tokens), tokens.stride(0), _p(stop_lens), max_len, eos, _p(pos),
                                      _p(epoch), _stream()), "unast_decode_end_text")


def decode_end_speech(head, M, outputs, stops, stop_lens, max_len, pos, epoch):
    check(lib().unast_decode_end_speech(_p(head), head.stride(0), M, head.shape[0], _p(outputs), outputs.stride(0), _p(stops), stops.stride(0), _p(stop_lens),
                                        max_len, _p(pos), _p(epoch), _stream()), "unast_decode_end_speech")


def scale_inplace(a, alpha):
    check(lib().unast_scale_inplace(_p(a), float(alpha), a.numel(), _stream()), "unast_scale_inplace")


_JITTER = [0]


def jitter():
    """config.STREAM_JITTER > 0: a spin of pseudo-random length (0 .. STREAM_JITTER us, a third of the calls none) on the current stream."""
    if not config.STREAM_JITTER:
        return
    _JITTER[0] = (_JITTER[0] * 1103515245 + 12345 + config.STREAM_JITTER_SEED) & 0x7FFFFFFF
    r = (_JITTER[0] >> 8) % 3000
    if r >= 2000:
        return
    check(lib().unast_spin(int(r * config.STREAM_JITTER / 2000), _stream()), "unast_spin")


def shift_frames(mel3d, out3d):
    """out[b,0] = 0, out[b,t] = mel[b,t-1] (the decoder input of teacher forcing)."""
    B, T, M = mel3d.shape
    check(lib().unast_shift_frames(_p(mel3d), _p(out3d), B, T, M, _stream()), "unast_shift_frames")
    return out3d


def add_strided(dst2d, src2d, cols):
    """dst2d[:, :cols] += src2d[:, :cols] (row strides may differ)."""
    rows = dst2d.shape[0]
    check(lib().unast_add_strided(_p(dst2d), dst2d.stride(0), _p(src2d), src2d.stride(0), rows, cols, _stream()), "unast_add_strided")


def specaugment(mel, lens_i32, out, seed, stream_id, freq_mask=20, time_mask=100):
    B, T, M = mel.shape
    ws = torch.empty(B, dtype=torch.float32, device=mel.device)
    check(lib().unast_specaugment(_p(mel), _p(lens_i32), _p(out), _p(ws), B, T, M, freq_mask, time_mask, seed & 0xFFFFFFFF, stream_id, _stream()),
          "unast_specaugment")


def disc_gather(t_hid, s_hid, t_len, s_len, perm, out, out_len):
    B, Tt, D = t_hid.shape
    Ts = s_hid.shape[1]
    check(lib().unast_disc_gather(_p(t_hid), _p(s_hid), _p(t_len), _p(s_len), _p(perm), _p(out), _p(out_len), B, Tt, Ts, D, _stream()),
          "unast_disc_gather")


def disc_scatter(dout, perm, dt_hid, ds_hid):
    B, Tt, D = dt_hid.shape
    Ts = ds_hid.shape[1]
    check(lib().unast_disc_scatter(_p(dout), _p(perm), _p(dt_hid), _p(ds_hid), B, Tt, Ts, D, _stream()), "unast_disc_scatter")


# ---- losses ------------------------------------------------------------------------------------------------
def speech_loss_fwd(gold, head, post, lens_i32, eos_weight, ws, loss):
    B, T, M = gold.shape
    check(lib().unast_speech_loss_fwd(_p(gold), _p(head), head.stride(-2), _p(post), _p(lens_i32), B, T, M, eos_weight, _p(ws), _p(loss),
                                      _stream()), "unast_speech_loss_fwd")


def speech_loss_bwd(gold, head, post, lens_i32, eos_weight, gscale, d_head, d_post):
    B, T, M = gold.shape
    check(lib().unast_speech_loss_bwd(_p(gold), _p(head), head.stride(-2), _p(post), _p(lens_i32), B, T, M, eos_weight, _p(gscale),
                                      _p(d_head), _p(d_post), _stream()), "unast_speech_loss_bwd")


def text_loss_fwd(logits2d, gold, V, eos_weight, ws, loss):
    check(lib().unast_text_loss_fwd(_p(logits2d), logits2d.stride(0), _p(gold), logits2d.shape[0], V, eos_weight, _p(ws), _p(loss),
                                    _stream()), "unast_text_loss_fwd")


def text_head_loss(x2d, W, bias, gold, V, eos_weight, gscale, logits2d, dlogits2d, ws, loss):
    """TextPostnet.fc1 + text_loss + its gradient with respect to the logits in one launch (csrc/loss.hip text_head_loss_kernel)."""
    check(lib().unast_text_head_loss(_p(x2d), x2d.stride(0), _p(W), _p(bias), _p(gold), x2d.shape[0], x2d.shape[1], V, float(eos_weight), float(gscale),
                                     _p(logits2d), _p(dlogits2d), logits2d.stride(0), _p(ws), _p(loss), _stream()), "unast_text_head_loss")


def speech_head_loss(x2d, W, bias, gold2d, lens, B, T, M, eos_weight, gscale, head, d_head, ws):
    """[linear_project | stop_linear] + the pre-net MSE and stop BCE of speech_loss + their gradient in one launch (csrc/loss.hip)."""
    check(lib().unast_speech_head_loss(_p(x2d), x2d.stride(0), _p(W), _p(bias), _p(gold2d), _p(lens), B, T, x2d.shape[1], M, float(eos_weight), float(gscale),
                                       _p(head), _p(d_head), head.stride(0), _p(ws), _stream()), "unast_speech_head_loss")


def speech_post_loss(gold2d, post2d, lens, B, T, M, gscale, d_post, ws, loss):
    """The post-net MSE term, its gradient and the finished speech_loss scalar (after speech_head_loss on the same stream)."""
    check(lib().unast_speech_post_loss(_p(gold2d), _p(post2d), _p(lens), B, T, M, float(gscale), _p(d_post), _p(ws), _p(loss), _stream()), "unast_speech_post_loss")


def text_loss_bwd(logits2d, gold, V, eos_weight, ws, gscale, dlogits):
    check(lib().unast_text_loss_bwd(_p(logits2d), logits2d.stride(0), _p(gold), logits2d.shape[0], V, eos_weight, _p(ws), _p(gscale),
                                    _p(dlogits), _stream()), "unast_text_loss_bwd")


def disc_targets(perm, B, flip, out, smoothing=0.1):
    check(lib().unast_disc_targets(_p(perm), perm.numel(), B, int(flip), smoothing, _p(out), _stream()), "unast_disc_targets")


def randperm(n, seed, stream_id, device):
    out = torch.empty(n, dtype=torch.int64, device=device)
    check(lib().unast_randperm(_p(out), n, seed & 0xFFFFFFFF, stream_id, _stream()), "unast_randperm")
    return out


def bce_logits(logits, ldx, targets, n, loss=None, gscale=None, dlogits=None, ldd=1):
    check(lib().unast_bce_logits(_p(logits), ldx, _p(targets), n, _p(gscale), _p(loss), _p(dlogits), ldd, _stream()), "unast_bce_logits")


# ---- LSTM discriminator ------------------------------------------------------------------------------------
def _lstm_hidden(whh, other, per_unit, name):
    """The LSTM kernels' width: W_hh's row length, which the saved-state operand (4 H gate rows or H cell states per step) must share."""
    H = whh.shape[-1]
    if other.shape[-1] != per_unit * H:
        raise ValueError("%s: W_hh has rows of %d but the state operand's last dimension is %d, not %d" % (name, H, other.shape[-1], per_unit * H))
    return H


def lstm_fwd(xproj, whh, b_ih, b_hh, lens_i32, y, gates, cs, hprev, hfinal, ndir, whh_dir_stride, bias_dir_stride):
    Bd, T = xproj.shape[0], xproj.shape[1]
    H = _lstm_hidden(whh, cs, 1, "lstm_fwd")
    check(lib().unast_lstm_fwd(_p(xproj), _p(whh), _p(b_ih), _p(b_hh), _p(lens_i32), _p(y), _p(gates), _p(cs), _p(hprev), _p(hfinal), Bd, T,
                               ndir, H, whh_dir_stride, bias_dir_stride, _stream()), "unast_lstm_fwd")


def lstm_bwd(dy, dhfinal, whh, gates, cs, lens_i32, dgates, ndir, whh_dir_stride):
    Bd, T = gates.shape[0], gates.shape[1]
    H = _lstm_hidden(whh, gates, 4, "lstm_bwd")
    check(lib().unast_lstm_bwd(_p(dy), _p(dhfinal), _p(whh), _p(gates), _p(cs), _p(lens_i32), _p(dgates), Bd, T, ndir, H, whh_dir_stride,
                               _stream()), "unast_lstm_bwd")


# ---- RNN model family: eval path and encoder training (csrc/rnn.hip) --------------------------------------
def _dense_f32(t, name, shape=None):
    _f32(t, name)
    if not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError("%s must be contiguous%s (got shape %s, strides %s)" % (name, "" if shape is None else " with shape %s" % (tuple(shape),),
                                                                              tuple(t.shape), t.stride()))


def lstm_whh_fragments(whh):
    """W_hh [ndir, 1024, 256] (or [1024, 256]) in the fragment order unast_lstm_seq_fwd streams: [ndir][64 row tiles][16 k groups][64 lanes][4]
    with frag[d][n][g][16 q + j][s] = W_hh[d][16 n + j][16 g + 4 q + s].  A copy: callers cache it next to the weight."""
    if whh.dim() == 2:
        whh = whh.unsqueeze(0)
    if whh.dim() != 3 or whh.shape[1:] != (1024, 256):
        raise ValueError("lstm_whh_fragments: W_hh must be [ndir, 1024, 256] (hidden 256), got %s" % (tuple(whh.shape),))
    nd = whh.shape[0]
    return whh.detach().reshape(nd, 64, 16, 16, 4, 4).permute(0, 1, 3, 4, 2, 5).contiguous().view(nd, 64, 16, 64, 4)


def lstm_seq_fwd(xproj, wfrag, b_ih, b_hh, lens_i32, y, hfinal, cfinal):
    """One packed nn.LSTM layer's recurrence at hidden 256, forward only.  xproj [B,T,ndir*1024], wfrag = lstm_whh_fragments(W_hh),
    b_ih / b_hh [ndir*1024] (or [ndir,1024]), lens int32 [B]; writes y [B,T,ndir*256] (zeros at t >= lens[b]), hfinal / cfinal [B,ndir*256]."""
    if xproj.dim() != 3 or wfrag.dim() != 5 or tuple(wfrag.shape[1:]) != (64, 16, 64, 4):
        raise ValueError("lstm_seq_fwd: xproj [B,T,ndir*1024] and wfrag [ndir,64,16,64,4] (ops.lstm_whh_fragments)")
    B, T, _ = xproj.shape
    ndir = wfrag.shape[0]
    if ndir not in (1, 2) or B < 1 or T < 1:
        raise ValueError("lstm_seq_fwd: ndir must be 1 or 2, B and T at least 1 (got ndir=%d, B=%d, T=%d)" % (ndir, B, T))
    _dense_f32(xproj, "xproj", (B, T, ndir * 1024))
    _dense_f32(wfrag, "wfrag")
    for t, n in ((b_ih, "b_ih"), (b_hh, "b_hh")):
        _f32(t, n)
        if not t.is_contiguous() or t.numel() != ndir * 1024:
            raise ValueError("lstm_seq_fwd: %s must hold ndir*1024 contiguous floats" % n)
    _dense_f32(y, "y", (B, T, ndir * 256))
    _dense_f32(hfinal, "hfinal", (B, ndir * 256))
    _dense_f32(cfinal, "cfinal", (B, ndir * 256))
    if not (lens_i32.is_cuda and lens_i32.dtype == torch.int32 and lens_i32.is_contiguous() and lens_i32.numel() == B):
        raise TypeError("lstm_seq_fwd: lens must be a contiguous int32 CUDA tensor [B]")
    check(lib().unast_lstm_seq_fwd(_p(xproj), _p(wfrag), _p(b_ih), _p(b_hh), _p(lens_i32), _p(y), _p(hfinal), _p(cfinal), B, T, ndir, 256, _stream()),
          "unast_lstm_seq_fwd")
    return y


def lstm_whh_fragments_bwd(whh):
    """W_hh [ndir, 1024, 256] (or [1024, 256]) in the fragment order unast_lstm_seq_bwd streams, the B operand [k = gate row][n = unit]:
    [ndir][16 unit tiles][64 k groups][64 lanes][4] with frag[d][n][g][16 q + j][s] = W_hh[d][16 g + 4 q + s][16 n + j].  A copy."""
    if whh.dim() == 2:
        whh = whh.unsqueeze(0)
    if whh.dim() != 3 or whh.shape[1:] != (1024, 256):
        raise ValueError("lstm_whh_fragments_bwd: W_hh must be [ndir, 1024, 256] (hidden 256), got %s" % (tuple(whh.shape),))
    nd = whh.shape[0]
    return whh.detach().reshape(nd, 64, 4, 4, 16, 16).permute(0, 4, 1, 2, 5, 3).contiguous().view(nd, 16, 64, 64, 4)


def _lstm_seq_dims(name, lead, lead_cols, wfrag, frag_shape, lens_i32):
    if lead.dim() != 3 or wfrag.dim() != 5 or tuple(wfrag.shape[1:]) != frag_shape:
        raise ValueError("%s: a [B,T,ndir*%d] operand and W_hh fragments [ndir,%d,%d,%d,%d]" % ((name, lead_cols) + frag_shape))
    B, T, _ = lead.shape
    ndir = wfrag.shape[0]
    if ndir not in (1, 2) or B < 1 or T < 1:
        raise ValueError("%s: ndir must be 1 or 2, B and T at least 1 (got ndir=%d, B=%d, T=%d)" % (name, ndir, B, T))
    _dense_f32(lead, name + " operand", (B, T, ndir * lead_cols))
    _dense_f32(wfrag, "wfrag")
    if not (lens_i32.is_cuda and lens_i32.dtype == torch.int32 and lens_i32.is_contiguous() and lens_i32.numel() == B):
        raise TypeError("%s: lens must be a contiguous int32 CUDA tensor [B]" % name)
    return B, T, ndir


def lstm_seq_fwd_train(xproj, wfrag, b_ih, b_hh, lens_i32, y, hfinal, cfinal, saved, hprev):
    """lstm_seq_fwd (bit-identical y, hfinal, cfinal) that also writes what lstm_seq_bwd reads: saved [B,T,ndir,5,256] (i, f, g, o, c_t; rows
    t >= lens[b] are left as they are and never read) and hprev [B,T,ndir*256] (h_{t-1}; zeros at t >= lens[b])."""
    B, T, ndir = _lstm_seq_dims("lstm_seq_fwd_train", xproj, 1024, wfrag, (64, 16, 64, 4), lens_i32)
    for t, n in ((b_ih, "b_ih"), (b_hh, "b_hh")):
        _f32(t, n)
        if not t.is_contiguous() or t.numel() != ndir * 1024:
            raise ValueError("lstm_seq_fwd_train: %s must hold ndir*1024 contiguous floats" % n)
    _dense_f32(y, "y", (B, T, ndir * 256))
    _dense_f32(hfinal, "hfinal", (B, ndir * 256))
    _dense_f32(cfinal, "cfinal", (B, ndir * 256))
    _dense_f32(saved, "saved", (B, T, ndir, 5, 256))
    _dense_f32(hprev, "hprev", (B, T, ndir * 256))
    check(lib().unast_lstm_seq_fwd_train(_p(xproj), _p(wfrag), _p(b_ih), _p(b_hh), _p(lens_i32), _p(y), _p(hfinal), _p(cfinal), _p(saved), _p(hprev),
                                         B, T, ndir, 256, _stream()), "unast_lstm_seq_fwd_train")
    return y


def lstm_seq_bwd(dy, wfrag_t, saved, lens_i32, dxproj, dhfinal=None, dcfinal=None):
    """Backward of lstm_seq_fwd_train's recurrence.  dy [B,T,ndir*256] (rows t >= lens[b] are not read), wfrag_t = lstm_whh_fragments_bwd(W_hh),
    saved as lstm_seq_fwd_train wrote it, dhfinal / dcfinal [B,ndir*256] or None (zero); writes dxproj [B,T,ndir*1024], the gradient of the
    gate pre-activations (exact zeros at t >= lens[b])."""
    B, T, ndir = _lstm_seq_dims("lstm_seq_bwd", dy, 256, wfrag_t, (16, 64, 64, 4), lens_i32)
    _dense_f32(saved, "saved", (B, T, ndir, 5, 256))
    _dense_f32(dxproj, "dxproj", (B, T, ndir * 1024))
    for t, n in ((dhfinal, "dhfinal"), (dcfinal, "dcfinal")):
        if t is not None:
            _dense_f32(t, n, (B, ndir * 256))
    check(lib().unast_lstm_seq_bwd(_p(dy), _p(dhfinal), _p(dcfinal), _p(wfrag_t), _p(saved), _p(lens_i32), _p(dxproj), B, T, ndir, 256, _stream()),
          "unast_lstm_seq_bwd")
    return dxproj


ATTN_LUONG, ATTN_LSA = 0, 1


def rnn_attn_step(mode, h, Wq, mem, v, enc, lens_i32, ctx, prev=None, cum=None, conv_w=None, dense_w=None):
    """One additive-attention step (mode ATTN_LUONG / ATTN_LSA) for B sequences: h [B,256] query rows (row stride free), Wq [A,256],
    mem [B,Tk,A], v [A], enc [B,Tk,512], lens int32 [B]; writes ctx [B,512] (row stride free) and the weights into prev [B,Tk]
    (optional in Luong mode).  LSA mode reads prev and cum [B,Tk], adds the weights to cum and needs conv_w [32,2,31], dense_w [A,32]."""
    if mode not in (ATTN_LUONG, ATTN_LSA):
        raise ValueError("rnn_attn_step: mode must be ATTN_LUONG (0) or ATTN_LSA (1), got %r" % (mode,))
    if mem.dim() != 3 or enc.dim() != 3:
        raise ValueError("rnn_attn_step: mem [B,Tk,A] and enc [B,Tk,512]")
    B, Tk, A = mem.shape
    if A % 4 or A > 64 or A < 4:
        raise ValueError("rnn_attn_step: attn_dim must be a multiple of 4, at most 64 (got %d)" % A)
    if not 1 <= Tk <= 2048:
        raise ValueError("rnn_attn_step: 1 <= Tk <= 2048 (got %d)" % Tk)
    _dense_f32(mem, "mem")
    _dense_f32(enc, "enc", (B, Tk, 512))
    _dense_f32(Wq, "Wq", (A, 256))
    _f32(v, "v")
    if not v.is_contiguous() or v.numel() != A:
        raise ValueError("rnn_attn_step: v must hold A contiguous floats")
    for t, n, cols in ((h, "h", 256), (ctx, "ctx", 512)):
        _f32(t, n)
        if t.dim() != 2 or tuple(t.shape) != (B, cols) or t.stride(1) != 1 or t.stride(0) % 4 or t.stride(0) < cols or t.data_ptr() % 16:
            raise ValueError("rnn_attn_step: %s must be [B,%d] with unit column stride and 16-byte aligned rows" % (n, cols))
    if not (lens_i32.is_cuda and lens_i32.dtype == torch.int32 and lens_i32.is_contiguous() and lens_i32.numel() == B):
        raise TypeError("rnn_attn_step: lens must be a contiguous int32 CUDA tensor [B]")
    for t, n in ((prev, "prev"), (cum, "cum")):
        if t is not None:
            _dense_f32(t, n, (B, Tk))
    if mode == ATTN_LSA:
        if prev is None or cum is None or conv_w is None or dense_w is None:
            raise ValueError("rnn_attn_step: LSA mode needs prev, cum, conv_w and dense_w")
        _dense_f32(conv_w, "conv_w", (32, 2, 31))
        _dense_f32(dense_w, "dense_w", (A, 32))
    check(lib().unast_rnn_attn_step(mode, _p(h), h.stride(0), _p(Wq), _p(mem), _p(v), _p(enc), _p(lens_i32), _p(prev), _p(cum), _p(conv_w), _p(dense_w),
                                    _p(ctx), ctx.stride(0), B, Tk, A, _stream()), "unast_rnn_attn_step")
    return ctx


def lstm_cell(gates, c, h):
    """c, h = LSTM cell update from the summed gate pre-activations [B,1024] (i,f,g,o) at hidden 256; c [B,256] in place, h [B,256] written."""
    B = gates.shape[0]
    for t, n, cols in ((gates, "gates", 1024), (c, "c", 256), (h, "h", 256)):
        _f32(t, n)
        if t.dim() != 2 or tuple(t.shape) != (B, cols) or t.stride(1) != 1 or t.stride(0) < cols:
            raise ValueError("lstm_cell: %s must be [B,%d] with unit column stride" % (n, cols))
    check(lib().unast_lstm_cell(_p(gates), gates.stride(0), _p(c), c.stride(0), _p(h), h.stride(0), B, 256, _stream()), "unast_lstm_cell")
    return h


# ---- SpeechRNN decoder training (csrc/rnn.hip; unast_amd/train_rnn.py) -------------------------------------------------------------------
def _rows(t, name, B, cols, align=1):
    """A [B, cols] float32 view with unit column stride (a position's slice of a [B,T,...] slab); returns its row stride."""
    _f32(t, name)
    if t.dim() != 2 or tuple(t.shape) != (B, cols) or t.stride(1) != 1 or t.stride(0) < cols or t.stride(0) % align or t.data_ptr() % (4 * align):
        raise ValueError("%s must be [%d,%d] with unit column stride%s (got shape %s, strides %s)"
                         % (name, B, cols, " and %d-byte aligned rows" % (4 * align) if align > 1 else "", tuple(t.shape), t.stride()))
    return t.stride(0)


def _attn_operands(name, h, Wq, mem, v, enc, lens_i32):
    if mem.dim() != 3 or enc.dim() != 3:
        raise ValueError("%s: mem [B,Tk,A] and enc [B,Tk,512]" % name)
    B, Tk, A = mem.shape
    if A % 4 or A > 64 or A < 4:
        raise ValueError("%s: attn_dim must be a multiple of 4, at most 64 (got %d)" % (name, A))
    if not 1 <= Tk <= 2048:
        raise ValueError("%s: 1 <= Tk <= 2048 (got %d)" % (name, Tk))
    _dense_f32(mem, "mem")
    _dense_f32(enc, "enc", (B, Tk, 512))
    _dense_f32(Wq, "Wq", (A, 256))
    _f32(v, "v")
    if not v.is_contiguous() or v.numel() != A:
        raise ValueError("%s: v must hold A contiguous floats" % name)
    _rows(h, "h", B, 256, 4)
    if not (lens_i32.is_cuda and lens_i32.dtype == torch.int32 and lens_i32.is_contiguous() and lens_i32.numel() == B):
        raise TypeError("%s: lens must be a contiguous int32 CUDA tensor [B]" % name)
    return B, Tk, A


def _same_stride(name, B, Tk, *named):
    ld = None
    for t, n in named:
        if t is None:
            continue
        s = _rows(t, n, B, Tk)
        if ld is not None and s != ld:
            raise ValueError("%s: %s must share one row stride (got %d and %d)" % (name, " / ".join(n for _, n in named), ld, s))
        ld = s
    return ld or 0


def rnn_attn_step_train(mode, h, Wq, mem, v, enc, lens_i32, ctx, w_out, prev_in=None, cum_in=None, cum_out=None, conv_w=None, dense_w=None):
    """rnn_attn_step out of place (ctx and the weights carry its bits): the weights go to w_out [B,Tk]; LSA mode reads prev_in / cum_in and
    writes cum_in + weights to cum_out.  All [B,Tk] operands are row-strided views (prev_in / cum_in share a stride, w_out / cum_out another)."""
    if mode not in (ATTN_LUONG, ATTN_LSA):
        raise ValueError("rnn_attn_step_train: mode must be ATTN_LUONG (0) or ATTN_LSA (1), got %r" % (mode,))
    B, Tk, A = _attn_operands("rnn_attn_step_train", h, Wq, mem, v, enc, lens_i32)
    ldc = _rows(ctx, "ctx", B, 512, 2)
    if mode == ATTN_LSA:
        if prev_in is None or cum_in is None or cum_out is None or conv_w is None or dense_w is None:
            raise ValueError("rnn_attn_step_train: LSA mode needs prev_in, cum_in, cum_out, conv_w and dense_w")
        _dense_f32(conv_w, "conv_w", (32, 2, 31))
        _dense_f32(dense_w, "dense_w", (A, 32))
    else:
        prev_in = cum_in = cum_out = None
    ld_in = _same_stride("rnn_attn_step_train", B, Tk, (prev_in, "prev_in"), (cum_in, "cum_in"))
    ld_out = _same_stride("rnn_attn_step_train", B, Tk, (w_out, "w_out"), (cum_out, "cum_out"))
    check(lib().unast_rnn_attn_step_train(mode, _p(h), h.stride(0), _p(Wq), _p(mem), _p(v), _p(enc), _p(lens_i32), _p(prev_in), _p(cum_in), ld_in,
                                          _p(w_out), _p(cum_out), ld_out, _p(conv_w), _p(dense_w), _p(ctx), ldc, B, Tk, A, _stream()),
          "unast_rnn_attn_step_train")
    return ctx


def rnn_attn_step_bwd_ws(B, Tk, A, device):
    return torch.empty(lib().unast_rnn_attn_step_bwd_ws_floats(B, Tk, A), dtype=torch.float32, device=device)


def rnn_attn_step_bwd(mode, d_ctx, w, h, Wq, mem, v, enc, lens_i32, d_h, d_q, d_mem, dv_part, ws, prev=None, cum=None, conv_w=None, dense_w=None,
                      d_w_a=None, d_w_b=None, carry=False, ddense_part=None, dconv_part=None, d_prev=None, d_cum=None):
    """Backward of one attention position (include/unast_hip.h): d_ctx [B,512], the saved weights w (and LSA's prev / cum) [B,Tk] row-strided,
    the forward's h, Wq, mem, v, enc, lens; incoming weight gradients d_w_a + d_w_b [B,Tk] (None = zero).  Writes d_h [B,256], d_q [B,A]; adds
    to d_mem [B,Tk,A] and the per-sequence partial sums dv_part [B,A], ddense_part [B,A,32], dconv_part [B,32,2,31]; LSA writes d_prev and
    d_cum [B,Tk] (d_cum += d_w_b with carry).  ws = rnn_attn_step_bwd_ws(B, Tk, A, device)."""
    if mode not in (ATTN_LUONG, ATTN_LSA):
        raise ValueError("rnn_attn_step_bwd: mode must be ATTN_LUONG (0) or ATTN_LSA (1), got %r" % (mode,))
    B, Tk, A = _attn_operands("rnn_attn_step_bwd", h, Wq, mem, v, enc, lens_i32)
    lddc = _rows(d_ctx, "d_ctx", B, 512)
    lddh = _rows(d_h, "d_h", B, 256)
    lddq = _rows(d_q, "d_q", B, A)
    _dense_f32(d_mem, "d_mem", (B, Tk, A))
    _dense_f32(dv_part, "dv_part", (B, A))
    _dense_f32(ws, "ws")
    if mode == ATTN_LSA:
        if any(t is None for t in (prev, cum, conv_w, dense_w, ddense_part, dconv_part, d_prev, d_cum)):
            raise ValueError("rnn_attn_step_bwd: LSA mode needs prev, cum, conv_w, dense_w, ddense_part, dconv_part, d_prev and d_cum")
        _dense_f32(conv_w, "conv_w", (32, 2, 31))
        _dense_f32(dense_w, "dense_w", (A, 32))
        _dense_f32(ddense_part, "ddense_part", (B, A, 32))
        _dense_f32(dconv_part, "dconv_part", (B, 32, 2, 31))
    else:
        prev = cum = conv_w = dense_w = ddense_part = dconv_part = d_prev = d_cum = None
    ldw = _same_stride("rnn_attn_step_bwd", B, Tk, (w, "w"), (prev, "prev"), (cum, "cum"))
    ldd = _same_stride("rnn_attn_step_bwd", B, Tk, (d_w_a, "d_w_a"), (d_w_b, "d_w_b"), (d_prev, "d_prev"), (d_cum, "d_cum"))
    check(lib().unast_rnn_attn_step_bwd(mode, _p(d_ctx), lddc, _p(w), _p(prev), _p(cum), ldw, _p(h), h.stride(0), _p(Wq), _p(mem), _p(v), _p(enc),
                                        _p(lens_i32), _p(conv_w), _p(dense_w), _p(d_w_a), _p(d_w_b), int(bool(carry)), ldd, _p(d_h), lddh, _p(d_q), lddq,
                                        _p(d_mem), _p(dv_part), _p(ddense_part), _p(dconv_part), _p(d_prev), _p(d_cum), _p(ws), ws.numel(), B, Tk, A,
                                        _stream()), "unast_rnn_attn_step_bwd")
    return d_h


def lstm_cell_train(gates, c_prev, saved, h, mask=None, hd=None):
    """lstm_cell out of place (h and c_t carry its bits): gates [B,1024], c_prev [B,256]; writes saved [B,5,256] = (i, f, g, o, c_t) and h [B,256];
    hd [B,256] (optional) = h * mask (mask optional: a dropout factor tensor).  All operands may be row-strided views."""
    B = gates.shape[0]
    ldg, ldcp, ldh = _rows(gates, "gates", B, 1024), _rows(c_prev, "c_prev", B, 256), _rows(h, "h", B, 256)
    _f32(saved, "saved")
    if saved.dim() != 3 or tuple(saved.shape) != (B, 5, 256) or saved.stride(2) != 1 or saved.stride(1) != 256:
        raise ValueError("lstm_cell_train: saved must be [B,5,256] with dense rows")
    if mask is not None and hd is None:
        raise ValueError("lstm_cell_train: a mask needs hd")
    ldm = _rows(mask, "mask", B, 256) if mask is not None else 0
    ldhd = _rows(hd, "hd", B, 256) if hd is not None else 0
    check(lib().unast_lstm_cell_train(_p(gates), ldg, _p(c_prev), ldcp, _p(saved), saved.stride(0), _p(h), ldh, _p(mask), ldm, _p(hd), ldhd, B, 256,
                                      _stream()), "unast_lstm_cell_train")
    return h


def lstm_cell_bwd(saved, c_prev, dG, dc_out, dh=None, dh2=None, mask=None, dc_in=None):
    """Backward of one cell update: dh_total = dh + dh2 * mask (each optional), dc = dc_in + dh_total o (1 - tanh^2 c_t); writes dG [B,1024]
    (gate pre-activation gradients) and dc_out = dc f (may be dc_in).  Row-strided views are fine."""
    B = dG.shape[0]
    ldg, ldcp, lddco = _rows(dG, "dG", B, 1024), _rows(c_prev, "c_prev", B, 256), _rows(dc_out, "dc_out", B, 256)
    _f32(saved, "saved")
    if saved.dim() != 3 or tuple(saved.shape) != (B, 5, 256) or saved.stride(2) != 1 or saved.stride(1) != 256:
        raise ValueError("lstm_cell_bwd: saved must be [B,5,256] with dense rows")
    if mask is not None and dh2 is None:
        raise ValueError("lstm_cell_bwd: a mask needs dh2")
    ld = lambda t, n: _rows(t, n, B, 256) if t is not None else 0                        # noqa: E731
    check(lib().unast_lstm_cell_bwd(_p(dh), ld(dh, "dh"), _p(dh2), ld(dh2, "dh2"), _p(mask), ld(mask, "mask"), _p(dc_in), ld(dc_in, "dc_in"), _p(saved),
                                    saved.stride(0), _p(c_prev), ldcp, _p(dG), ldg, _p(dc_out), lddco, B, 256, _stream()), "unast_lstm_cell_bwd")
    return dG


def tanh_bwd(dy2d, y2d):
    """dy *= 1 - y^2 in place (y = the stored tanh output)."""
    if not (dy2d.dim() == 2 and dy2d.shape == y2d.shape and dy2d.stride(1) == 1 and y2d.stride(1) == 1):
        raise ValueError("tanh_bwd: dy and y [rows, C], unit column strides")
    _f32(dy2d, "dy"), _f32(y2d, "y")
    check(lib().unast_tanh_bwd(_p(dy2d), dy2d.stride(0), _p(y2d), y2d.stride(0), dy2d.shape[0], dy2d.shape[1], _stream()), "unast_tanh_bwd")
    return dy2d


def tanh_rows(x2d):
    """x = tanh(x) in place over a [rows, cols] view with unit column stride."""
    _f32(x2d, "x")
    if x2d.dim() != 2 or x2d.stride(1) != 1:
        raise ValueError("tanh_rows: a 2-D view with unit column stride")
    check(lib().unast_tanh_rows(_p(x2d), x2d.stride(0), x2d.shape[0], x2d.shape[1], _stream()), "unast_tanh_rows")
    return x2d


def text_window(tokens, emb, out, pos, teacher_forced, sos):
    """out [B,W,E] = embedding rows of the last W positions of the prefix at device position `pos` (zero rows before the prefix starts).
    tokens int64 [B,L] with unit column stride: the generated tokens (SOS first), or -- teacher_forced -- the target."""
    B, W, E = out.shape
    _dense_f32(out, "out")
    _dense_f32(emb, "emb")
    if not (tokens.is_cuda and tokens.dtype == torch.int64 and tokens.dim() == 2 and tokens.shape[0] == B and tokens.stride(1) == 1):
        raise TypeError("text_window: tokens must be an int64 CUDA tensor [B,L] with unit column stride")
    if emb.shape[1] != E or E % 4 or not (pos.is_cuda and pos.dtype == torch.int64):
        raise ValueError("text_window: emb [V,E] with E % 4 == 0 matching out, pos an int64 CUDA scalar")
    check(lib().unast_text_window(_p(tokens), tokens.stride(0), _p(emb), E, emb.shape[0], _p(out), B, W, _p(pos), int(bool(teacher_forced)), sos, _stream()),
          "unast_text_window")
    return out


def window_mask(x3d, pos, teacher_forced):
    """Clears the rows of x [B,W,C] that stand for positions before the prefix (see text_window)."""
    _dense_f32(x3d, "x")
    B, W, C = x3d.shape
    if C % 4:
        raise ValueError("window_mask: C % 4 == 0")
    check(lib().unast_window_mask(_p(x3d), B, W, C, _p(pos), int(bool(teacher_forced)), _stream()), "unast_window_mask")
    return x3d


def pos_advance(pos, epoch=None):
    check(lib().unast_pos_advance(_p(pos), _p(epoch), _stream()), "unast_pos_advance")


def rnn_linear(X, W, bias, Y, R=None, act=0, pos=None, x_frames=None, y_frames=None):
    """Y = act(X W^T + bias + R) with plain fp32 products for the few rows of one RNN decoder step (csrc/rnn.hip; K <= 1024).
    x_frames [B,T,K] / y_frames [B,T,N]: the rows are the slice at the device-resident position `pos`."""
    N, K = W.shape
    if W.stride(1) != 1 or K % 4 or K > 1024:
        raise ValueError("rnn_linear: W [N,K] with unit column stride, K % 4 == 0, K <= 1024 (got %s)" % (tuple(W.shape),))
    if x_frames is not None:
        if x_frames.dim() != 3 or x_frames.shape[2] != K or x_frames.stride(2) != 1 or pos is None:
            raise ValueError("rnn_linear: x_frames [B,T,K] with unit column stride, and pos")
        X, ldx, xps, M = x_frames, x_frames.stride(0), x_frames.stride(1), x_frames.shape[0]
    else:
        if X.dim() != 2 or X.shape[1] != K or X.stride(1) != 1:
            raise ValueError("rnn_linear: X [M,%d] with unit column stride (got %s)" % (K, tuple(X.shape)))
        ldx, xps, M = X.stride(0), 0, X.shape[0]
    if y_frames is not None:
        if y_frames.dim() != 3 or y_frames.shape[0] != M or y_frames.shape[2] < N or y_frames.stride(2) != 1 or pos is None:
            raise ValueError("rnn_linear: y_frames [M,T,>=N] with unit column stride, and pos")
        Y, ldy, yps = y_frames, y_frames.stride(0), y_frames.stride(1)
    else:
        if Y.dim() != 2 or Y.shape[0] != M or Y.shape[1] < N or Y.stride(1) != 1:
            raise ValueError("rnn_linear: Y [M,>=N] with unit column stride")
        ldy, yps = Y.stride(0), 0
    if R is not None and (R.dim() != 2 or R.shape[0] != M or R.shape[1] < N or R.stride(1) != 1):
        raise ValueError("rnn_linear: R [M,>=N] with unit column stride")
    for t, n in ((X, "X"), (W, "W"), (bias, "bias"), (R, "R"), (Y, "Y")):
        _f32(t, n)
    check(lib().unast_rnn_linear(_p(X), ldx, xps, _p(W), W.stride(0), _p(bias), _p(R), R.stride(0) if R is not None else 0, _p(Y), ldy, yps, _p(pos),
                                 M, N, K, act, _stream()), "unast_rnn_linear")
    return Y


def leaky_dropout(x, dy, out, slope, drop_p=0.0, seed=0, stream_id=0):
    rows = x.shape[0]
    D = x.numel() // rows
    check(lib().unast_leaky_dropout(_p(x), _p(dy), _p(out), rows, D, slope, drop_p, seed & 0xFFFFFFFF, stream_id, _stream()),
          "unast_leaky_dropout")


# ---- CBHG vocoder (eval forward) ---------------------------------------------------------------------------
def conv_taps_fwd(x3d, Wp, bias, out, pad_left, act=0, R=None):
    """x3d [B,T,Cin] (a column slice of a wider buffer is fine), Wp [Cout,taps,Cin] (tap-major, contiguous), out [B,T,Cout] (likewise a
    slice): out[b,t] = epi(sum_j Wp[:,j,:] x[b, t + j - pad_left]), zero outside each sequence; epi = + bias -> relu if act -> + R."""
    B, T, Cin = x3d.shape
    Cout, taps, _ = Wp.shape
    dense = lambda t: B == 1 or t.stride(0) == T * t.stride(1)              # noqa: E731  (a single sequence has no batch stride to speak of)
    if not (Wp.is_contiguous() and Wp.shape[2] == Cin and x3d.stride(2) == 1 and out.stride(2) == 1 and dense(x3d) and dense(out) and out.shape == (B, T, Cout)):
        raise ValueError("conv_taps_fwd: tap-major contiguous weights and [B,T,C] operands with dense batch strides")
    if (bias is not None and bias.numel() != Cout) or (R is not None and not (R.shape[-1] == Cout and R.numel() == B * T * Cout and R.stride(-1) == 1
                                                                         and (R.dim() == 2 or dense(R)))):
        raise ValueError("conv_taps_fwd: bias [Cout]; R [B*T, Cout] or [B,T,Cout] with dense batch strides")
    if x3d.dtype is not _F32 or Wp.dtype is not _F32 or out.dtype is not _F32 or not out.is_cuda:
        for t, n in ((x3d, "x"), (Wp, "W"), (out, "out"), (bias, "bias"), (R, "R")):
            _f32(t, n)
    check(lib().unast_conv_fwd(config.NSPLIT, _p(x3d), x3d.stride(1), _p(Wp), _p(out), out.stride(1), B, T, Cin, Cout, taps, pad_left,
                               _p(bias), act, _p(R), R.stride(-2) if R is not None else 0, _stream()), "unast_conv_fwd")
    return out


def maxpool_prev(x3d, out3d):
    """out[b,t] = max(x[b,t-1], x[b,t]) (out[b,0] = x[b,0])."""
    B, T, C = x3d.shape
    if not (out3d.shape == x3d.shape and x3d.stride(2) == 1 and out3d.stride(2) == 1 and x3d.stride(0) == T * x3d.stride(1)
            and out3d.stride(0) == T * out3d.stride(1)):
        raise ValueError("maxpool_prev: [B,T,C] operands of one shape with dense batch strides")
    _f32(x3d, "x"), _f32(out3d, "out")
    check(lib().unast_maxpool_prev(_p(x3d), x3d.stride(1), _p(out3d), out3d.stride(1), B, T, C, _stream()), "unast_maxpool_prev")
    return out3d


def highway_combine(ht, x, out):
    """ht [rows, 2C] = [linear | gate] pre-activations, out = relu(h) * sigmoid(t) + x * (1 - sigmoid(t)); out may be x."""
    rows, C = x.shape
    if not (tuple(ht.shape) == (rows, 2 * C) and out.shape == x.shape and ht.stride(1) == 1 and x.stride(1) == 1 and out.stride(1) == 1):
        raise ValueError("highway_combine: ht [rows, 2C], x and out [rows, C], unit column strides")
    _f32(ht, "ht"), _f32(x, "x"), _f32(out, "out")
    check(lib().unast_highway_combine(_p(ht), ht.stride(0), _p(x), x.stride(0), _p(out), out.stride(0), rows, C, _stream()), "unast_highway_combine")
    return out


def gru_fwd(xproj, whh, b_hn, y):
    """xproj [B,T,768] (input projections of both directions, b_ih + [b_hr, b_hz, 0] added), whh [2,384,128], b_hn [2,128], y [B,T,256]."""
    B, T = xproj.shape[0], xproj.shape[1]
    if not (xproj.is_contiguous() and whh.is_contiguous() and b_hn.is_contiguous() and y.is_contiguous() and xproj.shape[2] == 768
            and tuple(whh.shape) == (2, 384, 128) and tuple(y.shape) == (B, T, 256)):
        raise ValueError("gru_fwd: contiguous xproj [B,T,768], whh [2,384,128], b_hn [2,128], y [B,T,256]")
    for t, n in ((xproj, "xproj"), (whh, "whh"), (b_hn, "b_hn"), (y, "y")):
        _f32(t, n)
    check(lib().unast_gru_fwd(_p(xproj), _p(whh), _p(b_hn), _p(y), B, T, 128, _stream()), "unast_gru_fwd")
    return y


# ---- CBHG vocoder (training) -------------------------------------------------------------------------------
def _btc(t, B, T):
    """[B,T,C] with unit column stride and dense batch strides (a column slice of a wider buffer qualifies)."""
    return t.dim() == 3 and t.shape[0] == B and t.shape[1] == T and t.stride(2) == 1 and t.stride(0) == T * t.stride(1)


def gru_fwd_train(xproj, whh, b_hn, y, saved):
    """gru_fwd that also writes saved [B,T,2,512] = (r, z, n, W_hn h + b_hn) per step, direction and unit for gru_bwd."""
    B, T = xproj.shape[0], xproj.shape[1]
    if not (xproj.is_contiguous() and whh.is_contiguous() and b_hn.is_contiguous() and y.is_contiguous() and saved.is_contiguous()
            and xproj.dim() == 3 and xproj.shape[2] == 768 and tuple(whh.shape) == (2, 384, 128) and tuple(b_hn.shape) == (2, 128)
            and tuple(y.shape) == (B, T, 256) and tuple(saved.shape) == (B, T, 2, 512)):
        raise ValueError("gru_fwd_train: contiguous xproj [B,T,768], whh [2,384,128], b_hn [2,128], y [B,T,256], saved [B,T,2,512]")
    for t, n in ((xproj, "xproj"), (whh, "whh"), (b_hn, "b_hn"), (y, "y"), (saved, "saved")):
        _f32(t, n)
    check(lib().unast_gru_fwd_train(_p(xproj), _p(whh), _p(b_hn), _p(y), _p(saved), B, T, 128, _stream()), "unast_gru_fwd_train")
    return y


def gru_bwd(dy, y, saved, whh, dx_gates, dhn):
    """dy, y [B,T,256]; saved [B,T,2,512] from gru_fwd_train; whh [2,384,128] -> dx_gates [B,T,2,384] = (dr_pre, dz_pre, da), the gradient
    of xproj, and dhn [B,T,2,128] = r * da."""
    B, T = y.shape[0], y.shape[1]
    if not (dy.is_contiguous() and y.is_contiguous() and saved.is_contiguous() and whh.is_contiguous() and dx_gates.is_contiguous()
            and dhn.is_contiguous() and y.dim() == 3 and y.shape[2] == 256 and dy.shape == y.shape and tuple(saved.shape) == (B, T, 2, 512)
            and tuple(whh.shape) == (2, 384, 128) and tuple(dx_gates.shape) == (B, T, 2, 384) and tuple(dhn.shape) == (B, T, 2, 128)):
        raise ValueError("gru_bwd: contiguous dy, y [B,T,256], saved [B,T,2,512], whh [2,384,128], dx_gates [B,T,2,384], dhn [B,T,2,128]")
    for t, n in ((dy, "dy"), (y, "y"), (saved, "saved"), (whh, "whh"), (dx_gates, "dx_gates"), (dhn, "dhn")):
        _f32(t, n)
    check(lib().unast_gru_bwd(_p(dy), _p(y), _p(saved), _p(whh), _p(dx_gates), _p(dhn), B, T, 128, _stream()), "unast_gru_bwd")
    return dx_gates, dhn


def maxpool_prev_bwd(dy3d, x3d, dx3d, accumulate=False, relu_gate=False):
    """Backward of maxpool_prev (ties to the earlier frame); accumulate: dx += ; relu_gate: zero where x <= 0."""
    if x3d.dim() != 3:
        raise ValueError("maxpool_prev_bwd: [B,T,C] operands")
    B, T, C = x3d.shape
    if not (dy3d.shape == x3d.shape and dx3d.shape == x3d.shape and _btc(dy3d, B, T) and _btc(x3d, B, T) and _btc(dx3d, B, T)):
        raise ValueError("maxpool_prev_bwd: [B,T,C] operands of one shape with dense batch strides")
    _f32(dy3d, "dy"), _f32(x3d, "x"), _f32(dx3d, "dx")
    check(lib().unast_maxpool_prev_bwd(_p(dy3d), dy3d.stride(1), _p(x3d), x3d.stride(1), _p(dx3d), dx3d.stride(1), B, T, C,
                                       int(bool(accumulate)), int(bool(relu_gate)), _stream()), "unast_maxpool_prev_bwd")
    return dx3d


def relu_bwd(dy2d, y2d):
    """dy = dy where y > 0 else 0, in place."""
    if not (dy2d.dim() == 2 and dy2d.shape == y2d.shape and dy2d.stride(1) == 1 and y2d.stride(1) == 1):
        raise ValueError("relu_bwd: dy and y [rows, C], unit column strides")
    _f32(dy2d, "dy"), _f32(y2d, "y")
    check(lib().unast_relu_bwd(_p(dy2d), dy2d.stride(0), _p(y2d), y2d.stride(0), dy2d.shape[0], dy2d.shape[1], _stream()), "unast_relu_bwd")
    return dy2d


def highway_combine_bwd(dout, ht, x, dpre, dx):
    """Backward of highway_combine: dpre [rows, 2C] = gradient of ht, dx = dout * (1 - t) (dx may be dout)."""
    if x.dim() != 2:
        raise ValueError("highway_combine_bwd: x [rows, C]")
    rows, C = x.shape
    if not (tuple(ht.shape) == (rows, 2 * C) and tuple(dpre.shape) == (rows, 2 * C) and dout.shape == x.shape and dx.shape == x.shape
            and all(t.stride(1) == 1 for t in (dout, ht, x, dpre, dx))):
        raise ValueError("highway_combine_bwd: ht and dpre [rows, 2C], dout, x and dx [rows, C], unit column strides")
    for t, n in ((dout, "dout"), (ht, "ht"), (x, "x"), (dpre, "dpre"), (dx, "dx")):
        _f32(t, n)
    check(lib().unast_highway_combine_bwd(_p(dout), dout.stride(0), _p(ht), ht.stride(0), _p(x), x.stride(0), _p(dpre), dpre.stride(0),
                                          _p(dx), dx.stride(0), rows, C, _stream()), "unast_highway_combine_bwd")
    return dpre, dx


def sum_loss(pred2d, mag2d, dpred, l2, loss):
    """loss (float64 scalar tensor, zeroed by the caller) += sum |pred - mag| or sum (pred - mag)^2 over [rows, F]; dpred (or None)
    [rows, F] receives sign(diff) / 2 diff, and zeros in columns F .. ceil4(F) - 1 when its row stride has room for them."""
    if not (pred2d.dim() == 2 and mag2d.shape == pred2d.shape and pred2d.stride(1) == 1 and mag2d.stride(1) == 1
            and (dpred is None or (dpred.dim() == 2 and dpred.shape == pred2d.shape and dpred.stride(1) == 1 and dpred.stride(0) >= pred2d.shape[1]))):
        raise ValueError("sum_loss: pred, mag and dpred [rows, F] with unit column strides")
    if loss.dtype is not torch.float64 or loss.numel() != 1:
        raise ValueError("sum_loss: the loss accumulator is one float64")
    _f32(pred2d, "pred"), _f32(mag2d, "mag"), _f32(dpred, "dpred")
    if not loss.is_cuda:
        raise TypeError("sum_loss: the loss accumulator must live on the GPU")
    rows, F = pred2d.shape
    check(lib().unast_sum_loss(_p(pred2d), pred2d.stride(0), _p(mag2d), mag2d.stride(0), _p(dpred), dpred.stride(0) if dpred is not None else 0,
                               rows, F, int(bool(l2)), _p(loss), _stream()), "unast_sum_loss")
    return loss


def split_parts(x, hi=None, rest=None, resid=None):
    """The parts of x under the GEMM's split-bf16 operand preparation: hi = RNE_bf16(x), rest = x - hi, resid = rest - RNE_bf16(rest)
    (contiguous fp32 tensors of x's size; any of them may be None)."""
    outs = [t for t in (hi, rest, resid) if t is not None]
    if not outs or not x.is_contiguous() or any(not t.is_contiguous() or t.numel() != x.numel() for t in outs):
        raise ValueError("split_parts: contiguous tensors of one size, at least one output")
    for t, n in ((x, "x"), (hi, "hi"), (rest, "rest"), (resid, "resid")):
        _f32(t, n)
    check(lib().unast_split_parts(_p(x), _p(hi), _p(rest), _p(resid), x.numel(), _stream()), "unast_split_parts")


def _conv_grad_layout(name, dy3d, Wp, x3d, pad_left):
    if dy3d.dim() != 3 or x3d.dim() != 3 or Wp.dim() != 3:
        raise ValueError("%s: dy [B,T,Cout], x / dx [B,T,Cin], Wp [Cout,taps,Cin]" % name)
    B, T, Cout = dy3d.shape
    Cin = x3d.shape[2]
    taps = Wp.shape[1]
    if not (Wp.is_contiguous() and tuple(Wp.shape) == (Cout, taps, Cin) and 1 <= taps <= 16 and 0 <= pad_left < taps and _btc(dy3d, B, T) and _btc(x3d, B, T)
            and Cin % 4 == 0 and dy3d.stride(1) % 4 == 0 and x3d.stride(1) % 4 == 0):
        raise ValueError("%s: tap-major contiguous weights [Cout,1..16,Cin], [B,T,C] operands with dense batch strides, strides and Cin "
                         "multiples of 4" % name)
    for t, n in ((dy3d, "dy"), (Wp, "W"), (x3d, "x")):
        _f32(t, n)
    return B, T, Cin, Cout, taps


def conv_taps_dgrad(dy3d, Wp, dx3d, pad_left, beta=0):
    """Input gradient of conv_taps_fwd: dx[b,t,c] (+)= sum_{j,o} dy[b, t - j + pad_left, o] Wp[o,j,c]; operands may be column slices."""
    B, T, Cin, Cout, taps = _conv_grad_layout("conv_taps_dgrad", dy3d, Wp, dx3d, pad_left)
    if Cout % 4 != 0 or beta not in (0, 1):
        raise ValueError("conv_taps_dgrad: Cout %% 4 == 0 and beta 0 or 1")
    check(lib().unast_conv_dgrad(config.NSPLIT, _p(dy3d), dy3d.stride(1), _p(Wp), _p(dx3d), dx3d.stride(1), B, T, Cin, Cout, taps, pad_left,
                                 int(beta), _stream()), "unast_conv_dgrad")
    return dx3d


def conv_taps_wgrad(dy3d, x3d, dWp, pad_left, db=None):
    """dWp[o,j,c] += sum_{b,t} dy[b,t,o] x[b, t + j - pad_left, c]; db[o] += sum dy.  On the current stream."""
    if db is not None and not (db.numel() == dy3d.shape[-1] and db.is_contiguous()):
        raise ValueError("conv_taps_wgrad: db [Cout]")
    B, T, Cin, Cout, taps = _conv_grad_layout("conv_taps_wgrad", dy3d, dWp, x3d, pad_left)
    _f32(db, "db")
    sk = _splitk_for(Cout, taps * Cin, B * T)
    ws, ws_n = None, 0
    if sk > 1:
        ws_n = sk * Cout * taps * Cin
        ws = torch.empty(ws_n, dtype=torch.float32, device=dWp.device)
    check(lib().unast_conv_wgrad(config.NSPLIT, _p(dy3d), dy3d.stride(1), _p(x3d), x3d.stride(1), _p(dWp), B, T, Cin, Cout, taps, pad_left,
                                 _p(db), sk, _p(ws), ws_n, _stream()), "unast_conv_wgrad")
    return dWp


# ---- evaluation metrics (csrc/metrics.hip) -----------------------------------------------------------------
EDIT_THREADS, EDIT_CHUNK = 1024, 64                 # threads of the kernel's one workgroup, columns per thread chunk at most (the kernel's own: edit_distance_limits)
EDIT_MAX_COLS = EDIT_THREADS * EDIT_CHUNK           # ids the shorter side may hold (B * T)


def edit_distance_limits():
    out = (_ct.c_int * 2)()
    check(lib().unast_edit_distance_limits(_ct.addressof(out)), "unast_edit_distance_limits")
    return out[0], out[1]


def _ids_and_lens(name, ids, lens):
    if not (torch.is_tensor(ids) and ids.is_cuda and ids.dtype == torch.int64 and ids.dim() == 2):
        raise TypeError("edit_distance: %s must be an int64 CUDA tensor [B, T] (got %s)" % (name, (ids.dtype, tuple(ids.shape), str(ids.device)) if torch.is_tensor(ids) else type(ids)))
    if not (torch.is_tensor(lens) and lens.is_cuda and lens.dtype == torch.int32 and lens.is_contiguous() and tuple(lens.shape) == (ids.shape[0],)):
        raise TypeError("edit_distance: %s_len must be a contiguous int32 CUDA tensor [B]" % name)
    if ids.shape[1] > 1 and ids.stride(1) != 1 or ids.shape[0] > 1 and ids.stride(0) < ids.shape[1]:
        raise ValueError("edit_distance: %s needs unit column stride and a row stride of at least T" % name)


def edit_distance(ref, ref_len, hyp, hyp_len, out=None, ws=None, chunk=0):
    """out int32 [2] = {Levenshtein(flat(ref), flat(hyp)), len(flat(ref))} on the device; flat = each row's first len[b] ids in batch order.
    Raises ValueError before any launch when the shorter side could hold more than EDIT_MAX_COLS ids (min(B Tr, B Th))."""
    _ids_and_lens("ref", ref, ref_len)
    _ids_and_lens("hyp", hyp, hyp_len)
    B, Tr = ref.shape
    Th = hyp.shape[1]
    if hyp.shape[0] != B or B < 1:
        raise ValueError("edit_distance: ref and hyp need the same batch size >= 1 (got %d, %d)" % (B, hyp.shape[0]))
    if min(B * Tr, B * Th) > EDIT_MAX_COLS:
        raise ValueError("edit_distance: the shorter side holds up to %d ids; the kernel's limit is %d x %d" % (min(B * Tr, B * Th), EDIT_THREADS, EDIT_CHUNK))
    need = int(lib().unast_edit_distance_ws_bytes(B, Tr, Th))
    if ws is None:
        ws = torch.empty(max(need // 8, 1), dtype=torch.int64, device=ref.device)
    elif not (ws.is_cuda and ws.is_contiguous() and ws.numel() * ws.element_size() >= need):
        raise ValueError("edit_distance: the workspace needs %d bytes" % need)
    if out is None:
        out = torch.empty(2, dtype=torch.int32, device=ref.device)
    elif not (out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.numel() == 2):
        raise TypeError("edit_distance: out must be a contiguous int32 CUDA tensor [2]")
    check(lib().unast_edit_distance(_p(ref), ref.stride(0) if B > 1 else max(Tr, 1), _p(ref_len), Tr, _p(hyp), hyp.stride(0) if B > 1 else max(Th, 1), _p(hyp_len), Th, B,
                                    int(chunk), _p(ws), ws.numel() * ws.element_size(), _p(out), _stream()), "unast_edit_distance")
    return out


# ---- waveform synthesis (csrc/audio.hip) -------------------------------------------------------------------
STFT_SIZES = (256, 512, 1024, 2048)                 # n_fft the LDS FFT is built for
DEEMPH_CHUNK, DEEMPH_TILE = 16, 4096                # samples per thread and per workgroup tile of the de-preemphasis scan (the kernel's own constants)
_C64 = torch.complex64


def _audio_t(who, t, name, dtype, shape=None):
    kind = {_F32: "float32", _C64: "complex64", torch.int32: "int32"}[dtype]
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype):
        raise TypeError("%s: %s must be a %s CUDA tensor (got %s)" % (who, name, kind, (t.dtype, str(t.device)) if torch.is_tensor(t) else type(t)))
    if not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError("%s: %s must be contiguous%s (got %s)" % (who, name, "" if shape is None else " of shape %s" % (tuple(shape),), tuple(t.shape)))


def _stft_geometry(who, n_fft, hop, win):
    if n_fft not in STFT_SIZES:
        raise ValueError("%s: n_fft must be one of %s (got %r)" % (who, STFT_SIZES, n_fft))
    if not 1 <= win <= n_fft:
        raise ValueError("%s: win must be in 1..n_fft (win > n_fft has no centred padding; got win=%r, n_fft=%d)" % (who, win, n_fft))
    if hop < 1:
        raise ValueError("%s: hop must be positive (got %r)" % (who, hop))


def _rows_2d(who, t, name, min_cols):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == _F32):
        raise TypeError("%s: %s must be a float32 CUDA tensor (got %s)" % (who, name, (t.dtype, str(t.device)) if torch.is_tensor(t) else type(t)))
    if t.dim() != 2 or t.shape[1] < min_cols or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError("%s: %s must be [B, >= %d] with unit column stride (got %s)" % (who, name, min_cols, tuple(t.shape)))
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


def stft(y, frames, T_max, n_fft, hop, win, window, twiddle, spec, mag=None):
    """spec complex64 [B,T_max,1+n_fft/2] = the centred, reflect-padded STFT of y [B, >= hop (T_max-1)]; frames int32 [B].  With mag
    float32 [B,T_max,1+n_fft/2] the Griffin-Lim update mag * e / max(1e-8, |e|) is stored instead of e."""
    _stft_geometry("stft", n_fft, hop, win)
    F_ = n_fft // 2 + 1
    _audio_t("stft", frames, "frames", torch.int32)
    B = frames.numel()
    ld = _rows_2d("stft", y, "y", hop * (T_max - 1))
    _audio_t("stft", spec, "spec", _C64, (B, T_max, F_))
    _audio_t("stft", window, "window", _F32, (win,))
    _audio_t("stft", twiddle, "twiddle", _C64, (n_fft,))
    if mag is not None:
        _audio_t("stft", mag, "mag", _F32, (B, T_max, F_))
    if y.shape[0] != B:
        raise ValueError("stft: y has %d rows, frames %d" % (y.shape[0], B))
    check(lib().unast_stft(_p(y), ld, _p(frames), B, T_max, n_fft, hop, win, _p(window), _p(twiddle), _p(mag), _p(spec), _stream()), "unast_stft")
    return spec


def stft_momentum(y, frames, T_max, n_fft, hop, win, window, twiddle, spec, mag, alpha, tprev):
    """stft with the fast Griffin-Lim update (librosa.griffinlim) in its epilogue: with e the transform, c = e - alpha * tprev, then
    tprev <- e and spec <- mag * c / (|c| + 1e-16).  tprev complex64 [B,T_max,1+n_fft/2]; alpha = momentum / (1 + momentum) in [0, 0.5);
    alpha == 0 (the first iteration) does not read tprev."""
    _stft_geometry("stft_momentum", n_fft, hop, win)
    F_ = n_fft // 2 + 1
    _audio_t("stft_momentum", frames, "frames", torch.int32)
    B = frames.numel()
    ld = _rows_2d("stft_momentum", y, "y", hop * (T_max - 1))
    _audio_t("stft_momentum", spec, "spec", _C64, (B, T_max, F_))
    _audio_t("stft_momentum", tprev, "tprev", _C64, (B, T_max, F_))
    _audio_t("stft_momentum", mag, "mag", _F32, (B, T_max, F_))
    _audio_t("stft_momentum", window, "window", _F32, (win,))
    _audio_t("stft_momentum", twiddle, "twiddle", _C64, (n_fft,))
    if y.shape[0] != B:
        raise ValueError("stft_momentum: y has %d rows, frames %d" % (y.shape[0], B))
    if not 0.0 <= alpha < 0.5:
        raise ValueError("stft_momentum: alpha = momentum / (1 + momentum) must lie in [0, 0.5) (got %r)" % (alpha,))
    if tprev.data_ptr() == spec.data_ptr():
        raise ValueError("stft_momentum: tprev and spec are two buffers")
    check(lib().unast_stft_momentum(_p(y), ld, _p(frames), B, T_max, n_fft, hop, win, _p(window), _p(twiddle), _p(mag), alpha, _p(tprev), _p(spec), _stream()),
          "unast_stft_momentum")
    return spec


def gl_random_phase(M, frames, keys, seed, n_fft, twiddle, X0):
    """X0 complex64 [B,T,1+n_fft/2] = M * twiddle[m] for the frames t < frames[b], m a counter-based draw from (seed, keys[b], t, bin) over the
    n_fft levels of the twiddle table (include/unast_hip.h writes the function out).  keys: one uint32 per utterance, handed over as an int32 tensor [B] of the same bits."""
    _stft_geometry("gl_random_phase", n_fft, 1, n_fft)
    _audio_t("gl_random_phase", frames, "frames", torch.int32)
    B = frames.numel()
    _audio_t("gl_random_phase", M, "M", _F32)
    if M.dim() != 3 or M.shape[0] != B or M.shape[2] != n_fft // 2 + 1:
        raise ValueError("gl_random_phase: M must be [B, T, %d] with B = len(frames) (got %s)" % (n_fft // 2 + 1, tuple(M.shape)))
    _audio_t("gl_random_phase", X0, "X0", _C64, M.shape)
    _audio_t("gl_random_phase", twiddle, "twiddle", _C64, (n_fft,))
    if not (torch.is_tensor(keys) and keys.is_cuda and keys.dtype == torch.int32 and keys.is_contiguous() and tuple(keys.shape) == (B,)):
        raise TypeError("gl_random_phase: keys must be a contiguous int32 CUDA tensor [B] (the uint32 keys' bit patterns)")
    if not 0 <= int(seed) < 1 << 32:
        raise ValueError("gl_random_phase: seed must fit 32 bits (got %r)" % (seed,))
    check(lib().unast_gl_random_phase(_p(M), _p(frames), _p(keys), int(seed), B, M.shape[1], n_fft, _p(twiddle), _p(X0), _stream()), "unast_gl_random_phase")
    return X0


def istft_frames(spec, frames, n_fft, win, window, twiddle, fr):
    """fr float32 [B,T_max,win] = window * irfft(spec[b,t])[(n_fft-win)/2 : (n_fft-win)/2 + win] for t < frames[b]."""
    _stft_geometry("istft_frames", n_fft, 1, win)
    _audio_t("istft_frames", frames, "frames", torch.int32)
    _audio_t("istft_frames", spec, "spec", _C64)
    if spec.dim() != 3 or spec.shape[0] != frames.numel() or spec.shape[2] != n_fft // 2 + 1:
        raise ValueError("istft_frames: spec must be [B, T, %d] with B = len(frames) (got %s)" % (n_fft // 2 + 1, tuple(spec.shape)))
    B, T_max = spec.shape[0], spec.shape[1]
    _audio_t("istft_frames", fr, "fr", _F32, (B, T_max, win))
    _audio_t("istft_frames", window, "window", _F32, (win,))
    _audio_t("istft_frames", twiddle, "twiddle", _C64, (n_fft,))
    check(lib().unast_istft_frames(_p(spec), _p(frames), B, T_max, n_fft, win, _p(window), _p(twiddle), _p(fr), _stream()), "unast_istft_frames")
    return fr


def overlap_add(fr, frames, n_fft, hop, window, y):
    """y [B, >= hop (T_max-1)] = the frames fr [B,T_max,win] overlap-added and divided by the window's sum of squares (a gather, no atomics)."""
    _audio_t("overlap_add", fr, "fr", _F32)
    if fr.dim() != 3:
        raise ValueError("overlap_add: fr must be [B, T, win] (got %s)" % (tuple(fr.shape),))
    B, T_max, win = fr.shape
    _stft_geometry("overlap_add", n_fft, hop, win)
    _audio_t("overlap_add", frames, "frames", torch.int32, (B,))
    _audio_t("overlap_add", window, "window", _F32, (win,))
    ld = _rows_2d("overlap_add", y, "y", hop * (T_max - 1))
    if y.shape[0] != B:
        raise ValueError("overlap_add: y has %d rows, fr %d" % (y.shape[0], B))
    check(lib().unast_overlap_add(_p(fr), _p(frames), B, T_max, n_fft, hop, win, _p(window), _p(y), ld, _stream()), "unast_overlap_add")
    return y


def gl_prepare(mag, max_db, ref_db, power, M, X0=None):
    """M = (10 ** (0.05 * (clip(mag, 0, 1) * max_db - max_db + ref_db))) ** power for mag [..., F] with unit column stride and one row stride
    (a view of a padded buffer qualifies); X0 (complex64, optional) = M + 0j."""
    if not (torch.is_tensor(mag) and mag.is_cuda and mag.dtype == _F32):
        raise TypeError("gl_prepare: mag must be a float32 CUDA tensor (got %s)" % ((mag.dtype, str(mag.device)) if torch.is_tensor(mag) else type(mag),))
    if mag.dim() < 2 or mag.numel() == 0:
        raise ValueError("gl_prepare: mag must be [..., rows, F], not empty")
    F_ = mag.shape[-1]
    rows = mag.numel() // F_
    ld = mag.stride(-2) if rows > 1 else F_
    one_row_stride = all(mag.shape[i] == 1 or mag.stride(i) == mag.stride(i + 1) * mag.shape[i + 1] for i in range(mag.dim() - 2))
    if (F_ > 1 and mag.stride(-1) != 1) or ld < F_ or not one_row_stride:
        raise ValueError("gl_prepare: mag needs unit column stride and one row stride (got shape %s, strides %s)" % (tuple(mag.shape), mag.stride()))
    _audio_t("gl_prepare", M, "M", _F32, mag.shape)
    if X0 is not None:
        _audio_t("gl_prepare", X0, "X0", _C64, mag.shape)
    check(lib().unast_gl_prepare(_p(mag), ld, rows, F_, max_db, ref_db, power, _p(M), _p(X0), _stream()), "unast_gl_prepare")
    return M


def deemphasis(x, lens, coef, y):
    """y[b,k] = x[b,k] + coef * y[b,k-1] over the first lens[b] samples of each row of x [B,n]; y may be x."""
    _audio_t("deemphasis", lens, "lens", torch.int32)
    ldx = _rows_2d("deemphasis", x, "x", 0)
    ldy = _rows_2d("deemphasis", y, "y", 0)
    if x.shape != y.shape or x.shape[0] != lens.numel() or x.shape[1] < 1:
        raise ValueError("deemphasis: x and y [B, n >= 1] of one shape, lens [B]")
    if not -1.0 < coef < 1.0:
        raise ValueError("deemphasis: |coef| must be below 1 (got %r)" % coef)
    check(lib().unast_deemphasis(_p(x), ldx, _p(y), ldy, _p(lens), x.shape[0], coef, _stream()), "unast_deemphasis")
    return y


def trim_bounds(y, lens, top_db, frame_length, hop_length, pad_mode, out=None):
    """out int32 [B,2] = (start, end) of librosa.effects.trim for each row of y [B,n] with lens[b] samples; pad_mode 'reflect' or 'constant'."""
    if pad_mode not in ("reflect", "constant"):
        raise ValueError("trim_bounds: pad_mode is 'reflect' (librosa 0.8) or 'constant' (later versions), got %r" % (pad_mode,))
    _audio_t("trim_bounds", lens, "lens", torch.int32)
    ld = _rows_2d("trim_bounds", y, "y", 1)
    B, n_max = y.shape
    if lens.numel() != B or frame_length < 2 or hop_length < 1 or top_db <= 0:
        raise ValueError("trim_bounds: lens [B], frame_length >= 2, hop_length >= 1, top_db > 0")
    if out is None:
        out = torch.empty(B, 2, dtype=torch.int32, device=y.device)
    else:
        _audio_t("trim_bounds", out, "out", torch.int32, (B, 2))
    ws = torch.empty(B * (1 + n_max // hop_length), dtype=_F32, device=y.device)
    check(lib().unast_trim_bounds(_p(y), ld, _p(lens), B, n_max, top_db, frame_length, hop_length, 0 if pad_mode == "reflect" else 1, _p(ws), ws.numel(),
                                  _p(out), _stream()), "unast_trim_bounds")
    return out


def preemphasis(x, lens, coef, y, start=None):
    """y[b, start[b] + k] = x[b, start[b] + k] - coef * x[b, start[b] + k - 1] (the raw sample at k = 0) for k < lens[b], numpy's float32
    result bit for bit (src/utils.py:251); x, y [B, n] distinct, lens / start int32 [B] (start optional: zeros)."""
    _audio_t("preemphasis", lens, "lens", torch.int32)
    if start is not None:
        _audio_t("preemphasis", start, "start", torch.int32, (lens.numel(),))
    ldx = _rows_2d("preemphasis", x, "x", 1)
    ldy = _rows_2d("preemphasis", y, "y", 1)
    if x.shape != y.shape or x.shape[0] != lens.numel():
        raise ValueError("preemphasis: x and y [B, n >= 1] of one shape, lens [B]")
    if x.data_ptr() == y.data_ptr():
        raise ValueError("preemphasis: not in place: sample k reads sample k - 1 of the input")
    check(lib().unast_preemphasis(_p(x), ldx, _p(y), ldy, x.shape[1], _p(start), _p(lens), x.shape[0], coef, _stream()), "unast_preemphasis")
    return y


def features(y, start, samples, T_max, n_fft, hop, win, coef, window, twiddle, basis, ranges, ref_db, max_db, mel, mag, spec=None):
    """get_spectrograms (src/utils.py:251-276) in one launch: utterance b = y[b, start[b] : start[b] + samples[b]] (start optional) ->
    mel float32 [B,T_max,n_mels] and mag float32 [B,T_max,1+n_fft/2], normalised, for its 1 + samples[b] // hop frames; spec (complex64, same
    shape as mag; optional) receives the spectrum of the emphasised signal.  basis float32 [n_mels, 1+n_fft/2], ranges int32 [n_mels, 2]."""
    _stft_geometry("features", n_fft, hop, win)
    if hop > win:
        raise ValueError("features: hop must not exceed win (got hop=%r, win=%r)" % (hop, win))
    F_ = n_fft // 2 + 1
    _audio_t("features", samples, "samples", torch.int32)
    B = samples.numel()
    if start is not None:
        _audio_t("features", start, "start", torch.int32, (B,))
    ld = _rows_2d("features", y, "y", n_fft // 2 + 1)
    if y.shape[0] != B:
        raise ValueError("features: y has %d rows, samples %d" % (y.shape[0], B))
    _audio_t("features", basis, "basis", _F32)
    if basis.dim() != 2 or basis.shape[0] < 1 or basis.shape[1] != F_:
        raise ValueError("features: basis must be [n_mels >= 1, %d] (got %s)" % (F_, tuple(basis.shape)))
    n_mels = basis.shape[0]
    _audio_t("features", ranges, "ranges", torch.int32, (n_mels, 2))
    _audio_t("features", window, "window", _F32, (win,))
    _audio_t("features", twiddle, "twiddle", _C64, (n_fft,))
    _audio_t("features", mel, "mel", _F32, (B, T_max, n_mels))
    _audio_t("features", mag, "mag", _F32, (B, T_max, F_))
    if spec is not None:
        _audio_t("features", spec, "spec", _C64, (B, T_max, F_))
    check(lib().unast_features(_p(y), ld, y.shape[1], _p(start), _p(samples), B, T_max, n_fft, hop, win, coef, _p(window), _p(twiddle), _p(basis), _p(ranges),
                               n_mels, ref_db, max_db, _p(mel), _p(mag), _p(spec), _stream()), "unast_features")
    return mel, mag


# ---- optimizer ---------------------------------------------------------------------------------------------
_MSE_WS = {}


def masked_mse(gold, pred, mask):
    """src/train.py:100-103 on flat fp32 tensors; returns a device scalar.  The kernel's workspace (two sums and an arrival counter,
    zero on entry, left zero) is one per (device, stream): calls on different streams may overlap, calls on one stream are ordered."""
    dev = gold.device
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = _MSE_WS.get(key)
    if ws is None:
        ws = _MSE_WS[key] = torch.zeros(3, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)                  # filled once: nobody may run ahead of the fill
    if config.DEBUG_WORKSPACES and bool((ws != 0).any()):
        raise RuntimeError("masked_mse: workspace not zero on entry (an earlier call on this stream died midway?)")
    out = torch.empty((), dtype=torch.float32, device=dev)
    check(lib().unast_masked_mse(_p(gold), _p(pred), _p(mask), gold.numel(), _p(ws), _p(out), _stream()), "unast_masked_mse")
    return out


def sumsq(g, out):
    check(lib().unast_sumsq(_p(g), g.numel(), _p(out), _stream()), "unast_sumsq")


def scalar_combine(xs, div, out):
    """out = (xs[0] + xs[1] + xs[2]) / div over 1 to 3 device scalars."""
    a = xs[0]
    b = xs[1] if len(xs) > 1 else None
    c = xs[2] if len(xs) > 2 else None
    check(lib().unast_scalar_combine(_p(a), _p(b), _p(c), float(div), _p(out), _stream()), "unast_scalar_combine")
    return out


def adamw(p, g, m, v, sumsq_scalar, max_norm, lr, beta1, beta2, eps, wd, step, split_out=None, decoupled=True, dev_hyper=None, zero_grad=False):
    """dev_hyper: float32 [3] device tensor {lr, 1 - beta1^t, sqrt(1 - beta2^t)} read by the kernel instead of lr / step."""
    check(lib().unast_adamw(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(sumsq_scalar), max_norm, lr, beta1, beta2, eps, wd, step,
                            _p(split_out), int(bool(decoupled)), _p(dev_hyper), int(bool(zero_grad)), _stream()), "unast_adamw")


def adam_hyper(lr, beta1, beta2, step):
    """The three floats unast_adamw derives from (lr, step) on the host -- {lr, 1 - beta1^t, sqrt(1 - beta2^t)} with the betas
    rounded to fp32 first, as the C entry point receives them -- for the device-resident block a captured step reads."""
    import ctypes
    import math
    b1, b2 = ctypes.c_float(beta1).value, ctypes.c_float(beta2).value
    return [float(lr), 1.0 - b1 ** int(step), math.sqrt(1.0 - b2 ** int(step))]


def transpose_split(src_flat, dst_flat, tiles_i32, ntiles):
    check(lib().unast_transpose_split(_p(src_flat), _p(dst_flat), _p(tiles_i32), ntiles, _stream()), "unast_transpose_split")


def split_f32(src, dst):
    """dst = src in the GEMM's pre-split operand format (16-B chunks [hi x4 | lo x4] of bf16; same byte offsets)."""
    check(lib().unast_split_f32(_p(src), _p(dst), src.numel(), _stream()), "unast_split_f32")


_STEP_STATE = {}
STEP_STATE_WORDS = 64


def step_state():
    """Per-device block of 64 32-bit words in device memory that captured (HIP-graph) work reads at replay time:
    word 0 = the RNG epoch mixed into every dropout / noise stream (unast_set_rng_epoch), words 4.. = float triples
    {lr, 1 - beta1^t, sqrt(1 - beta2^t)} for unast_adamw's dev_hyper.  One small host-to-device copy refreshes all of it."""
    dev = torch.cuda.current_device()
    c = _STEP_STATE.get(dev)
    if c is None:
        torch.cuda.synchronize()
        c = torch.zeros(STEP_STATE_WORDS, dtype=torch.int32, device="cuda:%d" % dev)
        torch.cuda.synchronize()
        check(lib().unast_set_rng_epoch(c.data_ptr()), "unast_set_rng_epoch")
        _STEP_STATE[dev] = c
    return c


def rng_epoch_counter():
    """The device counter mixed into every dropout / noise stream (unast_set_rng_epoch): int32 [1], 0 outside graph replay."""
    return step_state()[0:1]


def set_step_state(epoch, hyper_by_slot):
    """One tiny launch: RNG epoch (word 0) and the hyper-parameter triples {slot: [lr, bc1, bc2_sqrt]} (words 4 + 3*slot ..)."""
    import ctypes
    import struct
    words = (ctypes.c_uint * 16)()
    words[0] = epoch & 0xFFFFFFFF
    n = 4
    for slot, vals in hyper_by_slot.items():
        if 4 + 3 * slot + 3 > 16:
            raise ValueError("set_step_state: at most 4 optimizer ranges")
        for j, v in enumerate(vals):
            words[4 + 3 * slot + j] = struct.unpack("<I", struct.pack("<f", float(v)))[0]
        n = max(n, 4 + 3 * slot + 3)
    check(lib().unast_set_words(_p(step_state()), ctypes.addressof(words), n, _stream()), "unast_set_words")


def hyper_slot(i):
    """float32 [3] view of the i-th optimizer hyper-parameter triple inside step_state()."""
    return step_state().view(torch.float32)[4 + 3 * i: 7 + 3 * i]
