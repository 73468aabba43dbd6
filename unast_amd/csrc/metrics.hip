// Evaluation metrics on the device: the Levenshtein distance behind compute_per (src/utils.py:24-34; jiwer 2.2.0 flattens both sentence
// lists into one id sequence each and takes ONE distance over them), so that evaluate() keeps its only quadratic piece off the host.
//
// One workgroup, one launch.  Prologue: both batches are flattened (each row's first len[b] ids, batch order) into the caller's workspace.
// Sweep: the shorter flattened sequence lies on the DP's columns, CH consecutive columns per thread in registers; the longer one is walked row
// by row.  The state is kept as q[j] = D[i][j] - j, in which the insertion chain D[i][j] = min(t[j], D[i][j-1] + 1) is a plain prefix minimum
// (unast_amd.utils.edit_distance resolves it the same way): per-thread scan, wave scan over lanes, wave totals through LDS -- one barrier per
// row, the totals double-buffered by row parity.  A thread's exclusive prefix minimum IS the finished q of the column left of its chunk, i.e.
// the diagonal neighbour of its first column in the next row: no second exchange.
// No atomics, no cooperative launch, no wait across workgroups (there is one), integer arithmetic in a fixed order: two runs give the same bits.
#include "common.h"

namespace {

constexpr int ED_THREADS = 1024;     // threads of the workgroup at most (16 waves)
constexpr int ED_CHUNK = 64;         // columns per thread at most
constexpr int ED_WAVES = ED_THREADS / UNAST_WAVE;
constexpr int ED_INF = 0x3FFFFFFF;

struct EdArgs {
    const long long* ref; const long long* hyp;
    const int* ref_len; const int* hyp_len;
    long long ld_ref, ld_hyp;
    int Tr, Th, B, chunk;
    long long* flat_ref; long long* flat_hyp;       // workspace: B*Tr and B*Th ids
    int* out;
};

// flat[0 .. total) = each row's first clamp(len[b], 0, T) ids in batch order; every thread walks the same rows, so all of them return the
// total.  Nothing at or behind len[b] is read.  wide: some copied id does not fit 32 bits.
__device__ __forceinline__ int ed_flatten(const long long* ids, long long ld, const int* lens, int B, int T, long long* flat, bool& wide) {
    int off = 0;
    for (int b = 0; b < B; ++b) {
        const int len = min(max(lens[b], 0), T);
        for (int t = threadIdx.x; t < len; t += blockDim.x) {
            const long long v = ids[b * ld + t];
            wide |= v != (long long)(int)v;
            flat[off + t] = v;
        }
        off += len;
    }
    return off;
}

template <int CH, bool WIDE>
__device__ void ed_sweep(const long long* __restrict__ cols, int m, const long long* __restrict__ rows, int n, int* s_tot, int* out) {
    const int tid = threadIdx.x, lane = tid & (UNAST_WAVE - 1), wave = tid >> 6;
    const int j0 = tid * CH;                        // first column of the chunk (0-based position in cols; DP column j0 + 1)
    const bool active = j0 < m;
    int lo[CH], hi[WIDE ? CH : 1], q[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const long long v = j0 + c < m ? cols[j0 + c] : 0ll;      // columns at or behind m decide nothing to their left
        lo[c] = (int)v;
        if (WIDE) hi[c] = (int)(v >> 32);
        q[c] = 0;                                   // row 0: D[0][j] = j
    }
    int left0 = 0;                                  // q of the column left of the chunk in the previous row
    // The row ids reach every wave 64 at a time (lane l holds row i0 + l, one coalesced load a block ahead) and are read out lane by lane.
    long long blk = lane < n ? rows[lane] : 0ll;
    for (int i0 = 0; i0 < n; i0 += UNAST_WAVE) {
        const long long blk_next = i0 + UNAST_WAVE + lane < n ? rows[i0 + UNAST_WAVE + lane] : 0ll;
        const int blo = (int)blk, bhi = (int)(blk >> 32);
        const int kn = min(UNAST_WAVE, n - i0);
        for (int k = 0; k < kn; ++k) {
            const int i = i0 + k + 1;
            const int rlo = __builtin_amdgcn_readlane(blo, k), rhi = WIDE ? __builtin_amdgcn_readlane(bhi, k) : 0;
            int tmin = ED_INF;
            if (active) {
                int left = left0;
#pragma unroll
                for (int c = 0; c < CH; ++c) {      // deletion and substitution: t[j] - j = min(q_prev[j] + 1, q_prev[j-1] - 1 + (col != row))
                    const bool ne = WIDE ? (lo[c] != rlo) | (hi[c] != rhi) : lo[c] != rlo;
                    const int u = min(q[c] + 1, left - 1 + (ne ? 1 : 0));
                    left = q[c];
                    q[c] = u;
                    tmin = min(tmin, u);
                }
            }
            int x = tmin;                           // inclusive prefix minimum over the lanes of the wave
#pragma unroll
            for (int d = 1; d < UNAST_WAVE; d <<= 1) {
                const int y = __shfl_up(x, d, UNAST_WAVE);
                if (lane >= d) x = min(x, y);
            }
            int excl = __shfl_up(x, 1, UNAST_WAVE);
            if (lane == 0) excl = ED_INF;
            int* tot = s_tot + (i & 1) * ED_WAVES;  // double-buffered by row parity: one barrier per row
            if (lane == UNAST_WAVE - 1) tot[wave] = x;
            __syncthreads();
            int carry = min(i, excl);               // column 0: D[i][0] - 0 = i
#pragma unroll
            for (int w = 0; w < ED_WAVES; ++w) {
                const int v = tot[w];
                if (w < wave) carry = min(carry, v);
            }
            if (active) {
                int run = carry;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    run = min(run, q[c]);
                    q[c] = run;
                }
            }
            left0 = carry;
        }
        blk = blk_next;
    }
    if (tid == (m - 1) / CH) {
        const int cm = (m - 1) % CH;
        int v = 0;
#pragma unroll
        for (int c = 0; c < CH; ++c)
            if (c == cm) v = q[c];
        out[0] = v + m;
    }
}

template <bool WIDE>
__device__ __forceinline__ void ed_dispatch(int ch, const long long* cols, int m, const long long* rows, int n, int* s_tot, int* out) {
    switch (ch) {
        case 1: ed_sweep<1, WIDE>(cols, m, rows, n, s_tot, out); break;
        case 2: ed_sweep<2, WIDE>(cols, m, rows, n, s_tot, out); break;
        case 4: ed_sweep<4, WIDE>(cols, m, rows, n, s_tot, out); break;
        case 8: ed_sweep<8, WIDE>(cols, m, rows, n, s_tot, out); break;
        case 16: ed_sweep<16, WIDE>(cols, m, rows, n, s_tot, out); break;
        case 32: ed_sweep<32, WIDE>(cols, m, rows, n, s_tot, out); break;
        default: ed_sweep<ED_CHUNK, WIDE>(cols, m, rows, n, s_tot, out); break;
    }
}

__global__ void __launch_bounds__(ED_THREADS) edit_distance_kernel(EdArgs a) {
    __shared__ int s_tot[2 * ED_WAVES];
    bool wide = false;
    const int n_ref = ed_flatten(a.ref, a.ld_ref, a.ref_len, a.B, a.Tr, a.flat_ref, wide);
    const int n_hyp = ed_flatten(a.hyp, a.ld_hyp, a.hyp_len, a.B, a.Th, a.flat_hyp, wide);
    __threadfence();                                // the flattened ids are read back by other threads of this workgroup
    __syncthreads();
    const int any_wide = __syncthreads_or(wide ? 1 : 0);
    if (threadIdx.x == 0) a.out[1] = n_ref;
    const bool swap = n_ref < n_hyp;                // the distance is symmetric: the shorter sequence goes on the columns
    const int m = swap ? n_ref : n_hyp, n = swap ? n_hyp : n_ref;
    if (m == 0) {                                   // uniform: before any barrier of the sweep
        if (threadIdx.x == 0) a.out[0] = n;
        return;
    }
    const long long* cols = swap ? a.flat_ref : a.flat_hyp;
    const long long* rows = swap ? a.flat_hyp : a.flat_ref;
    int ch = 1;                                     // the smallest chunk with which this workgroup covers m columns, or the caller's larger one
    while (ch < ED_CHUNK && (long long)ch * blockDim.x < m) ch <<= 1;
    ch = max(ch, a.chunk);
    if (any_wide) ed_dispatch<true>(ch, cols, m, rows, n, s_tot, a.out);
    else ed_dispatch<false>(ch, cols, m, rows, n, s_tot, a.out);
}

}  // namespace

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------
extern "C" int unast_edit_distance_limits(int* out2) {
    UNAST_REQUIRE(out2, "unast_edit_distance_limits: null pointer");
    out2[0] = ED_THREADS;
    out2[1] = ED_CHUNK;
    return UNAST_OK;
}

extern "C" int64_t unast_edit_distance_ws_bytes(int B, int Tr, int Th) {
    if (B < 0 || Tr < 0 || Th < 0) return -1;
    return ((int64_t)B * Tr + (int64_t)B * Th) * (int64_t)sizeof(long long);
}

extern "C" int unast_edit_distance(const int64_t* ref, int64_t ld_ref, const int* ref_len, int Tr, const int64_t* hyp, int64_t ld_hyp,
                                   const int* hyp_len, int Th, int B, int chunk, void* ws, int64_t ws_bytes, int* out2, hipStream_t stream) {
    UNAST_REQUIRE(B >= 1 && Tr >= 0 && Th >= 0 && ref_len && hyp_len && out2, "unast_edit_distance: need B >= 1, Tr, Th >= 0, lengths and out (B=%d Tr=%d Th=%d)", B, Tr, Th);
    UNAST_REQUIRE((ref || Tr == 0) && (hyp || Th == 0) && ld_ref >= Tr && ld_hyp >= Th, "unast_edit_distance: null ids or a row stride below the row length");
    const long long cap_ref = (long long)B * Tr, cap_hyp = (long long)B * Th;
    UNAST_REQUIRE(cap_ref <= (1ll << 30) && cap_hyp <= (1ll << 30), "unast_edit_distance: B*T must not exceed 2^30 ids per side");
    const long long cap_cols = cap_ref < cap_hyp ? cap_ref : cap_hyp;
    UNAST_REQUIRE(cap_cols <= (long long)ED_THREADS * ED_CHUNK,
                  "unast_edit_distance: the shorter side holds up to %lld ids, the limit is %d (threads) x %d (columns per thread)", cap_cols, ED_THREADS, ED_CHUNK);
    UNAST_REQUIRE(chunk == 0 || (chunk >= 1 && chunk <= ED_CHUNK && (chunk & (chunk - 1)) == 0), "unast_edit_distance: chunk is 0 or a power of two up to %d (got %d)", ED_CHUNK, chunk);
    UNAST_REQUIRE(ws_bytes >= unast_edit_distance_ws_bytes(B, Tr, Th) && (ws || ws_bytes == 0) && (((uintptr_t)ws) & 7) == 0,
                  "unast_edit_distance: the workspace needs unast_edit_distance_ws_bytes(B, Tr, Th) bytes, 8-byte aligned");
    EdArgs a;
    a.ref = (const long long*)ref; a.hyp = (const long long*)hyp; a.ref_len = ref_len; a.hyp_len = hyp_len; a.ld_ref = ld_ref; a.ld_hyp = ld_hyp;
    a.Tr = Tr; a.Th = Th; a.B = B; a.chunk = chunk;
    a.flat_ref = (long long*)ws; a.flat_hyp = (long long*)ws + cap_ref; a.out = out2;
    long long threads = (cap_cols + UNAST_WAVE - 1) / UNAST_WAVE * UNAST_WAVE;      // a workgroup no wider than the columns can need
    if (threads < UNAST_WAVE) threads = UNAST_WAVE;
    if (threads > ED_THREADS) threads = ED_THREADS;
    hipLaunchKernelGGL(edit_distance_kernel, dim3(1), dim3((unsigned)threads), 0, stream, a);
    return unast_check_launch("unast_edit_distance");
}
