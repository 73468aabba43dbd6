// The prefix prenet of TextRNN's teacher-forced decoder training (src/network.py:546-575): TextPrenet runs over the whole prefix at every
// position, each call with its own batch statistics.  All prefixes lie in ONE slab of rows (unast_amd.train_rnn.prefix_layout):
//
//   segment s = 0..T-1 holds B sequences of L_s = max(s, 1) live rows, each followed by TWO gap rows:   row(s, b, j) = off[s] + b (L_s + 2) + j
//
// so that the 5-tap convolutions run over the slab as one long sequence (the gaps are every neighbour's zero padding) and only the
// BatchNorm stages and the embedding need to know the segments.  This file holds those: statistics per segment, gap rows written as exact
// zeros, stage 3 reduced to each prefix's last row.
//
// Work is cut into CHUNKS of at most 64 slab rows that never straddle a segment (table built on the host: {segment, first row}); a segment
// of 2 rows is one short chunk, one of B*513 rows is spread over hundreds of workgroups.  Sums go chunk -> segment in two launches with a fixed
// order and no atomics (fp64 throughout), so two runs give the same bits.
#include "common.h"

#define PFX_CHUNK 64

struct PfxSeg { int s, off, L, st, end; };
__device__ __forceinline__ PfxSeg pfx_seg(const int* __restrict__ segoff, int s) {
    PfxSeg g;
    g.s = s; g.off = segoff[s]; g.end = segoff[s + 1]; g.L = s > 0 ? s : 1; g.st = g.L + 2;
    return g;
}

// fixed-order reduction of the row lanes of a workgroup: thread (ty, tx) holds 2 x 4 doubles for channel quad tx
__device__ __forceinline__ void pfx_block_reduce(double (*red)[256][4], const double* a, const double* q, int C, int cq, int nry, double* __restrict__ out) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[0][threadIdx.x][e] = a[e]; red[1][threadIdx.x][e] = q[e]; }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        const int qd = c >> 2, e = c & 3;
        double sa = 0.0, sq = 0.0;
        for (int yy = 0; yy < nry; ++yy) { sa += red[0][yy * cq + qd][e]; sq += red[1][yy * cq + qd][e]; }
        out[c] = sa;
        out[C + c] = sq;
    }
}

// ---- forward statistics ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pfx_stats_part_kernel(const float* __restrict__ x, const int* __restrict__ chunks, const int* __restrict__ segoff,
                                                             int C, double* __restrict__ part) {
    __shared__ double red[2][256][4];
    const int cq = C >> 2, nry = 256 / cq;
    const int tx = threadIdx.x % cq, ty = threadIdx.x / cq;
    const PfxSeg g = pfx_seg(segoff, chunks[2 * blockIdx.x]);
    const int r0 = chunks[2 * blockIdx.x + 1], r1 = min(r0 + PFX_CHUNK, g.end);
    double a[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
    if (ty < nry) {
        for (int r = r0 + ty; r < r1; r += nry) {
            if ((r - g.off) % g.st >= g.L) continue;                       // a gap row: not read
            const float4 v = *reinterpret_cast<const float4*>(x + (size_t)r * C + tx * 4);
            const double d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) { a[e] += d[e]; q[e] += d[e] * d[e]; }
        }
    }
    pfx_block_reduce(red, a, q, C, cq, nry, part + (size_t)blockIdx.x * 2 * C);
}

// one workgroup per segment: chunk partials in order -> mean, rstd (biased variance), the unbiased variance for the running statistics
__global__ __launch_bounds__(256) void pfx_stats_final_kernel(const double* __restrict__ part, const int* __restrict__ chunk_start, int B, int C, float eps,
                                                              float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ varu) {
    const int s = blockIdx.x;
    const double n = (double)B * (s > 0 ? s : 1);
    for (int c = threadIdx.x; c < C; c += 256) {
        double s1 = 0.0, s2 = 0.0;
        for (int k = chunk_start[s]; k < chunk_start[s + 1]; ++k) { s1 += part[(size_t)k * 2 * C + c]; s2 += part[(size_t)k * 2 * C + C + c]; }
        const double mu = s1 / n;
        double var = s2 / n - mu * mu;
        if (var < 0.0) var = 0.0;
        mean[(size_t)s * C + c] = (float)mu;
        rstd[(size_t)s * C + c] = (float)(1.0 / sqrt(var + (double)eps));
        varu[(size_t)s * C + c] = (float)(n > 1.0 ? var * n / (n - 1.0) : var);
    }
}

// T momentum updates in segment order, fp32 as unast_bn_fwd's; num_batches_tracked += T
__global__ __launch_bounds__(256) void pfx_running_kernel(const float* __restrict__ mean, const float* __restrict__ varu, int T, int C, float momentum,
                                                          float* __restrict__ running_mean, float* __restrict__ running_var, long long* __restrict__ nbt) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) {
        float rm = running_mean[c], rv = running_var[c];
        for (int s = 0; s < T; ++s) {
            rm = (1.f - momentum) * rm + momentum * mean[(size_t)s * C + c];
            rv = (1.f - momentum) * rv + momentum * varu[(size_t)s * C + c];
        }
        running_mean[c] = rm;
        running_var[c] = rv;
    }
    if (nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt += T;
}

// y = dropout(relu((x - mean_s) rstd_s gamma + beta)) on live rows, exact zeros on gap rows; the mask's row index is the slab row
__global__ __launch_bounds__(256) void pfx_apply_kernel(const float* __restrict__ x, const int* __restrict__ chunks, const int* __restrict__ segoff,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ y, int C, uint32_t drop_thresh, float drop_scale,
                                                        uint32_t seed, uint32_t stream) {
    const int cq = C >> 2, nry = 256 / cq;
    const int tx = threadIdx.x % cq, ty = threadIdx.x / cq;
    if (ty >= nry) return;
    const PfxSeg g = pfx_seg(segoff, chunks[2 * blockIdx.x]);
    const int r0 = chunks[2 * blockIdx.x + 1], r1 = min(r0 + PFX_CHUNK, g.end);
    const int c = tx * 4;
    const float4 m = *reinterpret_cast<const float4*>(mean + (size_t)g.s * C + c), rs = *reinterpret_cast<const float4*>(rstd + (size_t)g.s * C + c);
    const float4 ga = *reinterpret_cast<const float4*>(gamma + c), be = *reinterpret_cast<const float4*>(beta + c);
    for (int r = r0 + ty; r < r1; r += nry) {
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if ((r - g.off) % g.st < g.L) {
            const float4 v = *reinterpret_cast<const float4*>(x + (size_t)r * C + c);
            o[0] = (v.x - m.x) * rs.x * ga.x + be.x; o[1] = (v.y - m.y) * rs.y * ga.y + be.y;
            o[2] = (v.z - m.z) * rs.z * ga.z + be.z; o[3] = (v.w - m.w) * rs.w * ga.w + be.w;
            const uint32_t rkey = drop_thresh ? rng_row_key(seed, stream, (uint32_t)r) : 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = fmaxf(o[e], 0.f);
                if (drop_thresh) a = rng_keep(rkey, c + e, drop_thresh) ? a * drop_scale : 0.f;
                o[e] = a;
            }
        }
        *reinterpret_cast<float4*>(y + (size_t)r * C + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// stage 3: only each prefix's last row is used -> P[b, s, :]
__global__ __launch_bounds__(256) void pfx_apply_last_kernel(const float* __restrict__ x, const int* __restrict__ segoff, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             float* __restrict__ P, int B, int T, int C, uint32_t drop_thresh, float drop_scale, uint32_t seed,
                                                             uint32_t stream) {
    const int cq = C >> 2;
    const size_t total = (size_t)B * T * cq;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % cq) * 4;
        const int bs = (int)(i / cq), b = bs / T, s = bs - b * T;
        const int L = s > 0 ? s : 1;
        const int r = segoff[s] + b * (L + 2) + L - 1;
        const float4 v = *reinterpret_cast<const float4*>(x + (size_t)r * C + c);
        const float4 m = *reinterpret_cast<const float4*>(mean + (size_t)s * C + c), rs = *reinterpret_cast<const float4*>(rstd + (size_t)s * C + c);
        const float4 ga = *reinterpret_cast<const float4*>(gamma + c), be = *reinterpret_cast<const float4*>(beta + c);
        float o[4] = {(v.x - m.x) * rs.x * ga.x + be.x, (v.y - m.y) * rs.y * ga.y + be.y, (v.z - m.z) * rs.z * ga.z + be.z, (v.w - m.w) * rs.w * ga.w + be.w};
        const uint32_t rkey = drop_thresh ? rng_row_key(seed, stream, (uint32_t)r) : 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a = fmaxf(o[e], 0.f);
            if (drop_thresh) a = rng_keep(rkey, c + e, drop_thresh) ? a * drop_scale : 0.f;
            o[e] = a;
        }
        *reinterpret_cast<float4*>(P + (size_t)bs * C + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------------
// g = dy gated by the recomputed ReLU and dropout factor.  last_only: dy is d_P [B,T,C], non-zero on each prefix's last row only.
struct PfxGate { float g[4], xh[4]; };
__device__ __forceinline__ PfxGate pfx_gate(const float* __restrict__ dy, const float* __restrict__ x, int r, int c, int C, const PfxSeg& g, int T, int last_only,
                                            const float4& m, const float4& rs, const float4& ga, const float4& be, uint32_t drop_thresh, float drop_scale,
                                            uint32_t seed, uint32_t stream) {
    PfxGate o;
    const float4 v = *reinterpret_cast<const float4*>(x + (size_t)r * C + c);
    const float mm[4] = {m.x, m.y, m.z, m.w}, ss[4] = {rs.x, rs.y, rs.z, rs.w}, gg[4] = {ga.x, ga.y, ga.z, ga.w}, bb[4] = {be.x, be.y, be.z, be.w};
    const float xv[4] = {v.x, v.y, v.z, v.w};
    const int rel = r - g.off, b = rel / g.st, j = rel - b * g.st;
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    if (!last_only || j == g.L - 1) {
        const float4 d4 = *reinterpret_cast<const float4*>(last_only ? dy + ((size_t)b * T + g.s) * C + c : dy + (size_t)r * C + c);
        d[0] = d4.x; d[1] = d4.y; d[2] = d4.z; d[3] = d4.w;
    }
    const uint32_t rkey = drop_thresh ? rng_row_key(seed, stream, (uint32_t)r) : 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float xh = (xv[e] - mm[e]) * ss[e];
        const float pre = xh * gg[e] + bb[e];
        float dd = d[e];
        if (drop_thresh) dd = rng_keep(rkey, c + e, drop_thresh) ? dd * drop_scale : 0.f;
        o.g[e] = pre > 0.f ? dd : 0.f;
        o.xh[e] = xh;
    }
    return o;
}

__global__ __launch_bounds__(256) void pfx_bwd_part_kernel(const float* __restrict__ dy, const float* __restrict__ x, const int* __restrict__ chunks,
                                                           const int* __restrict__ segoff, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, int T, int C, int last_only,
                                                           uint32_t drop_thresh, float drop_scale, uint32_t seed, uint32_t stream, double* __restrict__ part) {
    __shared__ double red[2][256][4];
    const int cq = C >> 2, nry = 256 / cq;
    const int tx = threadIdx.x % cq, ty = threadIdx.x / cq;
    const PfxSeg g = pfx_seg(segoff, chunks[2 * blockIdx.x]);
    const int r0 = chunks[2 * blockIdx.x + 1], r1 = min(r0 + PFX_CHUNK, g.end);
    const int c = tx * 4;
    double a[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
    if (ty < nry) {
        const float4 m = *reinterpret_cast<const float4*>(mean + (size_t)g.s * C + c), rs = *reinterpret_cast<const float4*>(rstd + (size_t)g.s * C + c);
        const float4 ga = *reinterpret_cast<const float4*>(gamma + c), be = *reinterpret_cast<const float4*>(beta + c);
        for (int r = r0 + ty; r < r1; r += nry) {
            const int j = (r - g.off) % g.st;
            if (j >= g.L || (last_only && j != g.L - 1)) continue;         // gap rows are not read; rows with a zero cotangent add nothing
            const PfxGate o = pfx_gate(dy, x, r, c, C, g, T, last_only, m, rs, ga, be, drop_thresh, drop_scale, seed, stream);
#pragma unroll
            for (int e = 0; e < 4; ++e) { a[e] += (double)o.g[e]; q[e] += (double)o.g[e] * (double)o.xh[e]; }
        }
    }
    pfx_block_reduce(red, a, q, C, cq, nry, part + (size_t)blockIdx.x * 2 * C);
}

// one workgroup per segment: S[s] = {sum g, sum g xhat} from the chunk partials in order
__global__ __launch_bounds__(256) void pfx_bwd_final_kernel(const double* __restrict__ part, const int* __restrict__ chunk_start, int C, double* __restrict__ S) {
    const int s = blockIdx.x;
    for (int c = threadIdx.x; c < 2 * C; c += 256) {
        double a = 0.0;
        for (int k = chunk_start[s]; k < chunk_start[s + 1]; ++k) a += part[(size_t)k * 2 * C + c];
        S[(size_t)s * 2 * C + c] = a;
    }
}

// dbeta += sum_s S1, dgamma += sum_s S2, segments in order
__global__ __launch_bounds__(256) void pfx_bwd_params_kernel(const double* __restrict__ S, int T, int C, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double a = 0.0, q = 0.0;
    for (int s = 0; s < T; ++s) { a += S[(size_t)s * 2 * C + c]; q += S[(size_t)s * 2 * C + C + c]; }
    dbeta[c] += (float)a;
    dgamma[c] += (float)q;
}

// dz = rstd gamma (g - mean(g) - xhat mean(g xhat)) on live rows, exact zeros on gap rows
__global__ __launch_bounds__(256) void pfx_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x, const int* __restrict__ chunks,
                                                            const int* __restrict__ segoff, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, const double* __restrict__ S,
                                                            float* __restrict__ dz, int B, int T, int C, int last_only, uint32_t drop_thresh, float drop_scale,
                                                            uint32_t seed, uint32_t stream) {
    const int cq = C >> 2, nry = 256 / cq;
    const int tx = threadIdx.x % cq, ty = threadIdx.x / cq;
    if (ty >= nry) return;
    const PfxSeg g = pfx_seg(segoff, chunks[2 * blockIdx.x]);
    const int r0 = chunks[2 * blockIdx.x + 1], r1 = min(r0 + PFX_CHUNK, g.end);
    const int c = tx * 4;
    const float4 m = *reinterpret_cast<const float4*>(mean + (size_t)g.s * C + c), rs = *reinterpret_cast<const float4*>(rstd + (size_t)g.s * C + c);
    const float4 ga = *reinterpret_cast<const float4*>(gamma + c), be = *reinterpret_cast<const float4*>(beta + c);
    const double n = (double)B * g.L;
    const double* Ss = S + (size_t)g.s * 2 * C;
    float s1[4], s2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { s1[e] = (float)(Ss[c + e] / n); s2[e] = (float)(Ss[C + c + e] / n); }
    const float k[4] = {ga.x * rs.x, ga.y * rs.y, ga.z * rs.z, ga.w * rs.w};
    for (int r = r0 + ty; r < r1; r += nry) {
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if ((r - g.off) % g.st < g.L) {
            const PfxGate t = pfx_gate(dy, x, r, c, C, g, T, last_only, m, rs, ga, be, drop_thresh, drop_scale, seed, stream);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = k[e] * (t.g[e] - s1[e] - t.xh[e] * s2[e]);
        }
        *reinterpret_cast<float4*>(dz + (size_t)r * C + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ---- the embedded slab ---------------------------------------------------------------------------------------------------------------------
// out[row(s,b,j)] = dropout(E[id]) with id = SOS at s = 0, target[b, j] else; zeros on gap rows (and for an id outside the table)
__global__ __launch_bounds__(256) void pfx_embed_fwd_kernel(const int64_t* __restrict__ target, const float* __restrict__ E, const int* __restrict__ chunks,
                                                            const int* __restrict__ segoff, float* __restrict__ out, int T, int D, int vocab, int sos,
                                                            uint32_t drop_thresh, float drop_scale, uint32_t seed, uint32_t stream) {
    const int dq = D >> 2;
    const PfxSeg g = pfx_seg(segoff, chunks[2 * blockIdx.x]);
    const int r0 = chunks[2 * blockIdx.x + 1], r1 = min(r0 + PFX_CHUNK, g.end);
    const int total = (r1 - r0) * dq;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int r = r0 + i / dq, c = (i % dq) * 4;
        const int rel = r - g.off, b = rel / g.st, j = rel - b * g.st;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if (j < g.L) {
            const int64_t id = g.s == 0 ? (int64_t)sos : target[(size_t)b * T + j];
            if (id >= 0 && id < vocab) {
                const float4 v = *reinterpret_cast<const float4*>(E + (size_t)id * D + c);
                o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
                if (drop_thresh) {
                    const uint32_t rkey = rng_row_key(seed, stream, (uint32_t)r);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = rng_keep(rkey, c + e, drop_thresh) ? o[e] * drop_scale : 0.f;
                }
            }
        }
        *reinterpret_cast<float4*>(out + (size_t)r * D + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// The slab gradient summed over the prefixes that hold a token, segments in order: G[b, 0] = the SOS row of segment 0, G[b, 1 + t] =
// sum_{s > t} mask . dx[row(s, b, t)].  unast_embed_bwd over ids [SOS | target] then scatters G into dE.
__global__ __launch_bounds__(256) void pfx_embed_bwd_kernel(const float* __restrict__ dx, const int* __restrict__ segoff, float* __restrict__ G, int B, int T, int D,
                                                            uint32_t drop_thresh, float drop_scale, uint32_t seed, uint32_t stream) {
    const int dq = D >> 2;
    const size_t total = (size_t)B * (T + 1) * dq;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % dq) * 4;
        const int bk = (int)(i / dq), b = bk / (T + 1), k = bk - b * (T + 1);
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        const int t = k ? k - 1 : 0;
        const int sa = k ? k : 0, sb = k ? T : 1;                           // segments [sa, sb) hold this token at row j = t
        for (int s = sa; s < sb; ++s) {
            const int L = s > 0 ? s : 1;
            const int r = segoff[s] + b * (L + 2) + t;
            const float4 v = *reinterpret_cast<const float4*>(dx + (size_t)r * D + c);
            float d[4] = {v.x, v.y, v.z, v.w};
            if (drop_thresh) {
                const uint32_t rkey = rng_row_key(seed, stream, (uint32_t)r);
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = rng_keep(rkey, c + e, drop_thresh) ? d[e] * drop_scale : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] += d[e];
        }
        *reinterpret_cast<float4*>(G + (size_t)bk * D + c) = make_float4(a[0], a[1], a[2], a[3]);
    }
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------
static int pfx_grid(size_t work) {
    size_t b = (work + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}
#define PFX_GEOMETRY(name)                                                                                                                        \
    UNAST_REQUIRE(B >= 2 && T >= 1 && T <= 512 && nchunks >= T && slab_rows > 0, name ": need 2 <= B, 1 <= T <= 512, one chunk per segment at least");   \
    UNAST_REQUIRE(C > 0 && (C & 3) == 0 && C <= 1024 && 256 % (C >> 2) == 0, name ": need C %% 4 == 0, C/4 a divisor of 256 (C=%d)", C);                   \
    UNAST_REQUIRE((long long)slab_rows * C * 4 < 0x7FFFFFF0LL, name ": slab of %d rows x %d columns exceeds 2 GiB", slab_rows, C)

extern "C" int unast_prefix_bn_fwd(const float* x, const int* chunks, const int* chunk_start, const int* segoff, int nchunks, int slab_rows, int B, int T, int C,
                                   const float* gamma, const float* beta, float* y, float* p_last, float* mean, float* rstd, float* varu,
                                   float* running_mean, float* running_var, int64_t* num_batches_tracked, double* ws /* nchunks*2*C */, float eps,
                                   float momentum, float drop_p, unsigned int seed, unsigned int stream_id, hipStream_t stream) {
    UNAST_REQUIRE(x && chunks && chunk_start && segoff && gamma && beta && mean && rstd && varu && ws, "unast_prefix_bn_fwd: null pointer");
    UNAST_REQUIRE((y != nullptr) != (p_last != nullptr), "unast_prefix_bn_fwd: give y (the slab) or p_last ([B,T,C], stage 3), not both");
    UNAST_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "unast_prefix_bn_fwd: running_mean and running_var together");
    PFX_GEOMETRY("unast_prefix_bn_fwd");
    const float dsc = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
    hipLaunchKernelGGL(pfx_stats_part_kernel, dim3(nchunks), dim3(256), 0, stream, x, chunks, segoff, C, ws);
    hipLaunchKernelGGL(pfx_stats_final_kernel, dim3(T), dim3(256), 0, stream, ws, chunk_start, B, C, eps, mean, rstd, varu);
    if (running_mean)
        hipLaunchKernelGGL(pfx_running_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, mean, varu, T, C, momentum, running_mean, running_var,
                           (long long*)num_batches_tracked);
    if (y) hipLaunchKernelGGL(pfx_apply_kernel, dim3(nchunks), dim3(256), 0, stream, x, chunks, segoff, mean, rstd, gamma, beta, y, C, drop_threshold(drop_p), dsc, seed, stream_id);
    else hipLaunchKernelGGL(pfx_apply_last_kernel, dim3(pfx_grid((size_t)B * T * (C / 4))), dim3(256), 0, stream, x, segoff, mean, rstd, gamma, beta, p_last, B, T, C,
                            drop_threshold(drop_p), dsc, seed, stream_id);
    return unast_check_launch("unast_prefix_bn_fwd");
}

extern "C" int unast_prefix_bn_bwd(const float* dy, int last_only, const float* x, const int* chunks, const int* chunk_start, const int* segoff, int nchunks,
                                   int slab_rows, int B, int T, int C, const float* mean, const float* rstd, const float* gamma, const float* beta, float* dz,
                                   float* dgamma, float* dbeta, double* ws /* (nchunks + T)*2*C */, float drop_p, unsigned int seed, unsigned int stream_id,
                                   hipStream_t stream) {
    UNAST_REQUIRE(dy && x && chunks && chunk_start && segoff && mean && rstd && gamma && beta && dz && ws, "unast_prefix_bn_bwd: null pointer");
    UNAST_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), "unast_prefix_bn_bwd: dgamma/dbeta must both be given or both null");
    PFX_GEOMETRY("unast_prefix_bn_bwd");
    const float dsc = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
    const uint32_t th = drop_threshold(drop_p);
    double* S = ws + (size_t)nchunks * 2 * C;
    hipLaunchKernelGGL(pfx_bwd_part_kernel, dim3(nchunks), dim3(256), 0, stream, dy, x, chunks, segoff, mean, rstd, gamma, beta, T, C, last_only ? 1 : 0, th, dsc, seed,
                       stream_id, ws);
    hipLaunchKernelGGL(pfx_bwd_final_kernel, dim3(T), dim3(256), 0, stream, ws, chunk_start, C, S);
    if (dgamma) hipLaunchKernelGGL(pfx_bwd_params_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, S, T, C, dgamma, dbeta);
    hipLaunchKernelGGL(pfx_bwd_apply_kernel, dim3(nchunks), dim3(256), 0, stream, dy, x, chunks, segoff, mean, rstd, gamma, beta, S, dz, B, T, C, last_only ? 1 : 0, th,
                       dsc, seed, stream_id);
    return unast_check_launch("unast_prefix_bn_bwd");
}

extern "C" int unast_prefix_embed_fwd(const int64_t* target, const float* E, const int* chunks, const int* segoff, int nchunks, int slab_rows, int B, int T, int C,
                                      int vocab, int sos, float* out, float drop_p, unsigned int seed, unsigned int stream_id, hipStream_t stream) {
    UNAST_REQUIRE(target && E && chunks && segoff && out && vocab > 0 && sos >= 0 && sos < vocab, "unast_prefix_embed_fwd: bad arguments");
    PFX_GEOMETRY("unast_prefix_embed_fwd");
    hipLaunchKernelGGL(pfx_embed_fwd_kernel, dim3(nchunks), dim3(256), 0, stream, target, E, chunks, segoff, out, T, C, vocab, sos, drop_threshold(drop_p),
                       drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f, seed, stream_id);
    return unast_check_launch("unast_prefix_embed_fwd");
}

extern "C" int unast_prefix_embed_bwd(const float* dx, const int* segoff, int slab_rows, int B, int T, int C, float* G, float drop_p, unsigned int seed,
                                      unsigned int stream_id, hipStream_t stream) {
    UNAST_REQUIRE(dx && segoff && G, "unast_prefix_embed_bwd: null pointer");
    const int nchunks = T;
    PFX_GEOMETRY("unast_prefix_embed_bwd");
    hipLaunchKernelGGL(pfx_embed_bwd_kernel, dim3(pfx_grid((size_t)B * (T + 1) * (C / 4))), dim3(256), 0, stream, dx, segoff, G, B, T, C, drop_threshold(drop_p),
                       drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f, seed, stream_id);
    return unast_check_launch("unast_prefix_embed_bwd");
}

UNAST_DEFINE_RNG_EPOCH_SETTER(prefix)
