// Kernels of the RNN model family (TextRNN / SpeechRNN, src/network.py:279-402, 503-624; src/module.py:297-497) at the width every
// full-size reference config uses, hidden 256: the eval path and the encoders' training (unast_amd/train_rnn.py).
//   lstm_seq_fwd_kernel   recurrence of one packed nn.LSTM layer (src/module.py:306, 315-317); <true> also saves what the backward reads
//   lstm_seq_bwd_kernel   backpropagation through time of that recurrence
//   rnn_attn_step_kernel  one step of Luong / location-sensitive additive attention (src/module.py:395-497)
//   lstm_cell_kernel      pointwise cell update of one decoder step (the nn.LSTM call of src/module.py:371 at sequence length 1)
#include "common.h"

namespace {

constexpr int RH = 256;              // hidden units
constexpr int RG = 4 * RH;           // gate rows of W_hh (i, f, g, o)
constexpr int SEQ_TILE = 16;         // sequences per workgroup = M of the MFMA tile
constexpr int LDH = RH + 4;          // LDS row of one sequence's h (floats; padded by one 16-byte slot)
constexpr int SEQ_THREADS = 512;     // 8 waves, each owning 32 hidden units of all four gates

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// h_t = LSTM(x_t, h_{t-1}) for a tile of 16 sequences of one direction.  Per step the tile's gates are the [16,256] x [256,1024] product
// h . W_hh^T on the f32-input MFMA (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation), started from xproj + b_ih + b_hh.
// h lives in LDS (double buffered, one barrier per step), c and the lane's own h in registers.  A wave owns hidden units
// [32 w, 32 w + 32) of all four gates, so the accumulator lane that holds gate i of (sequence, unit) also holds f, g and o of it and the
// cell update needs no exchange.  W_hh is streamed from L2 every step in fragment order (wfrag, see unast_lstm_seq_fwd): one float4 per
// lane is the B operand of four consecutive k-steps, a wave's load is 1 KiB contiguous.
// MFMA k order: k-step s of group g takes k = 16 g + 4 (lane >> 4) + s from both operands (any permutation of k is a valid contraction
// as long as A and B agree), which makes the A operand a float4 of the row-major h row.
//
// TRAIN (unast_lstm_seq_fwd_train): the same instructions in the same order on y, hfinal and cfinal, plus what unast_lstm_seq_bwd reads:
//   saved [B,T,ndir,5,256]   the activations i, f, g, o and the cell state c_t of every live (b, t, dir, unit); rows t >= lens[b] are neither
//                            written here nor read by the backward
//   hprev [B,T,ndir*256]     h_{t-1} in the direction's own order (zero at a sequence's first step in its direction); rows t >= lens[b] are
//                            written as zeros, since dW_hh = dxproj^T hprev is a GEMM over all B T rows
template <bool TRAIN>
__global__ __launch_bounds__(SEQ_THREADS) void lstm_seq_fwd_kernel(const float* __restrict__ xproj, const float* __restrict__ wfrag,
                                                                   const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                                   const int* __restrict__ lens, float* __restrict__ y, float* __restrict__ hfinal,
                                                                   float* __restrict__ cfinal, float* __restrict__ saved, float* __restrict__ hprev,
                                                                   int B, int T, int ndir) {
    __shared__ __attribute__((aligned(16))) float hs[2][SEQ_TILE][LDH];
    __shared__ int s_len[SEQ_TILE];
    const int dir = blockIdx.y, b0 = blockIdx.x * SEQ_TILE;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, j = lane & 15;

    for (int i = tid; i < 2 * SEQ_TILE * LDH; i += SEQ_THREADS) (&hs[0][0][0])[i] = 0.f;
    if (tid < SEQ_TILE) {
        int n = 0;
        if (b0 + tid < B) n = min(max(lens[b0 + tid], 0), T);
        s_len[tid] = n;
    }
    __syncthreads();
    int tmax = 0;
#pragma unroll
    for (int i = 0; i < SEQ_TILE; ++i) tmax = max(tmax, s_len[i]);
    int len_r[4];
    bool live_r[4];                                   // the row is a sequence of the batch (not tile padding)
#pragma unroll
    for (int r = 0; r < 4; ++r) { len_r[r] = s_len[4 * q + r]; live_r[r] = b0 + 4 * q + r < B; }

    const float4* wf = reinterpret_cast<const float4*>(wfrag) + (size_t)dir * (RG * RH / 4);
    const int unit0 = wave * 32 + j;                  // + 16 u
    float bsum[4][2];
#pragma unroll
    for (int G = 0; G < 4; ++G)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int n = dir * RG + G * RH + unit0 + 16 * u;
            bsum[G][u] = b_ih[n] + b_hh[n];
        }

    const size_t xrow = (size_t)ndir * RG, yrow = (size_t)ndir * RH;
    auto load_x = [&](int s, float (&x)[4][2][4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool on = s < len_r[r];
            const int t = dir ? len_r[r] - 1 - s : s;
            const float* p = xproj + ((size_t)(b0 + 4 * q + r) * T + (on ? t : 0)) * xrow + (size_t)dir * RG + unit0;
#pragma unroll
            for (int G = 0; G < 4; ++G)
#pragma unroll
                for (int u = 0; u < 2; ++u) x[G][u][r] = on ? p[G * RH + 16 * u] : 0.f;
        }
    };

    float c[2][4], h[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) { c[u][r] = 0.f; h[u][r] = 0.f; }
    float xc[4][2][4], xn[4][2][4];
    load_x(0, xc);

    for (int s = 0; s < T; ++s) {
        if (s >= tmax) {                              // past every sequence of the tile: only the zero padding of y is left
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (live_r[r]) {
                    float* yp = y + ((size_t)(b0 + 4 * q + r) * T + s) * yrow + (size_t)dir * RH + unit0;
                    yp[0] = 0.f; yp[16] = 0.f;
                    if constexpr (TRAIN) {
                        float* hp = hprev + ((size_t)(b0 + 4 * q + r) * T + s) * yrow + (size_t)dir * RH + unit0;
                        hp[0] = 0.f; hp[16] = 0.f;
                    }
                }
            continue;
        }
        const int cur = s & 1;
        f32x4 acc[4][2];
#pragma unroll
        for (int G = 0; G < 4; ++G)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[G][u][r] = xc[G][u][r] + bsum[G][u];
        load_x(s + 1, xn);                            // (s + 1 >= len: zeros, no load)

#pragma unroll 2
        for (int g = 0; g < 16; ++g) {
            const float4 a = *reinterpret_cast<const float4*>(&hs[cur][j][g * 16 + q * 4]);
            float4 w[4][2];
#pragma unroll
            for (int G = 0; G < 4; ++G)
#pragma unroll
                for (int u = 0; u < 2; ++u) w[G][u] = wf[((size_t)((G * 16 + wave * 2 + u) * 16 + g)) * 64 + lane];
#pragma unroll
            for (int G = 0; G < 4; ++G)
#pragma unroll
                for (int u = 0; u < 2; ++u) acc[G][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w[G][u].x, acc[G][u], 0, 0, 0);
#pragma unroll
            for (int G = 0; G < 4; ++G)
#pragma unroll
                for (int u = 0; u < 2; ++u) acc[G][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w[G][u].y, acc[G][u], 0, 0, 0);
#pragma unroll
            for (int G = 0; G < 4; ++G)
#pragma unroll
                for (int u = 0; u < 2; ++u) acc[G][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w[G][u].z, acc[G][u], 0, 0, 0);
#pragma unroll
            for (int G = 0; G < 4; ++G)
#pragma unroll
                for (int u = 0; u < 2; ++u) acc[G][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w[G][u].w, acc[G][u], 0, 0, 0);
        }

#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool on = s < len_r[r];
            const int t = on ? (dir ? len_r[r] - 1 - s : s) : s;       // a finished sequence's row s is padding
            float* yp = y + ((size_t)(b0 + 4 * q + r) * T + t) * yrow + (size_t)dir * RH + unit0;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if constexpr (TRAIN) {
                    if (live_r[r]) hprev[((size_t)(b0 + 4 * q + r) * T + t) * yrow + (size_t)dir * RH + unit0 + 16 * u] = on ? h[u][r] : 0.f;
                }
                if (on) {
                    const float ig = sigmoidf_(acc[0][u][r]), fg = sigmoidf_(acc[1][u][r]), gg = tanhf(acc[2][u][r]), og = sigmoidf_(acc[3][u][r]);
                    c[u][r] = fg * c[u][r] + ig * gg;
                    h[u][r] = og * tanhf(c[u][r]);
                    if constexpr (TRAIN) {
                        float* sp = saved + (((size_t)(b0 + 4 * q + r) * T + t) * ndir + dir) * (5 * RH) + unit0 + 16 * u;
                        sp[0] = ig; sp[RH] = fg; sp[2 * RH] = gg; sp[3 * RH] = og; sp[4 * RH] = c[u][r];
                    }
                }
                if (live_r[r]) yp[16 * u] = on ? h[u][r] : 0.f;
                hs[cur ^ 1][4 * q + r][unit0 + 16 * u] = h[u][r];
            }
        }
#pragma unroll
        for (int G = 0; G < 4; ++G)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) xc[G][u][r] = xn[G][u][r];
        __syncthreads();
    }

#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (live_r[r]) {
            const size_t o = (size_t)(b0 + 4 * q + r) * yrow + (size_t)dir * RH + unit0;
#pragma unroll
            for (int u = 0; u < 2; ++u) { hfinal[o + 16 * u] = h[u][r]; cfinal[o + 16 * u] = c[u][r]; }
        }
}

// Backward of lstm_seq_fwd_kernel<true> through time for a tile of 16 sequences of one direction, in the reverse of the forward's step order.
// Per step: dh = dy[b,t] + dh_rec (+ dhfinal / dcfinal at the sequence's own last forward step, s = len - 1: t = len - 1 forward, t = 0
// reverse), the pointwise gate gradients from `saved` (layout: lstm_seq_fwd_kernel), dG_t [16,1024] to global memory as dxproj [B,T,ndir*1024]
// (the gradient of the forward's xproj input) and to LDS, then dh_rec [16,256] = dG_t [16,1024] x W_hh [1024,256] on v_mfma_f32_16x16x4_f32.
// A wave owns hidden units [32 w, 32 w + 32): two 16x16 output tiles, each summed over its 256 k-steps in two interleaved chains (four
// independent accumulators per wave), 512 MFMAs per wave and step as in the forward.  The accumulator lane layout is the forward's gate
// layout, so dh_rec, dc and the pointwise step stay in the lane's registers; only dG_t goes through LDS (two buffers of 16 rows of 1024 + 4
// floats, 128.5 KiB, one barrier per step: a wave writes buffer s & 1 two barriers after the last read of it).
// W_hh is streamed from L2 every step in a second fragment order (wfrag_t, ops.lstm_whh_fragments_bwd), the B operand [k = gate row][n = unit]:
//   wfrag_t[d][n][g][16 q + j][s] = W_hh[d][16 g + 4 q + s][16 n + j]      n: 16 unit tiles, g: 64 k groups
// so that the A operand of the group's four k-steps is a float4 of the LDS row.
// A row that is not live at step s (s >= len, or tile padding) writes a zero dG row: its dh_rec stays zero until its own last step.  dy and
// saved at t >= lens[b] are never read; dxproj at t >= lens[b] is written as exact zeros; steps past the tile's longest sequence skip the product.
constexpr int LDG = RG + 4;          // LDS row of one sequence's dG (floats; padded by one 16-byte slot)

__global__ __launch_bounds__(SEQ_THREADS) void lstm_seq_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ dhfinal,
                                                                   const float* __restrict__ dcfinal, const float* __restrict__ wfrag_t,
                                                                   const float* __restrict__ saved, const int* __restrict__ lens,
                                                                   float* __restrict__ dxproj, int B, int T, int ndir) {
    __shared__ __attribute__((aligned(16))) float gs[2][SEQ_TILE][LDG];
    __shared__ int s_len[SEQ_TILE];
    const int dir = blockIdx.y, b0 = blockIdx.x * SEQ_TILE;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, j = lane & 15;

    if (tid < SEQ_TILE) {
        int n = 0;
        if (b0 + tid < B) n = min(max(lens[b0 + tid], 0), T);
        s_len[tid] = n;
    }
    __syncthreads();
    int tmax = 0;
#pragma unroll
    for (int i = 0; i < SEQ_TILE; ++i) tmax = max(tmax, s_len[i]);
    int len_r[4];
    bool live_r[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { len_r[r] = s_len[4 * q + r]; live_r[r] = b0 + 4 * q + r < B; }

    const float4* wf = reinterpret_cast<const float4*>(wfrag_t) + (size_t)dir * (RG * RH / 4);
    const int unit0 = wave * 32 + j;                  // + 16 u
    const size_t xrow = (size_t)ndir * RG, yrow = (size_t)ndir * RH;

    // padding rows of dxproj past the tile's longest sequence
    for (int s = tmax; s < T; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (live_r[r]) {
                float* dp = dxproj + ((size_t)(b0 + 4 * q + r) * T + s) * xrow + (size_t)dir * RG + unit0;
#pragma unroll
                for (int G = 0; G < 4; ++G) { dp[G * RH] = 0.f; dp[G * RH + 16] = 0.f; }
            }

    // what step s reads: v[0..3] = i, f, g, o, v[4] = c_t, v[5] = c_{t-1} (the cell state of step s - 1; zero at s = 0), v[6] = dy
    auto load_step = [&](int s, float (&v)[7][2][4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool on = s >= 0 && s < len_r[r];
            const int t = dir ? len_r[r] - 1 - s : s;
            const int tp = dir ? t + 1 : t - 1;
            const size_t row = (size_t)(b0 + 4 * q + r) * T;
            const float* sp = saved + ((row + (on ? t : 0)) * ndir + dir) * (5 * RH) + unit0;
            const float* cp = saved + ((row + (on && s > 0 ? tp : 0)) * ndir + dir) * (5 * RH) + 4 * RH + unit0;
            const float* yp = dy + (row + (on ? t : 0)) * yrow + (size_t)dir * RH + unit0;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
#pragma unroll
                for (int k = 0; k < 5; ++k) v[k][u][r] = on ? sp[k * RH + 16 * u] : 0.f;
                v[5][u][r] = on && s > 0 ? cp[16 * u] : 0.f;
                v[6][u][r] = on ? yp[16 * u] : 0.f;
            }
        }
    };

    float dhr[2][4], dc[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) { dhr[u][r] = 0.f; dc[u][r] = 0.f; }
    float vc[7][2][4], vn[7][2][4];
    load_step(tmax - 1, vc);

    for (int s = tmax - 1; s >= 0; --s) {
        const int cur = s & 1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool on = s < len_r[r];
            const bool last = s == len_r[r] - 1;
            const int t = on ? (dir ? len_r[r] - 1 - s : s) : s;       // a finished sequence's row s is padding
            const size_t fo = (size_t)(b0 + 4 * q + r) * yrow + (size_t)dir * RH + unit0;
            float* dp = dxproj + ((size_t)(b0 + 4 * q + r) * T + t) * xrow + (size_t)dir * RG + unit0;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                float gi = 0.f, gf = 0.f, gg = 0.f, go = 0.f;
                if (on) {
                    float dh = vc[6][u][r] + dhr[u][r];
                    if (last) {
                        if (dhfinal) dh += dhfinal[fo + 16 * u];
                        if (dcfinal) dc[u][r] += dcfinal[fo + 16 * u];
                    }
                    const float ia = vc[0][u][r], fa = vc[1][u][r], ga = vc[2][u][r], oa = vc[3][u][r];
                    const float tc = tanhf(vc[4][u][r]);
                    const float dct = dc[u][r] + dh * oa * (1.f - tc * tc);
                    go = dh * tc * oa * (1.f - oa);
                    gi = dct * ga * ia * (1.f - ia);
                    gg = dct * ia * (1.f - ga * ga);
                    gf = dct * vc[5][u][r] * fa * (1.f - fa);
                    dc[u][r] = dct * fa;
                }
                if (live_r[r]) { dp[16 * u] = gi; dp[RH + 16 * u] = gf; dp[2 * RH + 16 * u] = gg; dp[3 * RH + 16 * u] = go; }
                float* lp = &gs[cur][4 * q + r][unit0 + 16 * u];
                lp[0] = gi; lp[RH] = gf; lp[2 * RH] = gg; lp[3 * RH] = go;
            }
        }
        if (s == 0) break;                            // nothing reads the first step's dh_rec
        load_step(s - 1, vn);
        __syncthreads();

        f32x4 acc[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[u][h][r] = 0.f;
#pragma unroll 4
        for (int g = 0; g < 64; ++g) {
            const float4 a = *reinterpret_cast<const float4*>(&gs[cur][j][g * 16 + q * 4]);
            float4 w[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) w[u] = wf[((size_t)((wave * 2 + u) * 64 + g)) * 64 + lane];
#pragma unroll
            for (int u = 0; u < 2; ++u) acc[u][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w[u].x, acc[u][0], 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 2; ++u) acc[u][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w[u].y, acc[u][1], 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 2; ++u) acc[u][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w[u].z, acc[u][0], 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 2; ++u) acc[u][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w[u].w, acc[u][1], 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) dhr[u][r] = acc[u][0][r] + acc[u][1][r];
#pragma unroll
        for (int k = 0; k < 7; ++k)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) vc[k][u][r] = vn[k][u][r];
    }
}

// ---- additive attention, one decoder step -----------------------------------------------------------------------------------------
constexpr int ATT_THREADS = 256;
constexpr int ATT_MAX_A = 64;        // attention width
constexpr int LOC_F = 32, LOC_K = 31, LOC_PAD = 15;    // LocationLayer: Conv1d(2 -> 32, k = 31, pad 15), src/module.py:396-397
constexpr int ENC_D = 512;           // encoder output width (2 x hidden)

__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup per sequence.  LDS (dynamic, floats): qp[64] | vs[64] | red[4 + 12 pad] | sc[Tk4] and, in LSA mode, behind them
// pc[2][Tk4 + 32] (prev and cum with a zero halo of 15 on the left and at least 15 on the right) | conv[32*2*31] | dense[A*32].
__global__ __launch_bounds__(ATT_THREADS) void rnn_attn_step_kernel(int mode, const float* __restrict__ hq, int ldq, const float* __restrict__ Wq,
                                                                    const float* __restrict__ mem, const float* __restrict__ vw,
                                                                    const float* __restrict__ enc, const int* __restrict__ lens, float* __restrict__ prev,
                                                                    float* __restrict__ cum, const float* __restrict__ conv_w,
                                                                    const float* __restrict__ dense_w, float* __restrict__ ctx, int ldc, int Tk, int A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Tk4 = (Tk + 3) & ~3;
    float* qp = smem;
    float* vs = qp + ATT_MAX_A;
    float* red = vs + ATT_MAX_A;
    float* sc = red + 16;
    float* pc = sc + Tk4;
    const int ldp = Tk4 + 32;
    float* convs = pc + 2 * ldp;
    float* denses = convs + LOC_F * 2 * LOC_K;
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int len = min(max(lens[b], 0), Tk);

    // query-side projection: qp[a] = Wq[a,:] . h[b,:]  (query_layer / project_hid, no bias)
    {
        const float4 hv = *reinterpret_cast<const float4*>(hq + (size_t)b * ldq + lane * 4);
        for (int a = wave; a < A; a += ATT_THREADS / 64) {
            const float4 wv = *reinterpret_cast<const float4*>(Wq + (size_t)a * RH + lane * 4);
            const float s = wave_sum((wv.x * hv.x + wv.y * hv.y) + (wv.z * hv.z + wv.w * hv.w));
            if (lane == 0) qp[a] = s;
        }
    }
    if (tid < A) vs[tid] = vw[tid];
    if (mode == 1) {
        for (int i = tid; i < 2 * ldp; i += ATT_THREADS) {
            const int ch = i / ldp, t = i - ch * ldp - LOC_PAD;
            pc[i] = (t >= 0 && t < Tk) ? (ch ? cum : prev)[(size_t)b * Tk + t] : 0.f;
        }
        for (int i = tid; i < LOC_F * 2 * LOC_K; i += ATT_THREADS) convs[i] = conv_w[i];
        for (int i = tid; i < A * LOC_F; i += ATT_THREADS) denses[i] = dense_w[i];
    }
    __syncthreads();

    // energies of the live keys
    float mx = -INFINITY;
    for (int t = tid; t < len; t += ATT_THREADS) {
        float f[LOC_F];
        if (mode == 1) {
#pragma unroll
            for (int i = 0; i < LOC_F; ++i) f[i] = 0.f;
            for (int ch = 0; ch < 2; ++ch)
                for (int k = 0; k < LOC_K; ++k) {
                    const float x = pc[ch * ldp + t + k];           // = in[ch][t + k - 15]
#pragma unroll
                    for (int i = 0; i < LOC_F; ++i) f[i] = fmaf(convs[(i * 2 + ch) * LOC_K + k], x, f[i]);
                }
        }
        const float* mrow = mem + ((size_t)b * Tk + t) * A;
        float e = 0.f;
        for (int a = 0; a < A; ++a) {
            float x = qp[a];
            if (mode == 1) {
                float loc = 0.f;
#pragma unroll
                for (int i = 0; i < LOC_F; ++i) loc = fmaf(denses[a * LOC_F + i], f[i], loc);
                x += loc;
            }
            x += mrow[a];
            e = fmaf(vs[a], tanhf(x), e);
        }
        sc[t] = e;
        mx = fmaxf(mx, e);
    }
    mx = block_max(mx, red);
    float sum = 0.f;
    for (int t = tid; t < len; t += ATT_THREADS) {
        const float p = expf(sc[t] - mx);
        sc[t] = p;
        sum += p;
    }
    sum = block_sum(sum, red);
    const float inv = len > 0 ? 1.f / sum : 0.f;
    for (int t = tid; t < Tk; t += ATT_THREADS) {
        const float w = t < len ? sc[t] * inv : 0.f;                // masked keys: exactly zero
        if (t < len) sc[t] = w;
        if (prev) prev[(size_t)b * Tk + t] = w;
        if (mode == 1) cum[(size_t)b * Tk + t] = pc[ldp + LOC_PAD + t] + w;
    }
    __syncthreads();

    // context = weights . enc  (two columns per thread)
    const float* ep = enc + (size_t)b * Tk * ENC_D + 2 * tid;
    float c0 = 0.f, c1 = 0.f, d0 = 0.f, d1 = 0.f;
    int t = 0;
    for (; t + 1 < len; t += 2) {
        const float2 e0 = *reinterpret_cast<const float2*>(ep + (size_t)t * ENC_D);
        const float2 e1 = *reinterpret_cast<const float2*>(ep + (size_t)(t + 1) * ENC_D);
        const float w0 = sc[t], w1 = sc[t + 1];
        c0 = fmaf(w0, e0.x, c0); c1 = fmaf(w0, e0.y, c1);
        d0 = fmaf(w1, e1.x, d0); d1 = fmaf(w1, e1.y, d1);
    }
    if (t < len) {
        const float2 e0 = *reinterpret_cast<const float2*>(ep + (size_t)t * ENC_D);
        c0 = fmaf(sc[t], e0.x, c0); c1 = fmaf(sc[t], e0.y, c1);
    }
    float* cp = ctx + (size_t)b * ldc + 2 * tid;
    cp[0] = c0 + d0;
    cp[1] = c1 + d1;
}

// One decoder step's cell update: gates [B, 4*256] are the pre-activations (both products and both biases already summed).
__global__ void lstm_cell_kernel(const float* __restrict__ gates, int ldg, float* __restrict__ c, int ldcs, float* __restrict__ h, int ldh, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * RH) return;
    const int b = i / RH, u = i - b * RH;
    const float* g = gates + (size_t)b * ldg + u;
    const float ig = sigmoidf_(g[0]), fg = sigmoidf_(g[RH]), gg = tanhf(g[2 * RH]), og = sigmoidf_(g[3 * RH]);
    const float cn = fg * c[(size_t)b * ldcs + u] + ig * gg;
    c[(size_t)b * ldcs + u] = cn;
    h[(size_t)b * ldh + u] = og * tanhf(cn);
}

__global__ void tanh_rows_kernel(float* __restrict__ x, int ldx, int rows, int cols) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    const int r = i / cols, cidx = i - r * cols;
    x[(size_t)r * ldx + cidx] = tanhf(x[(size_t)r * ldx + cidx]);
}

// ---- TextRNN.decode's prenet window (src/network.py:573: TextPrenet over the whole prefix, last position taken) ---------------------------
// The last position p of a prefix depends on its last 7 tokens only (three 5-tap convs), so a step recomputes a window of W positions
// p - W + 1 .. p.  Prefix conventions (src/network.py:546-557, 590-600): generation feeds tokens[b, 0 .. pos] (tokens[b,0] = SOS), so p = pos;
// teacher forcing feeds [SOS] at step 0 and target[b, 0 .. pos-1] afterwards, so p = max(pos, 1) - 1.
__device__ __forceinline__ int64_t window_last(int64_t pos, int tf) { return tf ? (pos > 1 ? pos : 1) - 1 : pos; }

// out[b, w, :] = emb[token at prefix position p - (W-1-w)], zero rows for positions before the prefix.
__global__ void text_window_kernel(const int64_t* __restrict__ tokens, int ld_tok, const float* __restrict__ emb, int E, float* __restrict__ out,
                                   int B, int W, const int64_t* __restrict__ pos, int tf, int sos) {
    const int64_t pv = pos[0], p = window_last(pv, tf);
    const int E4 = E >> 2;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * W * E4; i += gridDim.x * blockDim.x) {
        const int c = i % E4, w = (i / E4) % W, b = i / (E4 * W);
        const int64_t k = p - (W - 1 - w);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k >= 0) {
            const int64_t tok = (tf && pv == 0) ? sos : tokens[(size_t)b * ld_tok + k];
            v = reinterpret_cast<const float4*>(emb + (size_t)tok * E)[c];
        }
        reinterpret_cast<float4*>(out)[i] = v;
    }
}
// Rows of x [B, W, C] that stand for positions before the prefix are the NEXT conv's zero padding (not the conv of zeros): cleared here.
__global__ void window_mask_kernel(float* __restrict__ x, int B, int W, int C, const int64_t* __restrict__ pos, int tf) {
    const int64_t p = window_last(pos[0], tf);
    const int C4 = C >> 2;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * W * C4; i += gridDim.x * blockDim.x) {
        const int w = (i / C4) % W;
        if (p - (W - 1 - w) < 0) reinterpret_cast<float4*>(x)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
__global__ void pos_advance_kernel(int64_t* pos, int* epoch) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { pos[0] += 1; if (epoch) epoch[0] += 1; }
}

// ---- the few-row contractions of one decoder step with plain fp32 products ------------------------------------------------------------
// Y[m, n] = act(X[m, :] . W[n, :] + bias[n] + R[m, n]) for the M = B rows of a position, K <= 1024.  Products and sums are fp32 FMAs on the
// vector ALUs: unast_decode_linear forms its products from three-term split-bf16 operands (2^-17 relative), and a greedy trajectory chains
// ~10 contractions per position through weights that amplify rounding.  A wave owns four output columns and keeps their weight rows in
// registers (K / 64 floats per column and lane); X rows are read once per wave, a wave reduction per (row, column).
constexpr int RL_COLS = 4, RL_CHUNKS = 4;             // columns per wave; 256-float K chunks (K <= 1024)
__global__ __launch_bounds__(256) void rnn_linear_kernel(const float* __restrict__ X, int ldx, int64_t x_pos_stride, const float* __restrict__ W, int ldw,
                                                         const float* __restrict__ bias, const float* __restrict__ R, int ldr, float* __restrict__ Y, int ldy,
                                                         int64_t y_pos_stride, const int64_t* __restrict__ pos, int M, int N, int K, int act) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n0 = (blockIdx.x * 4 + wave) * RL_COLS;
    if (n0 >= N) return;
    const int64_t pv = pos ? pos[0] : 0;
    X += pv * x_pos_stride;
    Y += pv * y_pos_stride;
    float4 w[RL_COLS][RL_CHUNKS];
#pragma unroll
    for (int c = 0; c < RL_COLS; ++c) {
        const float* wr = W + (size_t)min(n0 + c, N - 1) * ldw;
#pragma unroll
        for (int i = 0; i < RL_CHUNKS; ++i) {
            const int k = i * 256 + lane * 4;
            w[c][i] = k < K ? *reinterpret_cast<const float4*>(wr + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    for (int m = 0; m < M; ++m) {
        const float* xr = X + (size_t)m * ldx;
        float a[RL_COLS] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < RL_CHUNKS; ++i) {
            const int k = i * 256 + lane * 4;
            if (k < K) {
                const float4 x = *reinterpret_cast<const float4*>(xr + k);
#pragma unroll
                for (int c = 0; c < RL_COLS; ++c)
                    a[c] = fmaf(x.w, w[c][i].w, fmaf(x.z, w[c][i].z, fmaf(x.y, w[c][i].y, fmaf(x.x, w[c][i].x, a[c]))));
            }
        }
#pragma unroll
        for (int c = 0; c < RL_COLS; ++c) a[c] = wave_sum(a[c]);
        if (lane < RL_COLS && n0 + lane < N) {
            const int n = n0 + lane;
            float v = lane == 0 ? a[0] : lane == 1 ? a[1] : lane == 2 ? a[2] : a[3];
            if (bias) v += bias[n];
            if (R) v += R[(size_t)m * ldr + n];
            if (act == 1) v = fmaxf(v, 0.f);
            Y[(size_t)m * ldy + n] = v;
        }
    }
}

}  // namespace

extern "C" int unast_lstm_seq_fwd(const float* xproj, const float* wfrag, const float* b_ih, const float* b_hh, const int* lens, float* y,
                                  float* hfinal, float* cfinal, int B, int T, int ndir, int hidden, hipStream_t stream) {
    UNAST_REQUIRE(xproj && wfrag && b_ih && b_hh && lens && y && hfinal && cfinal, "unast_lstm_seq_fwd: null pointer");
    UNAST_REQUIRE(hidden == RH, "unast_lstm_seq_fwd: built for hidden=%d only (got %d); hidden 64 / 128 are unast_lstm_fwd's", RH, hidden);
    UNAST_REQUIRE(B > 0 && T > 0 && (ndir == 1 || ndir == 2), "unast_lstm_seq_fwd: bad dims (B=%d, T=%d, ndir=%d)", B, T, ndir);
    UNAST_REQUIRE((((uintptr_t)wfrag) & 15) == 0, "unast_lstm_seq_fwd: the W_hh fragments must be 16-byte aligned");
    hipLaunchKernelGGL(lstm_seq_fwd_kernel<false>, dim3((B + SEQ_TILE - 1) / SEQ_TILE, ndir), dim3(SEQ_THREADS), 0, stream, xproj, wfrag, b_ih, b_hh,
                       lens, y, hfinal, cfinal, (float*)nullptr, (float*)nullptr, B, T, ndir);
    return unast_check_launch("unast_lstm_seq_fwd");
}

extern "C" int unast_lstm_seq_fwd_train(const float* xproj, const float* wfrag, const float* b_ih, const float* b_hh, const int* lens, float* y,
                                        float* hfinal, float* cfinal, float* saved, float* hprev, int B, int T, int ndir, int hidden,
                                        hipStream_t stream) {
    UNAST_REQUIRE(xproj && wfrag && b_ih && b_hh && lens && y && hfinal && cfinal && saved && hprev, "unast_lstm_seq_fwd_train: null pointer");
    UNAST_REQUIRE(hidden == RH, "unast_lstm_seq_fwd_train: built for hidden=%d only (got %d)", RH, hidden);
    UNAST_REQUIRE(B > 0 && T > 0 && (ndir == 1 || ndir == 2), "unast_lstm_seq_fwd_train: bad dims (B=%d, T=%d, ndir=%d)", B, T, ndir);
    UNAST_REQUIRE((((uintptr_t)wfrag) & 15) == 0, "unast_lstm_seq_fwd_train: the W_hh fragments must be 16-byte aligned");
    hipLaunchKernelGGL(lstm_seq_fwd_kernel<true>, dim3((B + SEQ_TILE - 1) / SEQ_TILE, ndir), dim3(SEQ_THREADS), 0, stream, xproj, wfrag, b_ih, b_hh,
                       lens, y, hfinal, cfinal, saved, hprev, B, T, ndir);
    return unast_check_launch("unast_lstm_seq_fwd_train");
}

extern "C" int unast_lstm_seq_bwd(const float* dy, const float* dhfinal, const float* dcfinal, const float* wfrag_t, const float* saved,
                                  const int* lens, float* dxproj, int B, int T, int ndir, int hidden, hipStream_t stream) {
    UNAST_REQUIRE(dy && wfrag_t && saved && lens && dxproj, "unast_lstm_seq_bwd: null pointer");
    UNAST_REQUIRE(hidden == RH, "unast_lstm_seq_bwd: built for hidden=%d only (got %d); hidden 64 / 128 are unast_lstm_bwd's", RH, hidden);
    UNAST_REQUIRE(B > 0 && T > 0 && (ndir == 1 || ndir == 2), "unast_lstm_seq_bwd: bad dims (B=%d, T=%d, ndir=%d)", B, T, ndir);
    UNAST_REQUIRE((((uintptr_t)wfrag_t) & 15) == 0, "unast_lstm_seq_bwd: the W_hh fragments must be 16-byte aligned");
    hipLaunchKernelGGL(lstm_seq_bwd_kernel, dim3((B + SEQ_TILE - 1) / SEQ_TILE, ndir), dim3(SEQ_THREADS), 0, stream, dy, dhfinal, dcfinal, wfrag_t,
                       saved, lens, dxproj, B, T, ndir);
    return unast_check_launch("unast_lstm_seq_bwd");
}

extern "C" int unast_rnn_attn_step(int mode, const float* h, int ldh, const float* Wq, const float* mem, const float* v, const float* enc,
                                   const int* lens, float* prev, float* cum, const float* conv_w, const float* dense_w, float* ctx, int ldc,
                                   int B, int Tk, int A, hipStream_t stream) {
    UNAST_REQUIRE(mode == 0 || mode == 1, "unast_rnn_attn_step: mode 0 (Luong) or 1 (location-sensitive), got %d", mode);
    UNAST_REQUIRE(h && Wq && mem && v && enc && lens && ctx, "unast_rnn_attn_step: null pointer");
    UNAST_REQUIRE(mode == 0 || (prev && cum && conv_w && dense_w), "unast_rnn_attn_step: mode 1 needs prev, cum and the location layer's weights");
    UNAST_REQUIRE(B > 0 && Tk > 0 && Tk <= 2048, "unast_rnn_attn_step: B=%d, Tk=%d (1..2048: a sequence's keys are staged in LDS)", B, Tk);
    UNAST_REQUIRE(A > 0 && A <= ATT_MAX_A && A % 4 == 0, "unast_rnn_attn_step: attn_dim must be a multiple of 4, at most %d (got %d)", ATT_MAX_A, A);
    UNAST_REQUIRE(ldh >= RH && ldh % 4 == 0 && ldc >= ENC_D && ldc % 2 == 0, "unast_rnn_attn_step: bad row strides");
    UNAST_REQUIRE(((((uintptr_t)h) | ((uintptr_t)Wq)) & 15) == 0 && ((((uintptr_t)enc) | ((uintptr_t)ctx)) & 7) == 0,
                  "unast_rnn_attn_step: h and Wq must be 16-byte aligned, enc and ctx 8-byte aligned");
    const int Tk4 = (Tk + 3) & ~3;
    size_t fl = 2 * ATT_MAX_A + 16 + Tk4;
    if (mode == 1) fl += 2 * (size_t)(Tk4 + 32) + LOC_F * 2 * LOC_K + (size_t)A * LOC_F;
    hipLaunchKernelGGL(rnn_attn_step_kernel, dim3(B), dim3(ATT_THREADS), fl * sizeof(float), stream, mode, h, ldh, Wq, mem, v, enc, lens, prev, cum,
                       conv_w, dense_w, ctx, ldc, Tk, A);
    return unast_check_launch("unast_rnn_attn_step");
}

extern "C" int unast_lstm_cell(const float* gates, int ldg, float* c, int ldc, float* h, int ldh, int B, int hidden, hipStream_t stream) {
    UNAST_REQUIRE(gates && c && h, "unast_lstm_cell: null pointer");
    UNAST_REQUIRE(hidden == RH, "unast_lstm_cell: built for hidden=%d only (got %d)", RH, hidden);
    UNAST_REQUIRE(B > 0 && ldg >= RG && ldc >= RH && ldh >= RH, "unast_lstm_cell: bad dims");
    hipLaunchKernelGGL(lstm_cell_kernel, dim3((B * RH + 255) / 256), dim3(256), 0, stream, gates, ldg, c, ldc, h, ldh, B);
    return unast_check_launch("unast_lstm_cell");
}

extern "C" int unast_tanh_rows(float* x, int ldx, int rows, int cols, hipStream_t stream) {
    UNAST_REQUIRE(x && rows > 0 && cols > 0 && ldx >= cols, "unast_tanh_rows: bad arguments");
    hipLaunchKernelGGL(tanh_rows_kernel, dim3((rows * cols + 255) / 256), dim3(256), 0, stream, x, ldx, rows, cols);
    return unast_check_launch("unast_tanh_rows");
}

extern "C" int unast_text_window(const int64_t* tokens, int ld_tok, const float* emb, int E, int vocab, float* out, int B, int W, const int64_t* pos,
                                 int teacher_forced, int sos, hipStream_t stream) {
    UNAST_REQUIRE(tokens && emb && out && pos && B > 0 && W > 0 && ld_tok > 0, "unast_text_window: bad arguments");
    UNAST_REQUIRE(E > 0 && E % 4 == 0 && sos >= 0 && sos < vocab && ((((uintptr_t)emb) | ((uintptr_t)out)) & 15) == 0,
                  "unast_text_window: E %% 4 == 0, 16-byte aligned emb and out, sos inside the table");
    const int n = B * W * (E / 4);
    hipLaunchKernelGGL(text_window_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, tokens, ld_tok, emb, E, out, B, W, pos, teacher_forced, sos);
    return unast_check_launch("unast_text_window");
}

extern "C" int unast_window_mask(float* x, int B, int W, int C, const int64_t* pos, int teacher_forced, hipStream_t stream) {
    UNAST_REQUIRE(x && pos && B > 0 && W > 0 && C > 0 && C % 4 == 0 && (((uintptr_t)x) & 15) == 0, "unast_window_mask: bad arguments");
    const int n = B * W * (C / 4);
    hipLaunchKernelGGL(window_mask_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, x, B, W, C, pos, teacher_forced);
    return unast_check_launch("unast_window_mask");
}

extern "C" int unast_pos_advance(int64_t* pos, int* epoch, hipStream_t stream) {
    UNAST_REQUIRE(pos, "unast_pos_advance: null pointer");
    hipLaunchKernelGGL(pos_advance_kernel, dim3(1), dim3(64), 0, stream, pos, epoch);
    return unast_check_launch("unast_pos_advance");
}

extern "C" int unast_rnn_linear(const float* X, int ldx, int64_t x_pos_stride, const float* W, int ldw, const float* bias, const float* R, int ldr,
                                float* Y, int ldy, int64_t y_pos_stride, const int64_t* pos, int M, int N, int K, int act, hipStream_t stream) {
    UNAST_REQUIRE(X && W && Y && M > 0 && N > 0, "unast_rnn_linear: bad arguments");
    UNAST_REQUIRE(K >= 4 && K % 4 == 0 && K <= 256 * RL_CHUNKS, "unast_rnn_linear: K %% 4 == 0 and K <= %d (got %d)", 256 * RL_CHUNKS, K);
    UNAST_REQUIRE(ldx % 4 == 0 && ldw % 4 == 0 && x_pos_stride % 4 == 0 && ((((uintptr_t)X) | ((uintptr_t)W)) & 15) == 0 && ldx >= K && ldw >= K,
                  "unast_rnn_linear: X and W rows must be 16-byte aligned and hold K floats");
    UNAST_REQUIRE(ldy >= N && (!R || ldr >= N) && (act == 0 || act == 1), "unast_rnn_linear: bad output strides or act");
    UNAST_REQUIRE((x_pos_stride == 0 && y_pos_stride == 0) || pos, "unast_rnn_linear: position-indexed rows need pos");
    hipLaunchKernelGGL(rnn_linear_kernel, dim3((N + 4 * RL_COLS - 1) / (4 * RL_COLS)), dim3(256), 0, stream, X, ldx, x_pos_stride, W, ldw, bias, R, ldr, Y, ldy,
                       y_pos_stride, pos, M, N, K, act);
    return unast_check_launch("unast_rnn_linear");
}
