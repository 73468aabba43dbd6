// Kernels of the RNN model family (TextRNN / SpeechRNN, src/network.py:279-402, 503-624; src/module.py:297-497) at the width every
// full-size reference config uses, hidden 256: the eval path, the encoders' training and the SpeechRNN decoder's (unast_amd/train_rnn.py).
//   lstm_seq_fwd_kernel   recurrence of one packed nn.LSTM layer (src/module.py:306, 315-317); <true> also saves what the backward reads
//   lstm_seq_bwd_kernel   backpropagation through time of that recurrence
//   rnn_attn_step_kernel  one step of Luong / location-sensitive additive attention (src/module.py:395-497)
//   lstm_cell_kernel      pointwise cell update of one decoder step (the nn.LSTM call of src/module.py:371 at sequence length 1)
//   rnn_attn_step_bwd_kernel, lstm_cell_train_kernel, lstm_cell_bwd_kernel, tanh_bwd_kernel   one position of the decoder's training loops
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
// TRAIN (unast_rnn_attn_step_train): the same instructions on ctx and the weights, out of place -- prev / cum are read from prev_in / cum_in
// (row stride ld_in) and the weights / cum + weights written to prev / cum (row stride ld_out); <false> ignores those three arguments.
template <bool TRAIN>
__global__ __launch_bounds__(ATT_THREADS) void rnn_attn_step_kernel(int mode, const float* __restrict__ hq, int ldq, const float* __restrict__ Wq,
                                                                    const float* __restrict__ mem, const float* __restrict__ vw,
                                                                    const float* __restrict__ enc, const int* __restrict__ lens, float* __restrict__ prev,
                                                                    float* __restrict__ cum, const float* __restrict__ conv_w,
                                                                    const float* __restrict__ dense_w, float* __restrict__ ctx, int ldc, int Tk, int A,
                                                                    const float* __restrict__ prev_in, const float* __restrict__ cum_in, int ld_in,
                                                                    int ld_out) {
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
            if constexpr (TRAIN) pc[i] = (t >= 0 && t < Tk) ? (ch ? cum_in : prev_in)[(size_t)b * ld_in + t] : 0.f;
            else pc[i] = (t >= 0 && t < Tk) ? (ch ? cum : prev)[(size_t)b * Tk + t] : 0.f;
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
        if constexpr (TRAIN) {
            prev[(size_t)b * ld_out + t] = w;
            if (mode == 1) cum[(size_t)b * ld_out + t] = pc[ldp + LOC_PAD + t] + w;
        } else {
            if (prev) prev[(size_t)b * Tk + t] = w;
            if (mode == 1) cum[(size_t)b * Tk + t] = pc[ldp + LOC_PAD + t] + w;
        }
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

// ---- decoder training: what unast_amd.train_rnn.decoder_forward / decoder_backward launch per position -------------------------------------
// lstm_cell_kernel's arithmetic (the same expressions, so h and c_t carry its bits) out of place, storing what the backward reads:
// saved[b] = (i, f, g, o, c_t) as [5,256].  hd != NULL: a second copy of h for the next layer, times mask (nn.LSTM's inter-layer dropout as a
// factor tensor, 0 or 1/(1-p)) when there is one; the carried h stays undropped.
__global__ void lstm_cell_train_kernel(const float* __restrict__ gates, int ldg, const float* __restrict__ cprev, int ldcp, float* __restrict__ saved,
                                       int lds, float* __restrict__ h, int ldh, const float* __restrict__ mask, int ldm, float* __restrict__ hd, int ldhd,
                                       int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * RH) return;
    const int b = i / RH, u = i - b * RH;
    const float* g = gates + (size_t)b * ldg + u;
    const float ig = sigmoidf_(g[0]), fg = sigmoidf_(g[RH]), gg = tanhf(g[2 * RH]), og = sigmoidf_(g[3 * RH]);
    const float cn = fg * cprev[(size_t)b * ldcp + u] + ig * gg;
    float* s = saved + (size_t)b * lds + u;
    s[0] = ig; s[RH] = fg; s[2 * RH] = gg; s[3 * RH] = og; s[4 * RH] = cn;
    const float hn = og * tanhf(cn);
    h[(size_t)b * ldh + u] = hn;
    if (hd) hd[(size_t)b * ldhd + u] = mask ? hn * mask[(size_t)b * ldm + u] : hn;
}

// Backward of one cell update: dh_total = dh + dh2 (* mask), dc = dc_in + dh_total o (1 - tanh(c_t)^2) with tanh(c_t) recomputed;
// dG [B,1024] = gradient of the gate pre-activations, dc_out = dc f (dc_out may be dc_in: one thread reads and writes an element).
__global__ void lstm_cell_bwd_kernel(const float* __restrict__ dh, int lddh, const float* __restrict__ dh2, int lddh2, const float* __restrict__ mask,
                                     int ldm, const float* dc_in, int lddc, const float* __restrict__ saved, int lds,
                                     const float* __restrict__ cprev, int ldcp, float* __restrict__ dG, int ldg, float* dc_out, int lddco, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * RH) return;
    const int b = i / RH, u = i - b * RH;
    float d = dh ? dh[(size_t)b * lddh + u] : 0.f;
    if (dh2) {
        const float e = dh2[(size_t)b * lddh2 + u];
        d += mask ? e * mask[(size_t)b * ldm + u] : e;
    }
    const float* s = saved + (size_t)b * lds + u;
    const float ig = s[0], fg = s[RH], gg = s[2 * RH], og = s[3 * RH], tc = tanhf(s[4 * RH]);
    const float dc = (dc_in ? dc_in[(size_t)b * lddc + u] : 0.f) + d * og * (1.f - tc * tc);
    float* o = dG + (size_t)b * ldg + u;
    o[0] = dc * gg * ig * (1.f - ig);
    o[RH] = dc * cprev[(size_t)b * ldcp + u] * fg * (1.f - fg);
    o[2 * RH] = dc * ig * (1.f - gg * gg);
    o[3 * RH] = d * tc * og * (1.f - og);
    dc_out[(size_t)b * lddco + u] = dc * fg;
}

// dy *= 1 - y^2 in place: backward of y = tanh(.) from the stored output.
__global__ void tanh_bwd_kernel(float* __restrict__ dy, int lddy, const float* __restrict__ y, int ldy, int rows, int cols) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cols) return;
    const int r = i / cols, c = i - r * cols;
    const float t = y[(size_t)r * ldy + c];
    dy[(size_t)r * lddy + c] *= 1.f - t * t;
}

// Backward of one rnn_attn_step_kernel position, the same decomposition: one workgroup per sequence, fp32 on the vector ALUs, no atomics and
// no workgroup waits on another, so two runs give the same bits.  Everything a sequence's workgroup adds to (d_mem[b], the per-sequence partial
// sums of d_v, d_dense and d_conv_w) is owned by it; the partial sums are reduced over b after the loop in a fixed order.
//   dw[t]   = dwa[t] + dwb[t] + enc[b,t] . d_ctx[b]                  (t < len; the incoming gradient of the weights: LSA's d_prev of the next
//                                                                     position and the running d_cum)
//   de[t]   = w[t] (dw[t] - sum_s w[s] dw[s])                         softmax backward over the live keys (masked keys: w = 0, no gradient)
//   dx[t,a] = de[t] v[a] (1 - th^2), th = tanh(qp[a] + loc[t,a] + mem[b,t,a]) recomputed with the forward's expressions
//   d_q[a] = sum_t dx[t,a], d_h = d_q Wq, d_mem[b,t,:] += dx[t,:], d_v[a] += sum_t de[t] th[t,a]
//   LSA: F[t,f] = conv(prev, cum)[t,f] recomputed, dF[t,f] = sum_a dx[t,a] dense[a,f]; d_dense[a,f] += sum_t dx[t,a] F[t,f];
//        d_conv[f,ch,k] += sum_t dF[t,f] in[ch][t+k-15]; d_in[ch][s] = sum_{f,k} conv[f,ch,k] dF[s-k+15,f] (transposed conv, zero halo).
// Keys t >= len: enc, mem, prev, cum, dwa and dwb are never read there; d_prev / d_cum are written as exact zeros, d_mem is not touched.
// LDS (floats): qp[64] | vs[64] | red[16] | sdq[64] | part[4*2*64] | sdc[512] | sdw[Tk4] | sw[Tk4] and in LSA mode pc[2][Tk4+32] | conv[1984] |
// dense[A*32].  ws (global, per sequence Tk*(64+2A) floats, L2-resident): F | dF | dx | u = de th, written by the thread that owns key t and
// read by all after a barrier (phase 3: a thread owns a few output elements and makes one pass over the keys).
__global__ __launch_bounds__(ATT_THREADS) void rnn_attn_step_bwd_kernel(
    int mode, const float* __restrict__ dctx, int lddc, const float* __restrict__ w, const float* __restrict__ prev, const float* __restrict__ cum, int ldw,
    const float* __restrict__ hq, int ldq, const float* __restrict__ Wq, const float* __restrict__ mem, const float* __restrict__ vw,
    const float* __restrict__ enc, const int* __restrict__ lens, const float* __restrict__ conv_w, const float* __restrict__ dense_w,
    const float* __restrict__ dwa, const float* __restrict__ dwb, int carry, int ldd, float* __restrict__ dh, int lddh, float* __restrict__ dq, int lddq,
    float* dmem, float* __restrict__ dv_part, float* __restrict__ ddense_part, float* __restrict__ dconv_part, float* __restrict__ dprev,
    float* __restrict__ dcum, float* ws, int Tk, int A) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Tk4 = (Tk + 3) & ~3;
    float* qp = smem;
    float* vs = qp + ATT_MAX_A;
    float* red = vs + ATT_MAX_A;
    float* sdq = red + 16;
    float* part = sdq + ATT_MAX_A;
    float* sdc = part + 8 * 64;
    float* sdw = sdc + ENC_D;
    float* sw = sdw + Tk4;
    float* pc = sw + Tk4;
    const int ldp = Tk4 + 32;
    float* convs = pc + 2 * ldp;
    float* denses = convs + LOC_F * 2 * LOC_K;
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int len = min(max(lens[b], 0), Tk);

    {   // the forward's query-side projection, instruction for instruction
        const float4 hv = *reinterpret_cast<const float4*>(hq + (size_t)b * ldq + lane * 4);
        for (int a = wave; a < A; a += ATT_THREADS / 64) {
            const float4 wv = *reinterpret_cast<const float4*>(Wq + (size_t)a * RH + lane * 4);
            const float s = wave_sum((wv.x * hv.x + wv.y * hv.y) + (wv.z * hv.z + wv.w * hv.w));
            if (lane == 0) qp[a] = s;
        }
    }
    if (tid < A) vs[tid] = vw[tid];
    sdc[tid] = dctx[(size_t)b * lddc + tid];
    sdc[tid + ATT_THREADS] = dctx[(size_t)b * lddc + tid + ATT_THREADS];
    for (int t = tid; t < Tk4; t += ATT_THREADS) sw[t] = t < len ? w[(size_t)b * ldw + t] : 0.f;
    if (mode == 1) {
        for (int i = tid; i < 2 * ldp; i += ATT_THREADS) {
            const int ch = i / ldp, t = i - ch * ldp - LOC_PAD;
            pc[i] = (t >= 0 && t < len) ? (ch ? cum : prev)[(size_t)b * ldw + t] : 0.f;      // (the forward's weights are exact zeros at t >= len)
        }
        for (int i = tid; i < LOC_F * 2 * LOC_K; i += ATT_THREADS) convs[i] = conv_w[i];
        for (int i = tid; i < A * LOC_F; i += ATT_THREADS) denses[i] = dense_w[i];
    }
    __syncthreads();

    // phase 1: dw[t] = incoming + enc[b,t] . d_ctx[b], a wave per key row (2 KiB contiguous)
    {
        const float4 c0 = reinterpret_cast<const float4*>(sdc)[lane], c1 = reinterpret_cast<const float4*>(sdc)[64 + lane];
        for (int t0 = wave; t0 < len; t0 += 4 * (ATT_THREADS / 64)) {                        // four rows in flight per wave
            float s[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = t0 + u * (ATT_THREADS / 64);
                s[u] = 0.f;
                if (t < len) {
                    const float4* e = reinterpret_cast<const float4*>(enc + ((size_t)b * Tk + t) * ENC_D);
                    const float4 e0 = e[lane], e1 = e[64 + lane];
                    s[u] = ((e0.x * c0.x + e0.y * c0.y) + (e0.z * c0.z + e0.w * c0.w)) + ((e1.x * c1.x + e1.y * c1.y) + (e1.z * c1.z + e1.w * c1.w));
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] = wave_sum(s[u]);
            if (lane == 0) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int t = t0 + u * (ATT_THREADS / 64);
                    if (t < len) {
                        float v = s[u];
                        if (dwa) v += dwa[(size_t)b * ldd + t];
                        if (dwb) v += dwb[(size_t)b * ldd + t];
                        sdw[t] = v;
                    }
                }
            }
        }
    }
    __syncthreads();
    float dot = 0.f;
    for (int t = tid; t < len; t += ATT_THREADS) dot = fmaf(sw[t], sdw[t], dot);
    dot = block_sum(dot, red);
    for (int t = tid; t < len; t += ATT_THREADS) sdw[t] = sw[t] * (sdw[t] - dot);          // de[t]; each thread keeps to its own keys below

    // phase 2: a thread per key: tanh argument recomputed, dx / u / F / dF to the workspace, d_mem += dx
    const size_t wsb = (size_t)Tk * (2 * LOC_F + 2 * A);
    float* wsF = ws + (size_t)b * wsb;
    float* wsdF = wsF + (size_t)Tk * LOC_F;
    float* wsdx = wsdF + (size_t)Tk * LOC_F;
    float* wsu = wsdx + (size_t)Tk * A;
    for (int t = tid; t < len; t += ATT_THREADS) {
        float f[LOC_F], df[LOC_F];
        if (mode == 1) {
#pragma unroll
            for (int i = 0; i < LOC_F; ++i) { f[i] = 0.f; df[i] = 0.f; }
            for (int ch = 0; ch < 2; ++ch)
                for (int k = 0; k < LOC_K; ++k) {
                    const float x = pc[ch * ldp + t + k];
#pragma unroll
                    for (int i = 0; i < LOC_F; ++i) f[i] = fmaf(convs[(i * 2 + ch) * LOC_K + k], x, f[i]);
                }
        }
        const float de = sdw[t];
        const float* mrow = mem + ((size_t)b * Tk + t) * A;
        float* dmrow = dmem + ((size_t)b * Tk + t) * A;
        for (int a = 0; a < A; ++a) {
            float x = qp[a];
            if (mode == 1) {
                float loc = 0.f;
#pragma unroll
                for (int i = 0; i < LOC_F; ++i) loc = fmaf(denses[a * LOC_F + i], f[i], loc);
                x += loc;
            }
            x += mrow[a];
            const float th = tanhf(x);
            const float dxv = de * vs[a] * (1.f - th * th);
            wsu[(size_t)t * A + a] = de * th;
            wsdx[(size_t)t * A + a] = dxv;
            dmrow[a] += dxv;
            if (mode == 1) {
#pragma unroll
                for (int i = 0; i < LOC_F; ++i) df[i] = fmaf(dxv, denses[a * LOC_F + i], df[i]);
            }
        }
        if (mode == 1) {
#pragma unroll
            for (int i = 0; i < LOC_F; ++i) { wsF[(size_t)t * LOC_F + i] = f[i]; wsdF[(size_t)t * LOC_F + i] = df[i]; }
        }
    }
    __syncthreads();

    // phase 3: d_q and d_v: wave w sums the keys t = w (mod 4), lane = a; the four partial sums are combined in a fixed order
    if (lane < A) {
        float sq = 0.f, sv = 0.f;
#pragma unroll 4
        for (int t = wave; t < len; t += ATT_THREADS / 64) { sq += wsdx[(size_t)t * A + lane]; sv += wsu[(size_t)t * A + lane]; }
        part[(wave * 2 + 0) * 64 + lane] = sq;
        part[(wave * 2 + 1) * 64 + lane] = sv;
    }
    __syncthreads();
    if (tid < A) {
        const float q = (part[0 * 64 + tid] + part[2 * 64 + tid]) + (part[4 * 64 + tid] + part[6 * 64 + tid]);
        sdq[tid] = q;
        dq[(size_t)b * lddq + tid] = q;
        dv_part[(size_t)b * A + tid] += (part[1 * 64 + tid] + part[3 * 64 + tid]) + (part[5 * 64 + tid] + part[7 * 64 + tid]);
    }
    __syncthreads();
    {   // d_h[b, j] = sum_a d_q[a] Wq[a, j]
        float s = 0.f;
        for (int a = 0; a < A; ++a) s = fmaf(sdq[a], Wq[(size_t)a * RH + tid], s);
        dh[(size_t)b * lddh + tid] = s;
    }
    if (mode != 1) return;
    {   // d_dense[a, f] += sum_t dx[t,a] F[t,f]: lane = f, a thread owns a = tid / 32 + 8 r; one pass over the keys for all its outputs
        const int fi = tid & 31, a0 = tid >> 5;
        float acc[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[r] = 0.f;
#pragma unroll 2
        for (int t = 0; t < len; ++t) {
            const float fv = wsF[(size_t)t * LOC_F + fi];
            const float* dxr = wsdx + (size_t)t * A;
#pragma unroll
            for (int r = 0; r < 8; ++r)
                if (a0 + 8 * r < A) acc[r] = fmaf(dxr[a0 + 8 * r], fv, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < 8; ++r)
            if (a0 + 8 * r < A) ddense_part[((size_t)b * A + a0 + 8 * r) * LOC_F + fi] += acc[r];
    }
    {   // d_conv[f, ch, k] += sum_t dF[t,f] in[ch][t+k-15]: lane = (ch, k) (62 of 64), a thread owns f = tid / 64 + 4 r
        const int j = tid & 63, fg = tid >> 6;
        if (j < 2 * LOC_K) {
            const int ch = j / LOC_K, k = j - ch * LOC_K;
            const float* pin = pc + ch * ldp + k;
            float acc[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) acc[r] = 0.f;
#pragma unroll 2
            for (int t = 0; t < len; ++t) {
                const float x = pin[t];
                const float* dfr = wsdF + (size_t)t * LOC_F + fg;
#pragma unroll
                for (int r = 0; r < 8; ++r) acc[r] = fmaf(dfr[4 * r], x, acc[r]);
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) dconv_part[((size_t)b * LOC_F + fg + 4 * r) * 2 * LOC_K + j] += acc[r];
        }
    }
    for (int s_ = tid; s_ < Tk; s_ += ATT_THREADS) {
        float a0 = 0.f, a1 = 0.f;
        if (s_ < len) {
            for (int k = 0; k < LOC_K; ++k) {
                const int t = s_ - k + LOC_PAD;
                if (t < 0 || t >= len) continue;
                const float* row = wsdF + (size_t)t * LOC_F;
#pragma unroll
                for (int i = 0; i < LOC_F; ++i) {
                    a0 = fmaf(convs[(i * 2 + 0) * LOC_K + k], row[i], a0);
                    a1 = fmaf(convs[(i * 2 + 1) * LOC_K + k], row[i], a1);
                }
            }
            if (carry && dwb) a1 += dwb[(size_t)b * ldd + s_];
        }
        dprev[(size_t)b * ldd + s_] = a0;
        dcum[(size_t)b * ldd + s_] = a1;
    }
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
    hipLaunchKernelGGL(rnn_attn_step_kernel<false>, dim3(B), dim3(ATT_THREADS), fl * sizeof(float), stream, mode, h, ldh, Wq, mem, v, enc, lens, prev, cum,
                       conv_w, dense_w, ctx, ldc, Tk, A, (const float*)nullptr, (const float*)nullptr, 0, 0);
    return unast_check_launch("unast_rnn_attn_step");
}

extern "C" int unast_lstm_cell(const float* gates, int ldg, float* c, int ldc, float* h, int ldh, int B, int hidden, hipStream_t stream) {
    UNAST_REQUIRE(gates && c && h, "unast_lstm_cell: null pointer");
    UNAST_REQUIRE(hidden == RH, "unast_lstm_cell: built for hidden=%d only (got %d)", RH, hidden);
    UNAST_REQUIRE(B > 0 && ldg >= RG && ldc >= RH && ldh >= RH, "unast_lstm_cell: bad dims");
    hipLaunchKernelGGL(lstm_cell_kernel, dim3((B * RH + 255) / 256), dim3(256), 0, stream, gates, ldg, c, ldc, h, ldh, B);
    return unast_check_launch("unast_lstm_cell");
}

extern "C" int unast_rnn_attn_step_train(int mode, const float* h, int ldh, const float* Wq, const float* mem, const float* v, const float* enc,
                                         const int* lens, const float* prev_in, const float* cum_in, int ld_in, float* w_out, float* cum_out,
                                         int ld_out, const float* conv_w, const float* dense_w, float* ctx, int ldc, int B, int Tk, int A,
                                         hipStream_t stream) {
    UNAST_REQUIRE(mode == 0 || mode == 1, "unast_rnn_attn_step_train: mode 0 (Luong) or 1 (location-sensitive), got %d", mode);
    UNAST_REQUIRE(h && Wq && mem && v && enc && lens && ctx && w_out, "unast_rnn_attn_step_train: null pointer");
    UNAST_REQUIRE(mode == 0 || (prev_in && cum_in && cum_out && conv_w && dense_w),
                  "unast_rnn_attn_step_train: mode 1 needs prev_in, cum_in, cum_out and the location layer's weights");
    UNAST_REQUIRE(B > 0 && Tk > 0 && Tk <= 2048, "unast_rnn_attn_step_train: B=%d, Tk=%d (1..2048: a sequence's keys are staged in LDS)", B, Tk);
    UNAST_REQUIRE(A > 0 && A <= ATT_MAX_A && A % 4 == 0, "unast_rnn_attn_step_train: attn_dim must be a multiple of 4, at most %d (got %d)", ATT_MAX_A, A);
    UNAST_REQUIRE(ldh >= RH && ldh % 4 == 0 && ldc >= ENC_D && ldc % 2 == 0 && ld_out >= Tk && (mode == 0 || ld_in >= Tk),
                  "unast_rnn_attn_step_train: bad row strides");
    UNAST_REQUIRE(mode == 0 || (w_out != prev_in && w_out != cum_in && cum_out != cum_in && cum_out != prev_in && w_out != cum_out),
                  "unast_rnn_attn_step_train: the outputs must not be the inputs (out of place; unast_rnn_attn_step is the in-place form)");
    UNAST_REQUIRE(((((uintptr_t)h) | ((uintptr_t)Wq)) & 15) == 0 && ((((uintptr_t)enc) | ((uintptr_t)ctx)) & 7) == 0,
                  "unast_rnn_attn_step_train: h and Wq must be 16-byte aligned, enc and ctx 8-byte aligned");
    const int Tk4 = (Tk + 3) & ~3;
    size_t fl = 2 * ATT_MAX_A + 16 + Tk4;
    if (mode == 1) fl += 2 * (size_t)(Tk4 + 32) + LOC_F * 2 * LOC_K + (size_t)A * LOC_F;
    hipLaunchKernelGGL(rnn_attn_step_kernel<true>, dim3(B), dim3(ATT_THREADS), fl * sizeof(float), stream, mode, h, ldh, Wq, mem, v, enc, lens, w_out,
                       cum_out, conv_w, dense_w, ctx, ldc, Tk, A, prev_in, cum_in, ld_in, ld_out);
    return unast_check_launch("unast_rnn_attn_step_train");
}

extern "C" int64_t unast_rnn_attn_step_bwd_ws_floats(int B, int Tk, int A) {
    if (B <= 0 || Tk <= 0 || A <= 0) return 0;
    return (int64_t)B * Tk * (2 * LOC_F + 2 * A);
}

extern "C" int unast_rnn_attn_step_bwd(int mode, const float* d_ctx, int lddc, const float* w, const float* prev, const float* cum, int ldw,
                                       const float* h, int ldh, const float* Wq, const float* mem, const float* v, const float* enc, const int* lens,
                                       const float* conv_w, const float* dense_w, const float* d_w_a, const float* d_w_b, int carry, int ldd,
                                       float* d_h, int lddh, float* d_q, int lddq, float* d_mem, float* dv_part, float* ddense_part,
                                       float* dconv_part, float* d_prev, float* d_cum, float* ws, int64_t ws_floats, int B, int Tk, int A,
                                       hipStream_t stream) {
    UNAST_REQUIRE(mode == 0 || mode == 1, "unast_rnn_attn_step_bwd: mode 0 (Luong) or 1 (location-sensitive), got %d", mode);
    UNAST_REQUIRE(d_ctx && w && h && Wq && mem && v && enc && lens && d_h && d_q && d_mem && dv_part && ws, "unast_rnn_attn_step_bwd: null pointer");
    UNAST_REQUIRE(mode == 0 || (prev && cum && conv_w && dense_w && ddense_part && dconv_part && d_prev && d_cum),
                  "unast_rnn_attn_step_bwd: mode 1 needs prev, cum, the location layer's weights, their partial sums, d_prev and d_cum");
    UNAST_REQUIRE(B > 0 && Tk > 0 && Tk <= 2048, "unast_rnn_attn_step_bwd: B=%d, Tk=%d (1..2048: a sequence's keys are staged in LDS)", B, Tk);
    UNAST_REQUIRE(A > 0 && A <= ATT_MAX_A && A % 4 == 0, "unast_rnn_attn_step_bwd: attn_dim must be a multiple of 4, at most %d (got %d)", ATT_MAX_A, A);
    UNAST_REQUIRE(ldh >= RH && ldh % 4 == 0 && lddc >= ENC_D && ldw >= Tk && lddh >= RH && lddq >= A && ((!d_w_a && !d_w_b && mode == 0) || ldd >= Tk),
                  "unast_rnn_attn_step_bwd: bad row strides");
    UNAST_REQUIRE(((((uintptr_t)h) | ((uintptr_t)Wq) | ((uintptr_t)enc) | ((uintptr_t)ws)) & 15) == 0,
                  "unast_rnn_attn_step_bwd: h, Wq, enc and ws must be 16-byte aligned");
    UNAST_REQUIRE(ws_floats >= unast_rnn_attn_step_bwd_ws_floats(B, Tk, A), "unast_rnn_attn_step_bwd: workspace too small (%lld floats)", (long long)ws_floats);
    UNAST_REQUIRE(mode == 0 || ((d_prev != d_w_a) && (d_cum != d_w_b) && (d_prev != d_w_b) && (d_cum != d_w_a) && d_prev != d_cum),
                  "unast_rnn_attn_step_bwd: d_prev / d_cum must not be the incoming buffers (keys are read by other threads than write them)");
    const int Tk4 = (Tk + 3) & ~3;
    size_t fl = 3 * ATT_MAX_A + 16 + 8 * 64 + ENC_D + 2 * (size_t)Tk4;
    if (mode == 1) fl += 2 * (size_t)(Tk4 + 32) + LOC_F * 2 * LOC_K + (size_t)A * LOC_F;
    hipLaunchKernelGGL(rnn_attn_step_bwd_kernel, dim3(B), dim3(ATT_THREADS), fl * sizeof(float), stream, mode, d_ctx, lddc, w, prev, cum, ldw, h, ldh, Wq, mem,
                       v, enc, lens, conv_w, dense_w, d_w_a, d_w_b, carry, ldd, d_h, lddh, d_q, lddq, d_mem, dv_part, ddense_part, dconv_part, d_prev,
                       d_cum, ws, Tk, A);
    return unast_check_launch("unast_rnn_attn_step_bwd");
}

extern "C" int unast_lstm_cell_train(const float* gates, int ldg, const float* c_prev, int ldcp, float* saved, int lds, float* h, int ldh,
                                     const float* mask, int ldm, float* hd, int ldhd, int B, int hidden, hipStream_t stream) {
    UNAST_REQUIRE(gates && c_prev && saved && h, "unast_lstm_cell_train: null pointer");
    UNAST_REQUIRE(hidden == RH, "unast_lstm_cell_train: built for hidden=%d only (got %d)", RH, hidden);
    UNAST_REQUIRE(B > 0 && ldg >= RG && ldcp >= RH && lds >= 5 * RH && ldh >= RH && (!hd || ldhd >= RH) && (!mask || (hd && ldm >= RH)),
                  "unast_lstm_cell_train: bad dims (a mask needs hd)");
    hipLaunchKernelGGL(lstm_cell_train_kernel, dim3((B * RH + 255) / 256), dim3(256), 0, stream, gates, ldg, c_prev, ldcp, saved, lds, h, ldh, mask, ldm, hd,
                       ldhd, B);
    return unast_check_launch("unast_lstm_cell_train");
}

extern "C" int unast_lstm_cell_bwd(const float* dh, int lddh, const float* dh2, int lddh2, const float* mask, int ldm, const float* dc_in, int lddc,
                                   const float* saved, int lds, const float* c_prev, int ldcp, float* dG, int ldg, float* dc_out, int lddco, int B,
                                   int hidden, hipStream_t stream) {
    UNAST_REQUIRE(saved && c_prev && dG && dc_out, "unast_lstm_cell_bwd: null pointer");
    UNAST_REQUIRE(hidden == RH, "unast_lstm_cell_bwd: built for hidden=%d only (got %d)", RH, hidden);
    UNAST_REQUIRE(B > 0 && ldg >= RG && ldcp >= RH && lds >= 5 * RH && lddco >= RH && (!dh || lddh >= RH) && (!dh2 || lddh2 >= RH) &&
                      (!mask || (dh2 && ldm >= RH)) && (!dc_in || lddc >= RH),
                  "unast_lstm_cell_bwd: bad dims (a mask needs dh2)");
    hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3((B * RH + 255) / 256), dim3(256), 0, stream, dh, lddh, dh2, lddh2, mask, ldm, dc_in, lddc, saved, lds,
                       c_prev, ldcp, dG, ldg, dc_out, lddco, B);
    return unast_check_launch("unast_lstm_cell_bwd");
}

extern "C" int unast_tanh_bwd(float* dy, int lddy, const float* y, int ldy, int rows, int cols, hipStream_t stream) {
    UNAST_REQUIRE(dy && y && rows > 0 && cols > 0 && lddy >= cols && ldy >= cols && (long long)rows * cols <= 0x7FFFFFFF, "unast_tanh_bwd: bad arguments");
    hipLaunchKernelGGL(tanh_bwd_kernel, dim3((rows * cols + 255) / 256), dim3(256), 0, stream, dy, lddy, y, ldy, rows, cols);
    return unast_check_launch("unast_tanh_bwd");
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
