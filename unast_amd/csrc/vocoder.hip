// Kernels of the CBHG vocoder's eval forward (src/network.py:627-655, src/module.py:500-626) that are not contractions: the
// recurrent part of the bidirectional GRU, the stride-1 max pool over the previous frame and the highway combine.  The
// contractions (bank / projection convs with 1..16 taps, highway and GRU input projections, pre / post projection) run on the
// split-bf16 MFMA GEMM (gemm.hip: unast_conv_fwd, unast_gemm).  The eval kernels save nothing for a backward; the training kernels follow them.
#include "common.h"
#include "recur.h"
#include "../../include/unast_hip.h"

#define GH 128            // hidden size per direction
#define GG (3 * GH)       // gate rows (r, z, n)
#define GCH 16            // timesteps of input projections held in registers per chunk (even: the step's parity is i & 1)
#define VLOG2E 1.4426950408889634f

// Recurrent part of nn.GRU (2 directions, zero initial state, ALL T positions of every row: the reference does not pack).
//   r = sigmoid(xr + W_hr h), z = sigmoid(xz + W_hz h), n = tanh(xn + r * (W_hn h + b_hn)), h' = (1 - z) n + z h
// xproj [B,T,2*GG]: per direction [xr | xz | xn] with b_ih (and b_hr, b_hz, which only ever appear summed with it) already added by the
// input-projection GEMM; whh [2][GG][GH]; b_hn [2][GH]; y [B,T,2*GH] = [forward | backward].
//
// One 512-thread workgroup owns one (sequence, direction) for the whole sequence, as lstm_fwd_kernel does.  Wave w owns units
// [16 w, 16 w + 16); lane l = 16 q + c holds row q GH + 16 w + c of W_hh (128 floats in VGPRs, in rotation order: recur.h dot16) for
// q = 0, 1, 2 (r, z, n); lane row 3 carries xn of the unit (its dot product is a copy of row 2's and unused), so that after the
// activation three permlane swaps hand every lane r, z, W_hn h + b_hn and xn of its unit and the state update happens in place, four
// times redundantly.  h crosses waves through a double-buffered LDS vector: 8 ds_read_b32 per lane and ONE barrier per step.
// 384 x 128 multiply-adds per step = 128 v_fmac_dpp per wave, two waves per SIMD: the step is bound by vector issue
// (2 x 128 x 4 cycles per SIMD) plus one LDS round trip and the barrier.
__global__ __launch_bounds__(512) void gru_fwd_kernel(const float* __restrict__ xproj, const float* __restrict__ whh, const float* __restrict__ b_hn,
                                                      float* __restrict__ y, int T) {
    __shared__ __attribute__((aligned(16))) float h_lds[2][GH];
    const int b = blockIdx.x, dir = blockIdx.y, j = threadIdx.x;
    const int wave = j >> 6, lane = j & 63, q = lane >> 4, c16 = lane & 15;
    const int u = 16 * wave + c16;                     // hidden unit of this lane
    const int row = (q < 3 ? q : 2) * GH + u;          // its gate row
    float w[8][16];
    int src[16];
    RotSrc<0>::fill(c16, src);
    const float* wr = whh + ((size_t)dir * GG + row) * GH;
#pragma unroll
    for (int g = 0; g < 8; ++g)
#pragma unroll
        for (int n = 0; n < 16; ++n) w[g][n] = wr[16 * g + src[n]];
    const float bias = b_hn[dir * GH + u];
    if (j < GH) h_lds[0][j] = 0.f;
    __syncthreads();
    const size_t xs = 2 * GG;
    const float* xp = xproj + (size_t)b * T * xs + (size_t)dir * GG + (q == 0 ? 0 : q == 1 ? GH : 2 * GH) + u;
    const int tstep = dir ? -1 : 1;
    const int t0 = dir ? T - 1 : 0;
    float* yp = y + ((size_t)b * T + t0) * (2 * GH) + dir * GH + u;
    const ptrdiff_t y_inc = (ptrdiff_t)tstep * (2 * GH);
    const float act_on = q < 2 ? 1.f : 0.f;
    float h = 0.f;
    float xc[GCH], xn[GCH];
    auto load_chunk = [&](int s0, float (&x)[GCH]) {
#pragma unroll
        for (int i = 0; i < GCH; ++i) {
            const int st = min(s0 + i, T - 1);                     // clamped: a fixed number of loads per chunk
            x[i] = xp[(size_t)(t0 + st * tstep) * xs];
        }
    };
    load_chunk(0, xn);
    for (int s0 = 0; s0 < T; s0 += GCH) {
#pragma unroll
        for (int i = 0; i < GCH; ++i) xc[i] = xn[i];               // the only wait for global loads: once per chunk
        if (s0 + GCH < T) load_chunk(s0 + GCH, xn);
#pragma unroll
        for (int i = 0; i < GCH; ++i) {
            if (s0 + i < T) {                                      // (uniform; a guard, not a break, so that the chunk unrolls)
                const float* hl = h_lds[i & 1];
                float hv[8];
#pragma unroll
                for (int g = 0; g < 8; ++g) hv[g] = hl[16 * g + c16];
                float acc[4];
                dot16<true, false>(w[0], hv[0], acc);
#pragma unroll
                for (int g = 1; g < 8; ++g) dot16<false, false>(w[g], hv[g], acc);
                const float dot = (acc[0] + acc[1]) + (acc[2] + acc[3]);
                const float pre = q == 3 ? xc[i] : dot + (q == 2 ? bias : xc[i]);
                const float sig = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-VLOG2E * pre));
                const float v = act_on != 0.f ? sig : pre;
                float e16, o16, r, hn, z, xnv;
                swap16(v, e16, o16);                               // rows (0, 1): (r, z); rows (2, 3): (W_hn h + b_hn, xn)
                swap32(e16, r, hn);
                swap32(o16, z, xnv);
                const float a = __builtin_fmaf(r, hn, xnv);
                const float n = __builtin_fmaf(__builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f((-2.f * VLOG2E) * a)), 2.f, -1.f);
                h = __builtin_fmaf(z, h - n, n);                   // (1 - z) n + z h
                if (q == 0) h_lds[(i + 1) & 1][u] = h;
                if (q == 1) *yp = h;
                yp += y_inc;
                __syncthreads();
            }
        }
    }
}

// out[b,t,:] = max(in[b,t-1,:], in[b,t,:]), out[b,0,:] = in[b,0,:]: MaxPool1d(2, stride 1, padding 1) without its last column
// (src/module.py:583, 613) on the token-major layout.  C % 4 == 0, 16-byte rows.
__global__ __launch_bounds__(256) void maxpool_prev_kernel(const float* __restrict__ in, int ld_in, float* __restrict__ out, int ld_out, int rows, int T, int C4) {
    const size_t total = (size_t)rows * C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int r = (int)(i / C4), c = (int)(i - (size_t)r * C4) * 4;
        const float4 a = *reinterpret_cast<const float4*>(in + (size_t)r * ld_in + c);
        float4 o = a;
        if (r % T != 0) {
            const float4 p = *reinterpret_cast<const float4*>(in + (size_t)(r - 1) * ld_in + c);
            o = make_float4(fmaxf(a.x, p.x), fmaxf(a.y, p.y), fmaxf(a.z, p.z), fmaxf(a.w, p.w));
        }
        *reinterpret_cast<float4*>(out + (size_t)r * ld_out + c) = o;
    }
}

// One highway layer after its N = 2 C GEMM (src/module.py:524-528): ht [rows, 2 C] = [W1 x + b1 | W2 x + b2];
// out = relu(h) t + x (1 - t), t = sigmoid(.).  out may alias x.
__global__ __launch_bounds__(256) void highway_combine_kernel(const float* __restrict__ ht, int ld_ht, const float* x, int ld_x, float* out, int ld_out,
                                                              int rows, int C4) {
    const size_t total = (size_t)rows * C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int r = (int)(i / C4), c = (int)(i - (size_t)r * C4) * 4;
        const float4 hp = *reinterpret_cast<const float4*>(ht + (size_t)r * ld_ht + c);
        const float4 tp = *reinterpret_cast<const float4*>(ht + (size_t)r * ld_ht + 4 * C4 + c);
        const float4 xv = *reinterpret_cast<const float4*>(x + (size_t)r * ld_x + c);
        const float hh[4] = {hp.x, hp.y, hp.z, hp.w}, tt[4] = {tp.x, tp.y, tp.z, tp.w}, xx[4] = {xv.x, xv.y, xv.z, xv.w};
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t = 1.f / (1.f + __expf(-tt[k]));
            o[k] = __builtin_fmaf(fmaxf(hh[k], 0.f) - xx[k], t, xx[k]);
        }
        *reinterpret_cast<float4*>(out + (size_t)r * ld_out + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ---- training (unast_amd/train_vocoder.py; src/train_vocoder.py:85-94) ------------------------------------------------------------------
// Train forward of the GRU: gru_fwd_kernel's recurrence, bit for bit, that also keeps what the backward needs.  saved [B,T,2,4*GH]: per
// step, direction and unit (r, z, n, W_hn h + b_hn) -- every lane of a unit holds all four after the swaps, lane row q stores the q-th.
// A sibling, not a template: gru_fwd_kernel stays as the compiler sees it today.
__global__ __launch_bounds__(512) void gru_fwd_train_kernel(const float* __restrict__ xproj, const float* __restrict__ whh, const float* __restrict__ b_hn,
                                                            float* __restrict__ y, float* __restrict__ saved, int T) {
    __shared__ __attribute__((aligned(16))) float h_lds[2][GH];
    const int b = blockIdx.x, dir = blockIdx.y, j = threadIdx.x;
    const int wave = j >> 6, lane = j & 63, q = lane >> 4, c16 = lane & 15;
    const int u = 16 * wave + c16;
    const int row = (q < 3 ? q : 2) * GH + u;
    float w[8][16];
    int src[16];
    RotSrc<0>::fill(c16, src);
    const float* wr = whh + ((size_t)dir * GG + row) * GH;
#pragma unroll
    for (int g = 0; g < 8; ++g)
#pragma unroll
        for (int n = 0; n < 16; ++n) w[g][n] = wr[16 * g + src[n]];
    const float bias = b_hn[dir * GH + u];
    if (j < GH) h_lds[0][j] = 0.f;
    __syncthreads();
    const size_t xs = 2 * GG;
    const float* xp = xproj + (size_t)b * T * xs + (size_t)dir * GG + (q == 0 ? 0 : q == 1 ? GH : 2 * GH) + u;
    const int tstep = dir ? -1 : 1;
    const int t0 = dir ? T - 1 : 0;
    float* yp = y + ((size_t)b * T + t0) * (2 * GH) + dir * GH + u;
    const ptrdiff_t y_inc = (ptrdiff_t)tstep * (2 * GH);
    float* sp = saved + (((size_t)b * T + t0) * 2 + dir) * (4 * GH) + q * GH + u;
    const ptrdiff_t s_inc = (ptrdiff_t)tstep * (2 * 4 * GH);
    const float act_on = q < 2 ? 1.f : 0.f;
    float h = 0.f;
    float xc[GCH], xn[GCH];
    auto load_chunk = [&](int s0, float (&x)[GCH]) {
#pragma unroll
        for (int i = 0; i < GCH; ++i) {
            const int st = min(s0 + i, T - 1);
            x[i] = xp[(size_t)(t0 + st * tstep) * xs];
        }
    };
    load_chunk(0, xn);
    for (int s0 = 0; s0 < T; s0 += GCH) {
#pragma unroll
        for (int i = 0; i < GCH; ++i) xc[i] = xn[i];
        if (s0 + GCH < T) load_chunk(s0 + GCH, xn);
#pragma unroll
        for (int i = 0; i < GCH; ++i) {
            if (s0 + i < T) {
                const float* hl = h_lds[i & 1];
                float hv[8];
#pragma unroll
                for (int g = 0; g < 8; ++g) hv[g] = hl[16 * g + c16];
                float acc[4];
                dot16<true, false>(w[0], hv[0], acc);
#pragma unroll
                for (int g = 1; g < 8; ++g) dot16<false, false>(w[g], hv[g], acc);
                const float dot = (acc[0] + acc[1]) + (acc[2] + acc[3]);
                const float pre = q == 3 ? xc[i] : dot + (q == 2 ? bias : xc[i]);
                const float sig = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-VLOG2E * pre));
                const float v = act_on != 0.f ? sig : pre;
                float e16, o16, r, hn, z, xnv;
                swap16(v, e16, o16);
                swap32(e16, r, hn);
                swap32(o16, z, xnv);
                const float a = __builtin_fmaf(r, hn, xnv);
                const float n = __builtin_fmaf(__builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f((-2.f * VLOG2E) * a)), 2.f, -1.f);
                h = __builtin_fmaf(z, h - n, n);
                if (q == 0) h_lds[(i + 1) & 1][u] = h;
                if (q == 1) *yp = h;
                *sp = q == 0 ? r : q == 1 ? z : q == 2 ? n : hn;
                yp += y_inc;
                sp += s_inc;
                __syncthreads();
            }
        }
    }
}

// Backward of the recurrence: one 512-thread workgroup per (sequence, direction) walks the forward's steps in reverse, as
// lstm_bwd128_kernel does.  Lane 16 q + c of wave w is unit k = 16 w + c; rows q = 0, 1, 2 hold column k of the r, z, n block of W_hh as
// 128 floats in rotation order (row 3: zeros -- it computes da for the store and adds nothing to the sum).  With dht = dh + dy_t:
//   da = dht (1 - z)(1 - n^2)   dz_pre = dht (h_prev - n) z (1 - z)   dr_pre = da hn r (1 - r)   (hn = W_hn h_prev + b_hn)
//   dh_prev = z dht + W_hr^T dr_pre + W_hz^T dz_pre + W_hn^T (r da)
// Every lane's gradient is dht times a factor formed off the dependent chain, once per chunk of GBCH steps whose saved values are loaded
// one chunk ahead.  The three gate gradients cross waves through a double-buffered LDS vector, ONE barrier per step.  Outputs:
// dxg [B,T,2,GG] = (dr_pre, dz_pre, da), the gradient of the input projections; dhn [B,T,2,GH] = r da, the n block of the hidden side.
#define GBCH 4            // steps per chunk (even: the LDS buffer's parity is i & 1)
__global__ __launch_bounds__(512) void gru_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ saved,
                                                      const float* __restrict__ whh, float* __restrict__ dxg, float* __restrict__ dhn, int T) {
    __shared__ __attribute__((aligned(16))) float dg_lds[2][GG];
    const int b = blockIdx.x, dir = blockIdx.y, j = threadIdx.x;
    const int wave = j >> 6, lane = j & 63, q = lane >> 4, c16 = lane & 15;
    const int k = 16 * wave + c16;
    const int qb = q < 3 ? q : 2;
    float wt[8][16];
    int src[16];
    RotSrc<0>::fill(c16, src);
    const float* wr = whh + ((size_t)dir * GG + qb * GH) * GH + k;
#pragma unroll
    for (int jw = 0; jw < 8; ++jw)
#pragma unroll
        for (int n = 0; n < 16; ++n) {
            const float wv = wr[(size_t)(16 * ((wave + jw) & 7) + src[n]) * GH];
            wt[jw][n] = q < 3 ? wv : 0.f;
        }
    int ds[8];                                               // (ds[0], this wave's own gradients, is unused: they are in a register)
#pragma unroll
    for (int jw = 1; jw < 8; ++jw) ds[jw] = qb * GH + 16 * ((wave + jw) & 7) + c16;
    const int tstep = dir ? 1 : -1;                         // reverse of the forward processing order
    const int t0 = dir ? 0 : T - 1;
    const float* sv_p = saved + ((size_t)b * T * 2 + dir) * (4 * GH) + k;        // + t * 2 * 4 GH
    const float* dy_p = dy + (size_t)b * T * (2 * GH) + dir * GH + k;            // + t * 2 GH (y likewise)
    const float* y_p = y + (size_t)b * T * (2 * GH) + dir * GH + k;
    float* op = q == 2 ? dhn + ((size_t)b * T + t0) * (2 * GH) + dir * GH + k
                       : dxg + ((size_t)b * T + t0) * (2 * GG) + dir * GG + (q == 3 ? 2 : q) * GH + k;
    const ptrdiff_t o_inc = (ptrdiff_t)tstep * (q == 2 ? 2 * GH : 2 * GG);
    float vn[GBCH][6];                                       // r, z, n, hn, dy, h_prev of GBCH steps
    auto load_chunk = [&](int r0) {
#pragma unroll
        for (int i = 0; i < GBCH; ++i) {
            const int t = t0 + min(r0 + i, T - 1) * tstep, tp = t0 + min(r0 + i + 1, T - 1) * tstep;      // clamped: a fixed number of loads per chunk
            const float* s = sv_p + (size_t)t * (2 * 4 * GH);
            vn[i][0] = s[0]; vn[i][1] = s[GH]; vn[i][2] = s[2 * GH]; vn[i][3] = s[3 * GH];
            vn[i][4] = dy_p[(size_t)t * (2 * GH)];
            vn[i][5] = y_p[(size_t)tp * (2 * GH)];
        }
    };
    float dh = 0.f;
    load_chunk(0);
    for (int r0 = 0; r0 < T; r0 += GBCH) {
        float cy[GBCH], cz[GBCH], cd[GBCH];
#pragma unroll
        for (int i = 0; i < GBCH; ++i) {
            const float r = vn[i][0], z = vn[i][1], n = vn[i][2], hn = vn[i][3];
            const float hp = (r0 + i >= T - 1) ? 0.f : vn[i][5];              // (scalar condition) the first forward step starts from h = 0
            const float om = (1.f - z) * (1.f - n * n);
            cy[i] = q == 0 ? om * hn * (r * (1.f - r)) : q == 1 ? (hp - n) * (z * (1.f - z)) : q == 2 ? r * om : om;
            cz[i] = z;
            cd[i] = vn[i][4];
        }
        if (r0 + GBCH < T) load_chunk(r0 + GBCH);
#pragma unroll
        for (int i = 0; i < GBCH; ++i) {
            if (r0 + i < T) {                               // (uniform; a guard, not a break, so that the chunk unrolls)
                const float dht = dh + cd[i];
                const float mine = dht * cy[i];
                float* dgw = dg_lds[i & 1];
                if (q < 3) dgw[q * GH + k] = mine;
                *op = mine;
                op += o_inc;
                float acc[4];
                dot16<true, true>(wt[0], mine, acc);        // this wave's own 16 gradients: in front of the barrier, under the LDS write
                __syncthreads();
                float dv[8];
#pragma unroll
                for (int jw = 1; jw < 8; ++jw) dv[jw] = dgw[ds[jw]];
#pragma unroll
                for (int jw = 1; jw < 8; ++jw) dot16<false, false>(wt[jw], dv[jw], acc);
                float e16, o16, lo, up;
                swap16((acc[0] + acc[1]) + (acc[2] + acc[3]), e16, o16);
                swap32(e16 + o16, lo, up);
                dh = __builtin_fmaf(cz[i], dht, lo + up);   // the same sum in every lane of the unit (row 3 adds 0)
            }
        }
    }
}

// Backward of maxpool_prev: dx[t] = dy[t] [t == 0 or x[t-1] < x[t]] + dy[t+1] [x[t] >= x[t+1]] -- a tie goes to the EARLIER frame, torch's
// rule (post-ReLU zeros tie all the time).  accumulate: dx += ; gate: the result is kept where x[t] > 0 (the ReLU that produced x, read
// from the stored forward output itself) and zero elsewhere.
__global__ __launch_bounds__(256) void maxpool_prev_bwd_kernel(const float* __restrict__ dy, int ld_dy, const float* __restrict__ x, int ld_x, float* dx, int ld_dx,
                                                               int rows, int T, int C4, int accumulate, int gate) {
    const size_t total = (size_t)rows * C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int r = (int)(i / C4), c = (int)(i - (size_t)r * C4) * 4, t = r % T;
        const float4 xv = *reinterpret_cast<const float4*>(x + (size_t)r * ld_x + c);
        const float4 dv = *reinterpret_cast<const float4*>(dy + (size_t)r * ld_dy + c);
        const float xc[4] = {xv.x, xv.y, xv.z, xv.w}, dc[4] = {dv.x, dv.y, dv.z, dv.w};
        float o[4];
        if (t != 0) {
            const float4 p = *reinterpret_cast<const float4*>(x + (size_t)(r - 1) * ld_x + c);
            const float xp[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = xp[e] < xc[e] ? dc[e] : 0.f;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = dc[e];
        }
        if (t + 1 < T) {
            const float4 nx = *reinterpret_cast<const float4*>(x + (size_t)(r + 1) * ld_x + c);
            const float4 nd = *reinterpret_cast<const float4*>(dy + (size_t)(r + 1) * ld_dy + c);
            const float xn[4] = {nx.x, nx.y, nx.z, nx.w}, dn[4] = {nd.x, nd.y, nd.z, nd.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] += xc[e] >= xn[e] ? dn[e] : 0.f;
        }
        float* dp = dx + (size_t)r * ld_dx + c;
        if (accumulate) {
            const float4 a = *reinterpret_cast<const float4*>(dp);
            o[0] += a.x; o[1] += a.y; o[2] += a.z; o[3] += a.w;
        }
        if (gate) {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = xc[e] > 0.f ? o[e] : 0.f;
        }
        *reinterpret_cast<float4*>(dp) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// dy = dy where y > 0, else 0: the backward of a ReLU from its stored output (projection 1 of CBHG).
__global__ __launch_bounds__(256) void relu_bwd_kernel(float* dy, int ld_dy, const float* __restrict__ y, int ld_y, int rows, int C4) {
    const size_t total = (size_t)rows * C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int r = (int)(i / C4), c = (int)(i - (size_t)r * C4) * 4;
        const float4 yv = *reinterpret_cast<const float4*>(y + (size_t)r * ld_y + c);
        float4 d = *reinterpret_cast<float4*>(dy + (size_t)r * ld_dy + c);
        d.x = yv.x > 0.f ? d.x : 0.f; d.y = yv.y > 0.f ? d.y : 0.f; d.z = yv.z > 0.f ? d.z : 0.f; d.w = yv.w > 0.f ? d.w : 0.f;
        *reinterpret_cast<float4*>(dy + (size_t)r * ld_dy + c) = d;
    }
}

// Backward of highway_combine from the saved pre-activations ht = [h | t'] and the layer's input x (t = sigmoid(t')):
//   d_pre = [dout t [h > 0] | dout (relu(h) - x) t (1 - t)],   dx = dout (1 - t)  (the direct part; the GEMM adds d_pre W with beta = 1).
// dx may alias dout.
__global__ __launch_bounds__(256) void highway_combine_bwd_kernel(const float* dout, int ld_do, const float* __restrict__ ht, int ld_ht, const float* __restrict__ x, int ld_x,
                                                                  float* __restrict__ dpre, int ld_dp, float* dx, int ld_dx, int rows, int C4) {
    const size_t total = (size_t)rows * C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int r = (int)(i / C4), c = (int)(i - (size_t)r * C4) * 4;
        const float4 dv = *reinterpret_cast<const float4*>(dout + (size_t)r * ld_do + c);
        const float4 hp = *reinterpret_cast<const float4*>(ht + (size_t)r * ld_ht + c);
        const float4 tp = *reinterpret_cast<const float4*>(ht + (size_t)r * ld_ht + 4 * C4 + c);
        const float4 xv = *reinterpret_cast<const float4*>(x + (size_t)r * ld_x + c);
        const float dd[4] = {dv.x, dv.y, dv.z, dv.w}, hh[4] = {hp.x, hp.y, hp.z, hp.w}, tt[4] = {tp.x, tp.y, tp.z, tp.w}, xx[4] = {xv.x, xv.y, xv.z, xv.w};
        float dh[4], dt[4], o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t = 1.f / (1.f + __expf(-tt[e]));
            dh[e] = hh[e] > 0.f ? dd[e] * t : 0.f;
            dt[e] = dd[e] * (fmaxf(hh[e], 0.f) - xx[e]) * (t * (1.f - t));
            o[e] = dd[e] * (1.f - t);
        }
        *reinterpret_cast<float4*>(dpre + (size_t)r * ld_dp + c) = make_float4(dh[0], dh[1], dh[2], dh[3]);
        *reinterpret_cast<float4*>(dpre + (size_t)r * ld_dp + 4 * C4 + c) = make_float4(dt[0], dt[1], dt[2], dt[3]);
        *reinterpret_cast<float4*>(dx + (size_t)r * ld_dx + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// loss += sum |pred - mag| (l2 = 0) or sum (pred - mag)^2 (l2 = 1) over [rows, F], accumulated in fp64 (src/train_vocoder.py:41-46, 91);
// dpred (may be NULL) = sign(diff) (sign(0) = 0, as torch's) or 2 diff in the same pass, zeros in the columns F .. cols - 1 of its rows (cols = F rounded up to 4 when the
// row stride has room: the padding the input-gradient GEMM reads).
__global__ __launch_bounds__(256) void sum_loss_kernel(const float* __restrict__ pred, int ld_p, const float* __restrict__ mag, int ld_m, float* __restrict__ dpred, int ld_dp,
                                                       int rows, int F, int cols, int l2, double* __restrict__ loss) {
    __shared__ double red[256];
    const size_t total = (size_t)rows * cols;
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int r = (int)(i / cols), c = (int)(i - (size_t)r * cols);
        float g = 0.f;
        if (c < F) {
            const float d = pred[(size_t)r * ld_p + c] - mag[(size_t)r * ld_m + c];
            if (l2) { acc += (double)d * (double)d; g = 2.f * d; }
            else { acc += (double)fabsf(d); g = d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f; }
        }
        if (dpred) dpred[(size_t)r * ld_dp + c] = g;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd(loss, red[0]);
}

// The pieces of x that the GEMM's split-bf16 operand preparation (common.h: hi = RNE_bf16(x), lo = RNE_bf16(x - hi)) keeps and drops,
// as fp32 tensors: hi; rest = x - hi (exact); resid = rest - RNE_bf16(rest), what both bf16 parts leave out.  Any output may be NULL.
// The train forward's convolutions are formed from them as conv(hi, W) + conv(rest, W) + conv(x, resid(W)): every product the
// three-term form drops in one launch (x_lo W_lo and the parts below 2^-17 of either operand) is picked up by another.
__global__ __launch_bounds__(256) void split_parts_kernel(const float* __restrict__ x, float* __restrict__ hi, float* __restrict__ rest,
                                                          float* __restrict__ resid, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float v = x[i];
        const float h = (float)(__bf16)v;
        const float r = v - h;
        if (hi) hi[i] = h;
        if (rest) rest[i] = r;
        if (resid) resid[i] = r - (float)(__bf16)r;
    }
}

static bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
static unsigned ew_blocks(size_t work) {
    size_t blocks = (work + 255) / 256;
    return (unsigned)(blocks > 4096 ? 4096 : blocks);
}

extern "C" int unast_gru_fwd(const float* xproj, const float* whh, const float* b_hn, float* y, int B, int T, int hidden, hipStream_t stream) {
    UNAST_REQUIRE(xproj && whh && b_hn && y, "unast_gru_fwd: null pointer");
    UNAST_REQUIRE(hidden == GH, "unast_gru_fwd: this build supports hidden=%d only (got %d)", GH, hidden);
    UNAST_REQUIRE(B > 0 && B <= 65535 && T > 0, "unast_gru_fwd: bad dims B=%d T=%d", B, T);
    hipLaunchKernelGGL(gru_fwd_kernel, dim3(B, 2), dim3(512), 0, stream, xproj, whh, b_hn, y, T);
    return unast_check_launch("unast_gru_fwd");
}

extern "C" int unast_maxpool_prev(const float* in, int ld_in, float* out, int ld_out, int B, int T, int C, hipStream_t stream) {
    UNAST_REQUIRE(in && out && B > 0 && T > 0 && C > 0, "unast_maxpool_prev: bad arguments");
    UNAST_REQUIRE((C & 3) == 0 && (ld_in & 3) == 0 && (ld_out & 3) == 0 && ld_in >= C && ld_out >= C && al16(in) && al16(out),
                  "unast_maxpool_prev: C and the row strides must be multiples of 4 floats, rows 16-byte aligned");
    UNAST_REQUIRE((long long)B * T <= 0x7FFFFFFF, "unast_maxpool_prev: too many rows");
    hipLaunchKernelGGL(maxpool_prev_kernel, dim3(ew_blocks((size_t)B * T * (C / 4))), dim3(256), 0, stream, in, ld_in, out, ld_out, B * T, T, C / 4);
    return unast_check_launch("unast_maxpool_prev");
}

extern "C" int unast_highway_combine(const float* ht, int ld_ht, const float* x, int ld_x, float* out, int ld_out, int rows, int C, hipStream_t stream) {
    UNAST_REQUIRE(ht && x && out && rows > 0 && C > 0, "unast_highway_combine: bad arguments");
    UNAST_REQUIRE((C & 3) == 0 && (ld_ht & 3) == 0 && (ld_x & 3) == 0 && (ld_out & 3) == 0 && ld_ht >= 2 * C && ld_x >= C && ld_out >= C &&
                  al16(ht) && al16(x) && al16(out), "unast_highway_combine: C and the row strides must be multiples of 4 floats, rows 16-byte aligned");
    hipLaunchKernelGGL(highway_combine_kernel, dim3(ew_blocks((size_t)rows * (C / 4))), dim3(256), 0, stream, ht, ld_ht, x, ld_x, out, ld_out, rows, C / 4);
    return unast_check_launch("unast_highway_combine");
}

extern "C" int unast_gru_fwd_train(const float* xproj, const float* whh, const float* b_hn, float* y, float* saved, int B, int T, int hidden,
                                   hipStream_t stream) {
    UNAST_REQUIRE(xproj && whh && b_hn && y && saved, "unast_gru_fwd_train: null pointer");
    UNAST_REQUIRE(hidden == GH, "unast_gru_fwd_train: this build supports hidden=%d only (got %d)", GH, hidden);
    UNAST_REQUIRE(B > 0 && B <= 65535 && T > 0, "unast_gru_fwd_train: bad dims B=%d T=%d", B, T);
    hipLaunchKernelGGL(gru_fwd_train_kernel, dim3(B, 2), dim3(512), 0, stream, xproj, whh, b_hn, y, saved, T);
    return unast_check_launch("unast_gru_fwd_train");
}

extern "C" int unast_gru_bwd(const float* dy, const float* y, const float* saved, const float* whh, float* dx_gates, float* dhn, int B, int T,
                             int hidden, hipStream_t stream) {
    UNAST_REQUIRE(dy && y && saved && whh && dx_gates && dhn, "unast_gru_bwd: null pointer");
    UNAST_REQUIRE(hidden == GH, "unast_gru_bwd: this build supports hidden=%d only (got %d)", GH, hidden);
    UNAST_REQUIRE(B > 0 && B <= 65535 && T > 0, "unast_gru_bwd: bad dims B=%d T=%d", B, T);
    hipLaunchKernelGGL(gru_bwd_kernel, dim3(B, 2), dim3(512), 0, stream, dy, y, saved, whh, dx_gates, dhn, T);
    return unast_check_launch("unast_gru_bwd");
}

extern "C" int unast_maxpool_prev_bwd(const float* dy, int ld_dy, const float* x, int ld_x, float* dx, int ld_dx, int B, int T, int C,
                                      int accumulate, int relu_gate, hipStream_t stream) {
    UNAST_REQUIRE(dy && x && dx && B > 0 && T > 0 && C > 0, "unast_maxpool_prev_bwd: bad arguments");
    UNAST_REQUIRE((C & 3) == 0 && (ld_dy & 3) == 0 && (ld_x & 3) == 0 && (ld_dx & 3) == 0 && ld_dy >= C && ld_x >= C && ld_dx >= C &&
                  al16(dy) && al16(x) && al16(dx), "unast_maxpool_prev_bwd: C and the row strides must be multiples of 4 floats, rows 16-byte aligned");
    UNAST_REQUIRE((long long)B * T <= 0x7FFFFFFF, "unast_maxpool_prev_bwd: too many rows");
    hipLaunchKernelGGL(maxpool_prev_bwd_kernel, dim3(ew_blocks((size_t)B * T * (C / 4))), dim3(256), 0, stream, dy, ld_dy, x, ld_x, dx, ld_dx, B * T, T, C / 4,
                       accumulate, relu_gate);
    return unast_check_launch("unast_maxpool_prev_bwd");
}

extern "C" int unast_relu_bwd(float* dy, int ld_dy, const float* y, int ld_y, int rows, int C, hipStream_t stream) {
    UNAST_REQUIRE(dy && y && rows > 0 && C > 0, "unast_relu_bwd: bad arguments");
    UNAST_REQUIRE((C & 3) == 0 && (ld_dy & 3) == 0 && (ld_y & 3) == 0 && ld_dy >= C && ld_y >= C && al16(dy) && al16(y),
                  "unast_relu_bwd: C and the row strides must be multiples of 4 floats, rows 16-byte aligned");
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(ew_blocks((size_t)rows * (C / 4))), dim3(256), 0, stream, dy, ld_dy, y, ld_y, rows, C / 4);
    return unast_check_launch("unast_relu_bwd");
}

extern "C" int unast_highway_combine_bwd(const float* dout, int ld_do, const float* ht, int ld_ht, const float* x, int ld_x, float* dpre, int ld_dp,
                                         float* dx, int ld_dx, int rows, int C, hipStream_t stream) {
    UNAST_REQUIRE(dout && ht && x && dpre && dx && rows > 0 && C > 0, "unast_highway_combine_bwd: bad arguments");
    UNAST_REQUIRE((C & 3) == 0 && (ld_do & 3) == 0 && (ld_ht & 3) == 0 && (ld_x & 3) == 0 && (ld_dp & 3) == 0 && (ld_dx & 3) == 0 && ld_do >= C &&
                  ld_ht >= 2 * C && ld_x >= C && ld_dp >= 2 * C && ld_dx >= C && al16(dout) && al16(ht) && al16(x) && al16(dpre) && al16(dx),
                  "unast_highway_combine_bwd: C and the row strides must be multiples of 4 floats, rows 16-byte aligned");
    hipLaunchKernelGGL(highway_combine_bwd_kernel, dim3(ew_blocks((size_t)rows * (C / 4))), dim3(256), 0, stream, dout, ld_do, ht, ld_ht, x, ld_x, dpre, ld_dp,
                       dx, ld_dx, rows, C / 4);
    return unast_check_launch("unast_highway_combine_bwd");
}

extern "C" int unast_sum_loss(const float* pred, int ld_pred, const float* mag, int ld_mag, float* dpred, int ld_dpred, int rows, int F, int l2,
                              double* loss, hipStream_t stream) {
    UNAST_REQUIRE(pred && mag && loss && rows > 0 && F > 0, "unast_sum_loss: bad arguments");
    UNAST_REQUIRE(ld_pred >= F && ld_mag >= F && (!dpred || ld_dpred >= F), "unast_sum_loss: row strides shorter than the rows");
    UNAST_REQUIRE((((uintptr_t)loss) & 7) == 0, "unast_sum_loss: the loss accumulator is a double");
    const int F4 = (F + 3) & ~3;
    const int cols = (dpred && ld_dpred >= F4) ? F4 : F;         // the zero padding of a 16-byte row stride, where the rows have room for it
    hipLaunchKernelGGL(sum_loss_kernel, dim3(ew_blocks((size_t)rows * cols)), dim3(256), 0, stream, pred, ld_pred, mag, ld_mag, dpred, ld_dpred, rows, F, cols,
                       l2 ? 1 : 0, loss);
    return unast_check_launch("unast_sum_loss");
}

extern "C" int unast_split_parts(const float* x, float* hi, float* rest, float* resid, int64_t n, hipStream_t stream) {
    UNAST_REQUIRE(x && n > 0 && (hi || rest || resid), "unast_split_parts: bad arguments");
    hipLaunchKernelGGL(split_parts_kernel, dim3(ew_blocks((size_t)n)), dim3(256), 0, stream, x, hi, rest, resid, (size_t)n);
    return unast_check_launch("unast_split_parts");
}
