// Kernels of the CBHG vocoder's eval forward (src/network.py:627-655, src/module.py:500-626) that are not contractions: the
// recurrent part of the bidirectional GRU, the stride-1 max pool over the previous frame and the highway combine.  The
// contractions (bank / projection convs with 1..16 taps, highway and GRU input projections, pre / post projection) run on the
// split-bf16 MFMA GEMM (gemm.hip: unast_conv_fwd, unast_gemm).  Inference only: nothing is saved for a backward.
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
