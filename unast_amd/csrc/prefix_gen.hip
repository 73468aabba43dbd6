// The single-prefix prenet of TextRNN's greedy generation in TRAIN mode (UNAST.cm_speech_in, src/network.py:114-123, 586-617): at position i
// TextPrenet runs over the one prefix [SOS, c_0 .. c_{i-1}] of every sequence -- an ordinary [B, L = i + 1, 256] batch -- with fresh dropout masks,
// batch statistics over its B*L rows and one momentum update of the running statistics.  Four launches per position:
//
//   pgen_conv_kernel x 3    one prenet stage over the B*L rows: the loader produces the stage's input rows (stage 1: the embedding gather from the
//                           generated tokens + emb_dropout; stages 2, 3: the previous stage's BatchNorm + ReLU + dropout, its statistics reduced from
//                           that stage's per-workgroup partial sums), the 5-tap 'same' convolution runs on v_mfma_f32_16x16x4_f32 (exact fp32
//                           products), the epilogue adds the bias, stores the pre-BatchNorm output and this workgroup's fp64 sums of x and x^2
//   pgen_finish_kernel      stage 3's BatchNorm + ReLU + dropout on each sequence's LAST row -> pre [B,256]; the momentum update of the three
//                           BatchNorms and num_batches_tracked += 1, both only while some sequence is still running (a device flag)
//
// No workgroup waits on another and there are no atomics: sums cross workgroups at launch boundaries, reduced in tile order (two runs give the
// same bits).  Rows past B*L of any buffer and tokens past L - 1 are never read.  Beside them the small kernels that end a position of either
// generation (argmax / stop rule -> tokens, frames, lengths and the running flag, all gated on that flag) and the activation + dropout whose mask
// row is (position, sequence).
#include "common.h"
#include <string.h>

namespace {

constexpr int PG_C = 256;                 // output channels of every stage
constexpr int PG_ROWS = 32;               // prefix rows per workgroup (two MFMA row tiles)
constexpr int PG_COLS = 64;               // output channels per workgroup (four MFMA column tiles)
constexpr int PG_TAPS = 5;
constexpr int PG_LROWS = PG_ROWS + 4;     // with the two rows of halo on either side
constexpr int PG_MAXCIN = 256;
constexpr int PG_LDX = PG_MAXCIN + 4;     // LDS row (floats), padded by one 16-byte slot

struct PGenConv {
    const float* x;                       // stages 2, 3: the previous stage's pre-BatchNorm output [N,256]
    const double* part_in;                // its partial sums [ntiles][2][256]
    const float* gamma; const float* beta; float eps;
    const int64_t* tokens; int ld_tok;    // stage 1: generated tokens [B, ld_tok]; prefix row j > 0 is tokens[b, j-1], row 0 is SOS
    const float* emb; int vocab, sos;
    const float* W;                       // [256][5][Cin], tap-major
    const float* bias;
    float* z;                             // [N,256]
    double* part_out;                     // [ntiles][2][256]
    int B, L, Cin;
    uint32_t thresh; float dscale; uint32_t seed, stream, row0;
};

// mean and 1/sqrt(var + eps) of channel c from the tile partials in tile order (fp64), as unast_prefix_bn_fwd forms them
__device__ __forceinline__ void pgen_stats(const double* __restrict__ part, int ntiles, int c, double n, double& mu, double& var) {
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 8
    for (int k = 0; k < ntiles; ++k) { s1 += part[(size_t)k * 2 * PG_C + c]; s2 += part[(size_t)k * 2 * PG_C + PG_C + c]; }
    mu = s1 / n;
    var = s2 / n - mu * mu;
    if (var < 0.0) var = 0.0;
}

template <bool EMBED>
__global__ __launch_bounds__(256) void pgen_conv_kernel(const PGenConv p) {
    __shared__ __attribute__((aligned(16))) float xs[PG_LROWS * PG_LDX];       // the input rows; afterwards the four waves' partial products
    __shared__ float s_m[PG_C], s_rs[PG_C];
    __shared__ double s_red[4][PG_COLS][2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, j = lane & 15;
    const int N = p.B * p.L, L = p.L, Cin = p.Cin;
    const int r0 = blockIdx.x * PG_ROWS, co0 = blockIdx.y * PG_COLS;

    if (!EMBED) {
        double mu, var;
        pgen_stats(p.part_in, gridDim.x, tid, (double)N, mu, var);
        s_m[tid] = (float)mu;
        s_rs[tid] = (float)(1.0 / sqrt(var + (double)p.eps));
        __syncthreads();
    }

    // ---- the loader: rows r0 - 2 .. r0 + 33 of the stage's input, zeros outside [0, N) ------------------------------------------------------------
    const int cq = Cin >> 2;
    for (int i = tid; i < PG_LROWS * cq; i += 256) {
        const int lr = i / cq, c = (i - lr * cq) * 4;
        const int r = r0 - 2 + lr;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if (r >= 0 && r < N) {
            bool live = true;
            if (EMBED) {
                const int b = r / L, jj = r - b * L;
                const int64_t id = jj == 0 ? (int64_t)p.sos : p.tokens[(size_t)b * p.ld_tok + jj - 1];
                live = id >= 0 && id < p.vocab;
                if (live) {
                    const float4 v = *reinterpret_cast<const float4*>(p.emb + (size_t)id * Cin + c);
                    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
                }
            } else {
                const float4 v = *reinterpret_cast<const float4*>(p.x + (size_t)r * PG_C + c);
                const float4 ga = *reinterpret_cast<const float4*>(p.gamma + c), be = *reinterpret_cast<const float4*>(p.beta + c);
                o[0] = fmaxf((v.x - s_m[c]) * s_rs[c] * ga.x + be.x, 0.f);
                o[1] = fmaxf((v.y - s_m[c + 1]) * s_rs[c + 1] * ga.y + be.y, 0.f);
                o[2] = fmaxf((v.z - s_m[c + 2]) * s_rs[c + 2] * ga.z + be.z, 0.f);
                o[3] = fmaxf((v.w - s_m[c + 3]) * s_rs[c + 3] * ga.w + be.w, 0.f);
            }
            if (live && p.thresh) {
                const uint32_t rkey = rng_row_key(p.seed, p.stream, p.row0 + (uint32_t)r);
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = rng_keep(rkey, c + e, p.thresh) ? o[e] * p.dscale : 0.f;
            }
        }
        *reinterpret_cast<float4*>(&xs[lr * PG_LDX + c]) = make_float4(o[0], o[1], o[2], o[3]);
    }
    __syncthreads();

    // ---- the contraction: wave w takes input channels [w Cin/4, (w+1) Cin/4) of all five taps, for both row tiles and the four column tiles ---------
    // MFMA k order as in lstm_seq_fwd_kernel: k-step e of a group of 16 channels takes channel 16 g + 4 (lane >> 4) + e from both operands.
    // A sequence's own zero padding: tap t of row (b, jj) reads row jj + t - 2 of the SAME sequence or nothing.
    uint32_t ok[2] = {0u, 0u};                                                 // bit t: tap t of this lane's row of tile s is inside its sequence
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int r = r0 + 16 * s + j;
        const int b = r / L, jj = r - b * L;
#pragma unroll
        for (int t = 0; t < PG_TAPS; ++t)
            if (r < N && jj + t - 2 >= 0 && jj + t - 2 < L) ok[s] |= 1u << t;
    }
    const bool tile1 = r0 + 16 < N;                                            // (tile 0 always holds a live row)
    f32x4 acc[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[s][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int cw = Cin >> 2, ng = cw >> 4;
    const float* wrow = p.W + (size_t)(co0 + j) * PG_TAPS * Cin + wave * cw + 4 * q;
#pragma unroll 1
    for (int t = 0; t < PG_TAPS; ++t) {
        for (int g = 0; g < ng; ++g) {
            const int ci = wave * cw + 16 * g + 4 * q;
            float4 w[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) w[ct] = *reinterpret_cast<const float4*>(wrow + (size_t)ct * 16 * PG_TAPS * Cin + t * Cin + 16 * g);
            float4 a[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                a[s] = *reinterpret_cast<const float4*>(&xs[(16 * s + j + t) * PG_LDX + ci]);
                if (!((ok[s] >> t) & 1u)) a[s] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (s == 1 && !tile1) continue;
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) acc[s][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].x, w[ct].x, acc[s][ct], 0, 0, 0);
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) acc[s][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].y, w[ct].y, acc[s][ct], 0, 0, 0);
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) acc[s][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].z, w[ct].z, acc[s][ct], 0, 0, 0);
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) acc[s][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].w, w[ct].w, acc[s][ct], 0, 0, 0);
            }
        }
    }
    __syncthreads();                                                           // every wave is done with the input rows
    float* red = xs;                                                           // [4 waves][32 rows][64 columns]
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[(wave * PG_ROWS + 16 * s + 4 * q + r) * PG_COLS + 16 * ct + j] = acc[s][ct][r];
    __syncthreads();

    // ---- the epilogue: waves summed in order, + bias, the store, this workgroup's column sums ---------------------------------------------------------
    const int col = tid & 63, rg = tid >> 6;
    const float bv = p.bias[co0 + col];
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int k = 0; k < PG_ROWS / 4; ++k) {
        const int row = rg * (PG_ROWS / 4) + k, r = r0 + row;
        if (r < N) {
            float v = red[row * PG_COLS + col] + red[(PG_ROWS + row) * PG_COLS + col];
            v += red[(2 * PG_ROWS + row) * PG_COLS + col];
            v += red[(3 * PG_ROWS + row) * PG_COLS + col];
            v += bv;
            p.z[(size_t)r * PG_C + co0 + col] = v;
            s1 += (double)v;
            s2 += (double)v * (double)v;
        }
    }
    s_red[rg][col][0] = s1;
    s_red[rg][col][1] = s2;
    __syncthreads();
    if (tid < 2 * PG_COLS) {
        const int c = tid & 63, which = tid >> 6;
        const double a = ((s_red[0][c][which] + s_red[1][c][which]) + s_red[2][c][which]) + s_red[3][c][which];
        p.part_out[((size_t)blockIdx.x * 2 + which) * PG_C + co0 + c] = a;
    }
}

struct PGenFinish {
    const float* z3; const double* part;  // part: [3][ntiles][2][256]
    const float* gamma; const float* beta;
    float* pre; int ldp;
    float* rm[3]; float* rv[3]; long long* nbt[3];
    float eps, mom[3];
    const int* running;
    int B, L, ntiles;
    uint32_t thresh; float dscale; uint32_t seed, stream, row0;
};

// block s = prenet stage s: its statistics once more from the partials; block 2 also writes pre
__global__ __launch_bounds__(256) void pgen_finish_kernel(const PGenFinish p) {
    const int s = blockIdx.x, c = threadIdx.x;
    const int N = p.B * p.L;
    double mu, var;
    pgen_stats(p.part + (size_t)s * p.ntiles * 2 * PG_C, p.ntiles, c, (double)N, mu, var);
    const float mean = (float)mu;
    if (s == 2) {
        const float rstd = (float)(1.0 / sqrt(var + (double)p.eps));
        const float ga = p.gamma[c], be = p.beta[c];
        for (int b = 0; b < p.B; ++b) {
            const int r = b * p.L + p.L - 1;
            float a = fmaxf((p.z3[(size_t)r * PG_C + c] - mean) * rstd * ga + be, 0.f);
            if (p.thresh) a = rng_keep(rng_row_key(p.seed, p.stream, p.row0 + (uint32_t)r), c, p.thresh) ? a * p.dscale : 0.f;
            p.pre[(size_t)b * p.ldp + c] = a;
        }
    }
    const bool run = p.running ? p.running[0] != 0 : true;
    if (!run) return;
    if (p.rm[s]) {
        const float varu = (float)(N > 1 ? var * (double)N / ((double)N - 1.0) : var);
        const float m = p.mom[s];
        p.rm[s][c] = (1.f - m) * p.rm[s][c] + m * mean;
        p.rv[s][c] = (1.f - m) * p.rv[s][c] + m * varu;
    }
    if (c == 0 && p.nbt[s]) *p.nbt[s] += 1;
}

// out = drop_b(drop_a(act(x))) over [B, C]; the masks' row is row0 + b (row0 = position * B).  act: 0 none, 1 tanh, 2 relu
__global__ __launch_bounds__(256) void pgen_act_drop_kernel(const float* __restrict__ x, int ldx, float* __restrict__ out, int ldo, int B, int C, int act,
                                                            uint32_t th_a, float sc_a, uint32_t st_a, uint32_t th_b, float sc_b, uint32_t st_b, uint32_t seed,
                                                            uint32_t row0) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, c = i - b * C;
    float v = x[(size_t)b * ldx + c];
    if (act == 1) v = tanhf(v);
    else if (act == 2) v = fmaxf(v, 0.f);
    if (th_a) v = rng_keep(rng_row_key(seed, st_a, row0 + (uint32_t)b), c, th_a) ? v * sc_a : 0.f;
    if (th_b) v = rng_keep(rng_row_key(seed, st_b, row0 + (uint32_t)b), c, th_b) ? v * sc_b : 0.f;
    out[(size_t)b * ldo + c] = v;
}

// The end of a text position (src/network.py:601-609), one workgroup, everything under the running flag: token = first maximum of the logits ->
// tokens[b, pos]; a sequence that draws EOS for the first time gets the length pos + 1; running = some sequence has not stopped.
__global__ __launch_bounds__(256) void pgen_end_text_kernel(const float* __restrict__ logits, int ld, int V, int B, int64_t* __restrict__ tokens, int ld_tok,
                                                            int pos, int64_t* __restrict__ stop_lens, int64_t max_len, int eos, int* __restrict__ running) {
    const bool run = running[0] != 0;
    __syncthreads();                                                           // every thread has read the flag before thread 0 rewrites it
    if (!run) return;
    int open = 0;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float* xr = logits + (size_t)b * ld;
        float best = xr[0];
        int bi = 0;
        for (int c = 1; c < V; ++c) {                                          // first maximum, as torch.argmax
            const float v = xr[c];
            if (v > best) { best = v; bi = c; }
        }
        tokens[(size_t)b * ld_tok + pos] = bi;
        int64_t sl = stop_lens[b];
        if (bi == eos && sl == max_len) { sl = pos + 1; stop_lens[b] = sl; }
        open |= sl == max_len;
    }
    open = __syncthreads_or(open);
    if (threadIdx.x == 0) running[0] = open ? 1 : 0;
}

// The end of a speech position (src/network.py:326-337): head [B, >= M + 1] = [frame | stop logit] -> frames[b, pos + 1], stops[b, pos]; the stop
// rule sigmoid(stop) >= .5.  Gated as the text form.
__global__ __launch_bounds__(256) void pgen_end_speech_kernel(const float* __restrict__ head, int ld, int M, int B, float* __restrict__ frames, int ld_fr,
                                                              float* __restrict__ stops, int ld_stop, int pos, int64_t* __restrict__ stop_lens,
                                                              int64_t max_len, int* __restrict__ running) {
    const bool run = running[0] != 0;
    __syncthreads();
    if (!run) return;
    for (int i = threadIdx.x; i < B * M; i += 256) {
        const int b = i / M, c = i - b * M;
        frames[(size_t)b * ld_fr + (size_t)(pos + 1) * M + c] = head[(size_t)b * ld + c];
    }
    int open = 0;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float x = head[(size_t)b * ld + M];
        stops[(size_t)b * ld_stop + pos] = x;
        int64_t sl = stop_lens[b];
        if (1.f / (1.f + expf(-x)) >= .5f && sl == max_len) { sl = pos + 1; stop_lens[b] = sl; }
        open |= sl == max_len;
    }
    open = __syncthreads_or(open);
    if (threadIdx.x == 0) running[0] = open ? 1 : 0;
}

}  // namespace

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------
#define PGEN_GEOMETRY(name)                                                                                                          \
    UNAST_REQUIRE(B >= 2 && L >= 1 && (long long)B * L <= (1 << 20), name ": need 2 <= B, 1 <= L, B*L <= 2^20 (B=%d L=%d)", B, L)

extern "C" int unast_prefix_gen_tiles(int B, int L) { return (B * L + PG_ROWS - 1) / PG_ROWS; }

extern "C" int unast_prefix_gen_conv(const float* x, const double* part_in, const float* gamma, const float* beta, float eps, const int64_t* tokens, int ld_tok,
                                     const float* emb, int vocab, int sos, const float* W, const float* bias, float* z, double* part_out, int B, int L, int Cin,
                                     float drop_p, unsigned int seed, unsigned int stream_id, unsigned int row0, hipStream_t stream) {
    UNAST_REQUIRE(W && bias && z && part_out, "unast_prefix_gen_conv: null pointer");
    UNAST_REQUIRE((x != nullptr) != (tokens != nullptr), "unast_prefix_gen_conv: give x (stages 2, 3) or tokens (stage 1), not both");
    PGEN_GEOMETRY("unast_prefix_gen_conv");
    UNAST_REQUIRE(Cin >= 64 && Cin <= PG_MAXCIN && Cin % 64 == 0, "unast_prefix_gen_conv: input channels a multiple of 64, at most %d (got %d)", PG_MAXCIN, Cin);
    UNAST_REQUIRE(((((uintptr_t)W) | ((uintptr_t)z)) & 15) == 0, "unast_prefix_gen_conv: W and z must be 16-byte aligned");
    PGenConv p;
    memset(&p, 0, sizeof(p));
    p.W = W; p.bias = bias; p.z = z; p.part_out = part_out; p.B = B; p.L = L; p.Cin = Cin;
    p.thresh = drop_threshold(drop_p); p.dscale = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f; p.seed = seed; p.stream = stream_id; p.row0 = row0;
    const dim3 grid(unast_prefix_gen_tiles(B, L), PG_C / PG_COLS);
    if (x) {
        UNAST_REQUIRE(part_in && gamma && beta && Cin == PG_C, "unast_prefix_gen_conv: stages 2 and 3 need part_in, gamma, beta and 256 input channels");
        UNAST_REQUIRE(((((uintptr_t)x) | ((uintptr_t)gamma) | ((uintptr_t)beta)) & 15) == 0, "unast_prefix_gen_conv: x, gamma and beta must be 16-byte aligned");
        p.x = x; p.part_in = part_in; p.gamma = gamma; p.beta = beta; p.eps = eps;
        hipLaunchKernelGGL((pgen_conv_kernel<false>), grid, dim3(256), 0, stream, p);
    } else {
        UNAST_REQUIRE(emb && vocab > 0 && sos >= 0 && sos < vocab && ld_tok >= L - 1 && (((uintptr_t)emb) & 15) == 0,
                      "unast_prefix_gen_conv: stage 1 needs a 16-byte aligned emb, sos inside the table and ld_tok >= L - 1");
        p.tokens = tokens; p.ld_tok = ld_tok; p.emb = emb; p.vocab = vocab; p.sos = sos;
        hipLaunchKernelGGL((pgen_conv_kernel<true>), grid, dim3(256), 0, stream, p);
    }
    return unast_check_launch("unast_prefix_gen_conv");
}

extern "C" int unast_prefix_gen_finish(const float* z3, const double* part, const float* gamma, const float* beta, float eps, float* pre, int ldp,
                                       float* rm1, float* rv1, int64_t* nbt1, float mom1, float* rm2, float* rv2, int64_t* nbt2, float mom2,
                                       float* rm3, float* rv3, int64_t* nbt3, float mom3, const int* running, int B, int L, float drop_p, unsigned int seed,
                                       unsigned int stream_id, unsigned int row0, hipStream_t stream) {
    UNAST_REQUIRE(z3 && part && gamma && beta && pre && ldp >= PG_C, "unast_prefix_gen_finish: null pointer or ldp < 256");
    UNAST_REQUIRE((rm1 == nullptr) == (rv1 == nullptr) && (rm2 == nullptr) == (rv2 == nullptr) && (rm3 == nullptr) == (rv3 == nullptr),
                  "unast_prefix_gen_finish: running_mean and running_var together");
    PGEN_GEOMETRY("unast_prefix_gen_finish");
    PGenFinish p;
    memset(&p, 0, sizeof(p));
    p.z3 = z3; p.part = part; p.gamma = gamma; p.beta = beta; p.eps = eps; p.pre = pre; p.ldp = ldp;
    p.rm[0] = rm1; p.rv[0] = rv1; p.nbt[0] = (long long*)nbt1; p.mom[0] = mom1;
    p.rm[1] = rm2; p.rv[1] = rv2; p.nbt[1] = (long long*)nbt2; p.mom[1] = mom2;
    p.rm[2] = rm3; p.rv[2] = rv3; p.nbt[2] = (long long*)nbt3; p.mom[2] = mom3;
    p.running = running; p.B = B; p.L = L; p.ntiles = unast_prefix_gen_tiles(B, L);
    p.thresh = drop_threshold(drop_p); p.dscale = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f; p.seed = seed; p.stream = stream_id; p.row0 = row0;
    hipLaunchKernelGGL(pgen_finish_kernel, dim3(3), dim3(256), 0, stream, p);
    return unast_check_launch("unast_prefix_gen_finish");
}

extern "C" int unast_prefix_gen_act_drop(const float* x, int ldx, float* out, int ldo, int B, int C, int act, float drop_a, unsigned int stream_a, float drop_b,
                                         unsigned int stream_b, unsigned int seed, unsigned int row0, hipStream_t stream) {
    UNAST_REQUIRE(x && out && B > 0 && C > 0 && ldx >= C && ldo >= C && act >= 0 && act <= 2 && (long long)B * C <= 0x7FFFFFFF, "unast_prefix_gen_act_drop: bad arguments");
    hipLaunchKernelGGL(pgen_act_drop_kernel, dim3((B * C + 255) / 256), dim3(256), 0, stream, x, ldx, out, ldo, B, C, act, drop_threshold(drop_a),
                       drop_a > 0.f ? 1.f / (1.f - drop_a) : 1.f, stream_a, drop_threshold(drop_b), drop_b > 0.f ? 1.f / (1.f - drop_b) : 1.f, stream_b, seed, row0);
    return unast_check_launch("unast_prefix_gen_act_drop");
}

extern "C" int unast_prefix_gen_end_text(const float* logits, int ld, int V, int B, int64_t* tokens, int ld_tok, int pos, int64_t* stop_lens, int64_t max_len,
                                         int eos, int* running, hipStream_t stream) {
    UNAST_REQUIRE(logits && tokens && stop_lens && running && B > 0 && V > 0 && ld >= V && pos >= 0 && pos < max_len && ld_tok >= max_len,
                  "unast_prefix_gen_end_text: bad arguments (0 <= pos < max_len <= ld_tok)");
    hipLaunchKernelGGL(pgen_end_text_kernel, dim3(1), dim3(256), 0, stream, logits, ld, V, B, tokens, ld_tok, pos, stop_lens, max_len, eos, running);
    return unast_check_launch("unast_prefix_gen_end_text");
}

extern "C" int unast_prefix_gen_end_speech(const float* head, int ld, int M, int B, float* frames, int ld_fr, float* stops, int ld_stop, int pos,
                                           int64_t* stop_lens, int64_t max_len, int* running, hipStream_t stream) {
    UNAST_REQUIRE(head && frames && stops && stop_lens && running && B > 0 && M > 0 && ld > M && pos >= 0 && pos < max_len && ld_fr >= (max_len + 1) * M &&
                      ld_stop >= max_len,
                  "unast_prefix_gen_end_speech: bad arguments (0 <= pos < max_len, frames rows of (max_len + 1) * M, stops rows of max_len)");
    hipLaunchKernelGGL(pgen_end_speech_kernel, dim3(1), dim3(256), 0, stream, head, ld, M, B, frames, ld_fr, stops, ld_stop, pos, stop_lens, max_len, running);
    return unast_check_launch("unast_prefix_gen_end_speech");
}

UNAST_DEFINE_RNG_EPOCH_SETTER(prefix_gen)
