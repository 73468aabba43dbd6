// Waveform synthesis from a magnitude spectrogram (src/utils.py:281-328: spectrogram2wav, griffin_lim, invert_spectrogram): the short-time
// Fourier transform and its inverse at librosa's settings (centred frames, reflect padding, a periodic Hann window of win samples centred in
// n_fft, overlap-add divided by the window's sum of squares), the Griffin-Lim phase update, the de-normalisation, the de-preemphasis
// recurrence and the bounds of librosa.effects.trim.  DESIGN.md section 5q states the definitions these kernels are held to.
// Feature extraction, the other direction (src/utils.py:235-278, get_spectrograms): the preemphasis, the transform over an arbitrary sample
// count and, in its epilogue, |S|, the mel projection, dB, normalise and clip.
//
// The transform is a Stockham autosort FFT in LDS, written here: one workgroup of 256 threads per frame, the frame as n_fft complex points
// (2048 x 8 bytes = 16 KB per buffer, two buffers), radix-4 passes and one closing radix-2 pass where log2(n_fft) is odd
// (2048 = 4^5 x 2).  Real and imaginary parts live in separate float arrays whose index i is stored at i + i / 32: the radix-4 pass with
// sub-transform length Ns writes with a lane stride of 4 floats at Ns = 1, which without the pad is a 4-way conflict on the 32 banks of
// ds_write_b32 and with it none (lanes 8 apart land one bank further); the reads of every pass are unit-stride.  Twiddles come from a
// table exp(-2 pi i m / n_fft) that the host computes in float64 (unast_amd/audio.py); no sine or cosine is evaluated on the device.
// Every sum is formed in a fixed order by one thread or one workgroup, so results are the same bits on every run and do not depend
// on which batch an utterance is in; frames at or behind frames[b] and samples behind an utterance's length are neither read nor written.
#include "common.h"
#include "../../include/unast_hip.h"
#include <float.h>

namespace {

constexpr int FFT_THREADS = 256;
constexpr int FFT_MAX = 2048;
constexpr int FFT_LEN = FFT_MAX + FFT_MAX / 32;      // padded length of one float array
constexpr int DEEMPH_THREADS = 256;
constexpr int DEEMPH_CHUNK = 16;                      // consecutive samples per thread
constexpr int DEEMPH_TILE = DEEMPH_THREADS * DEEMPH_CHUNK;
constexpr int TRIM_THREADS = 256;

__device__ __forceinline__ int padi(int i) { return i + (i >> 5); }

struct FftLds {
    float re[2][FFT_LEN];
    float im[2][FFT_LEN];
};

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    return make_float2(__builtin_fmaf(a.x, b.x, -a.y * b.y), __builtin_fmaf(a.x, b.y, a.y * b.x));
}

// In-place (ping-pong) transform of the N points in buffer 0; returns the buffer that holds the result in natural order.  INV: the
// conjugate transform without the 1/N factor.  Pass with sub-transform length Ns, radix R: butterfly j takes the points j + r N/R,
// multiplies point r by w^(r k), k = j mod Ns, w = exp(-+2 pi i / (Ns R)), and writes output r to (j - k) R + k + r Ns.
template <bool INV>
__device__ int fft_lds(FftLds& s, const float2* __restrict__ tw, int N) {
    const int tid = threadIdx.x;
    int cur = 0, Ns = 1;
    const int q = N >> 2;
    for (; Ns * 4 <= N; Ns <<= 2) {
        const float* sr = s.re[cur];
        const float* si = s.im[cur];
        float* dr = s.re[cur ^ 1];
        float* di = s.im[cur ^ 1];
        const int tstride = N / (Ns * 4);
        for (int j = tid; j < q; j += FFT_THREADS) {
            const int k = j & (Ns - 1);
            float2 v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = padi(j + r * q);
                v[r] = make_float2(sr[p], si[p]);
            }
            if (Ns > 1) {
#pragma unroll
                for (int r = 1; r < 4; ++r) {
                    float2 t = tw[r * k * tstride];          // r k tstride < N
                    if (INV) t.y = -t.y;
                    v[r] = cmul(v[r], t);
                }
            }
            const float2 a0 = make_float2(v[0].x + v[2].x, v[0].y + v[2].y);
            const float2 a1 = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
            const float2 a2 = make_float2(v[1].x + v[3].x, v[1].y + v[3].y);
            const float2 d = make_float2(v[1].x - v[3].x, v[1].y - v[3].y);
            const float2 a3 = INV ? make_float2(-d.y, d.x) : make_float2(d.y, -d.x);      // (v1 - v3) times +i / -i
            const int o = ((j - k) << 2) + k;
            int p = padi(o);
            dr[p] = a0.x + a2.x; di[p] = a0.y + a2.y;
            p = padi(o + Ns);
            dr[p] = a1.x + a3.x; di[p] = a1.y + a3.y;
            p = padi(o + 2 * Ns);
            dr[p] = a0.x - a2.x; di[p] = a0.y - a2.y;
            p = padi(o + 3 * Ns);
            dr[p] = a1.x - a3.x; di[p] = a1.y - a3.y;
        }
        __syncthreads();
        cur ^= 1;
    }
    if (Ns < N) {                                             // Ns == N / 2: the closing radix-2 pass, k = j
        const float* sr = s.re[cur];
        const float* si = s.im[cur];
        float* dr = s.re[cur ^ 1];
        float* di = s.im[cur ^ 1];
        const int h = N >> 1;
        for (int j = tid; j < h; j += FFT_THREADS) {
            const int p0 = padi(j), p1 = padi(j + h);
            const float2 v0 = make_float2(sr[p0], si[p0]);
            float2 t = tw[j];
            if (INV) t.y = -t.y;
            const float2 v1 = cmul(make_float2(sr[p1], si[p1]), t);
            dr[p0] = v0.x + v1.x; di[p0] = v0.y + v1.y;
            dr[p1] = v0.x - v1.x; di[p1] = v0.y - v1.y;
        }
        __syncthreads();
        cur ^= 1;
    }
    return cur;
}

// S[b,t,:] = rfft(wp * yp[t hop : t hop + N]); with mag: mag * S / max(1e-8, |S|) (the Griffin-Lim update, src/utils.py:314-316).
// The reflect padding is index arithmetic: sample p of the padded signal is y[|p - N/2|] on the left and y[2 (n - 1) - (p - N/2)] on the
// right; n > N / 2 (checked by the caller through min_frames) makes one reflection enough.  Samples outside the window are zero and not loaded.
// MOMENTUM: the fast Griffin-Lim update of librosa.griffinlim in the same epilogue: with e = S, c = e - alpha tprev,
// the thread that owns bin k reads tprev[k], stores tprev[k] <- e and spec[k] <- mag c / (|c| + 1e-16).  alpha == 0 is the first iteration
// (tprev = 0 by definition) and plain Griffin-Lim: tprev is then not read, so it may be fresh memory.
template <bool MOMENTUM>
__global__ __launch_bounds__(FFT_THREADS) void stft_kernel(const float* __restrict__ y, long long ld_y, const int* __restrict__ frames, int T_max, int N,
                                                           int hop, int win, int min_frames, const float* __restrict__ window,
                                                           const float2* __restrict__ tw, const float* __restrict__ mag, float alpha,
                                                           float2* tprev, float2* __restrict__ spec) {
    __shared__ FftLds s;
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int f = min(frames[b], T_max);
    if (t >= f || f < min_frames) return;                     // uniform over the workgroup
    const int n = hop * (f - 1), lpad = (N - win) >> 1, half = N >> 1;
    const float* yb = y + (size_t)b * ld_y;
    for (int m = tid; m < N; m += FFT_THREADS) {
        const int j = m - lpad;
        float v = 0.f;
        if (j >= 0 && j < win) {
            int p = t * hop + m - half;
            if (p < 0) p = -p;
            if (p >= n) p = 2 * (n - 1) - p;
            p = max(0, min(p, n - 1));
            v = window[j] * yb[p];
        }
        const int pi = padi(m);
        s.re[0][pi] = v;
        s.im[0][pi] = 0.f;
    }
    __syncthreads();
    const int cur = fft_lds<false>(s, tw, N);
    const int F = half + 1;
    const size_t row = ((size_t)b * T_max + t) * F;
    for (int k = tid; k < F; k += FFT_THREADS) {
        const int pi = padi(k);
        float re = s.re[cur][pi], im = s.im[cur][pi];
        if (MOMENTUM) {
            const float2 e = make_float2(re, im);
            if (alpha != 0.f) {
                const float2 tp = tprev[row + k];
                re = __builtin_fmaf(-alpha, tp.x, re);
                im = __builtin_fmaf(-alpha, tp.y, im);
            }
            tprev[row + k] = e;
            const float a = sqrtf(__builtin_fmaf(re, re, im * im)) + 1e-16f;
            const float g = mag[row + k];
            re = g * re / a;
            im = g * im / a;
        } else if (mag) {
            const float a = fmaxf(1e-8f, sqrtf(__builtin_fmaf(re, re, im * im)));
            const float g = mag[row + k];
            re = g * re / a;
            im = g * im / a;
        }
        spec[row + k] = make_float2(re, im);
    }
}

// fr[b,t,j] = w[j] * irfft(S[b,t,:], N)[lpad + j], j < win (src/utils.py:323-328 before the overlap-add): Hermitian extension with the
// imaginary parts of the DC and Nyquist bins dropped, the conjugate transform, 1/N, the window.  Outside the window the frame is zero.
__global__ __launch_bounds__(FFT_THREADS) void istft_frames_kernel(const float2* __restrict__ spec, const int* __restrict__ frames, int T_max, int N, int win,
                                                                   const float* __restrict__ window, const float2* __restrict__ tw, float* __restrict__ fr) {
    __shared__ FftLds s;
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    if (t >= min(frames[b], T_max)) return;
    const int half = N >> 1, F = half + 1, lpad = (N - win) >> 1;
    const size_t fi = (size_t)b * T_max + t;
    const float2* sp = spec + fi * F;
    for (int m = tid; m < N; m += FFT_THREADS) {
        const int k = m <= half ? m : N - m;
        float2 v = sp[k];
        if (m > half) v.y = -v.y;
        if (k == 0 || k == half) v.y = 0.f;
        const int pi = padi(m);
        s.re[0][pi] = v.x;
        s.im[0][pi] = v.y;
    }
    __syncthreads();
    const int cur = fft_lds<true>(s, tw, N);
    const float inv_n = 1.f / (float)N;                       // a power of two: exact
    float* out = fr + fi * win;
    for (int j = tid; j < win; j += FFT_THREADS) out[j] = window[j] * (s.re[cur][padi(lpad + j)] * inv_n);
}

// y[b,m] = sum_t fr[b,t,m + N/2 - lpad - t hop] / sum_t w[.]^2 over the frames t < frames[b] that cover the sample, in ascending t.
__global__ __launch_bounds__(256) void overlap_add_kernel(const float* __restrict__ fr, const int* __restrict__ frames, int T_max, int N, int hop, int win,
                                                          const float* __restrict__ window, float* __restrict__ y, long long ld_y) {
    const int b = blockIdx.y;
    const int f = min(frames[b], T_max);
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f < 1 || m >= (long long)hop * (f - 1)) return;
    const int a = (int)m + (N >> 1) - ((N - win) >> 1);       // offset into frame 0's window; >= 0
    const int t_hi = min(a / hop, f - 1);
    const int t_lo = a - win + 1 <= 0 ? 0 : (a - win + hop) / hop;
    const float* fb = fr + (size_t)b * T_max * win;
    float num = 0.f, den = 0.f;
    for (int t = t_lo; t <= t_hi; ++t) {
        const int j = a - t * hop;
        const float w = window[j];
        num += fb[(size_t)t * win + j];
        den = __builtin_fmaf(w, w, den);
    }
    y[(size_t)b * ld_y + m] = den > FLT_MIN ? num / den : num;
}

// M = (10 ^ (0.05 (clip(mag, 0, 1) max_db - max_db + ref_db))) ^ power (src/utils.py:292-298), in double and rounded once; X0 = (M, 0).
__global__ __launch_bounds__(256) void gl_prepare_kernel(const float* __restrict__ mag, long long ld_mag, long long rows, int F, double max_db, double ref_db,
                                                         double power, float* __restrict__ M, float2* __restrict__ X0) {
    const long long total = rows * F;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / F;
        const int c = (int)(i - r * F);
        const double x = fmin(fmax((double)mag[r * ld_mag + c], 0.0), 1.0);
        const float v = (float)pow(pow(10.0, 0.05 * (x * max_db - max_db + ref_db)), power);
        M[i] = v;
        if (X0) X0[i] = make_float2(v, 0.f);
    }
}

// The phase index of librosa.griffinlim's random start: a counter-based draw from (seed, key, frame, bin), each
// argument entering under a pcg_hash of its own; tests/fast_griffin_lim_mirror.py restates it in numpy.
__device__ __forceinline__ uint32_t gl_phase_hash(uint32_t seed, uint32_t key, uint32_t t, uint32_t k) {
    return pcg_hash(k + pcg_hash(t + pcg_hash(key + pcg_hash(seed))));
}

// X0[b,t,k] = M[b,t,k] tw[m], m = gl_phase_hash(seed, keys[b], t, k) & (N - 1): a phase uniform over the N levels of the twiddle table.
__global__ __launch_bounds__(256) void gl_random_phase_kernel(const float* __restrict__ M, const int* __restrict__ frames, const uint32_t* __restrict__ keys,
                                                              uint32_t seed, int T_max, int N, const float2* __restrict__ tw, float2* __restrict__ X0) {
    const int b = blockIdx.y, F = (N >> 1) + 1;
    const int f = min(frames[b], T_max);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)f * F) return;
    const int t = (int)(i / F), k = (int)(i - (long long)t * F);
    const float2 w = tw[gl_phase_hash(seed, keys[b], (uint32_t)t, (uint32_t)k) & (uint32_t)(N - 1)];
    const size_t o = (size_t)b * T_max * F + (size_t)i;
    const float g = M[o];
    X0[o] = make_float2(g * w.x, g * w.y);
}

// y[k] = x[k] + c y[k-1] (scipy.signal.lfilter([1], [1, -c]), src/utils.py:301) as a blocked scan: one workgroup per utterance walks it in
// tiles of 256 x 16 samples; a thread runs the recurrence over its 16 samples from a zero state, the chunk ends are combined across the
// tile by a scan of the affine maps s -> c^16 s + e (exact in structure: every earlier sample reaches every later one), and each sample
// then adds c^(i+1) times the state entering its chunk.
__global__ __launch_bounds__(DEEMPH_THREADS) void deemphasis_kernel(const float* x, long long ld_x, float* y, long long ld_y, const int* __restrict__ lens, float c) {
    __shared__ float s_a[2][DEEMPH_THREADS], s_e[2][DEEMPH_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = lens[b];
    const float* xb = x + (size_t)b * ld_x;
    float* yb = y + (size_t)b * ld_y;
    float cp[DEEMPH_CHUNK + 1];
    cp[0] = 1.f;
#pragma unroll
    for (int i = 1; i <= DEEMPH_CHUNK; ++i) cp[i] = cp[i - 1] * c;
    float carry = 0.f;                                        // the state entering the tile (y of the sample before it)
    for (int base = 0; base < n; base += DEEMPH_TILE) {
        const int k0 = base + tid * DEEMPH_CHUNK;
        float v[DEEMPH_CHUNK];
        float st = 0.f;
#pragma unroll
        for (int i = 0; i < DEEMPH_CHUNK; ++i) {
            const float xv = k0 + i < n ? xb[k0 + i] : 0.f;
            st = __builtin_fmaf(c, st, xv);
            v[i] = st;
        }
        // inclusive scan over the threads of (A, E): state after chunk = A * state before + E
        int cur = 0;
        s_a[0][tid] = cp[DEEMPH_CHUNK];
        s_e[0][tid] = st;
        __syncthreads();
        for (int off = 1; off < DEEMPH_THREADS; off <<= 1) {
            float a = s_a[cur][tid], e = s_e[cur][tid];
            if (tid >= off) {
                const float ap = s_a[cur][tid - off], ep = s_e[cur][tid - off];
                e = __builtin_fmaf(a, ep, e);
                a = a * ap;
            }
            s_a[cur ^ 1][tid] = a;
            s_e[cur ^ 1][tid] = e;
            __syncthreads();
            cur ^= 1;
        }
        // the state entering this thread's chunk: the scan of the threads before it applied to the tile's carry
        const float in = tid == 0 ? carry : __builtin_fmaf(s_a[cur][tid - 1], carry, s_e[cur][tid - 1]);
        const float next = __builtin_fmaf(s_a[cur][DEEMPH_THREADS - 1], carry, s_e[cur][DEEMPH_THREADS - 1]);
#pragma unroll
        for (int i = 0; i < DEEMPH_CHUNK; ++i)
            if (k0 + i < n) yb[k0 + i] = __builtin_fmaf(cp[i + 1], in, v[i]);
        carry = next;
        __syncthreads();                                      // the scan buffers are rewritten by the next tile
    }
}

// Sample i of the signal padded by `pad` on both sides: reflect (numpy's 'reflect', any pad length) or zeros.
__device__ __forceinline__ float padded_sample(const float* yb, int n, int i, int pad, int reflect) {
    int p = i - pad;
    if (p >= 0 && p < n) return yb[p];
    if (!reflect) return 0.f;
    if (n == 1) return yb[0];
    const int period = 2 * (n - 1);
    p %= period;
    if (p < 0) p += period;
    if (p >= n) p = period - p;
    return yb[p];
}

// ws[b,i] = mean square of frame i (frame_length samples at i hop_length of the padded signal), i < 1 + n / hop_length.
__global__ __launch_bounds__(TRIM_THREADS) void trim_power_kernel(const float* __restrict__ y, long long ld_y, const int* __restrict__ lens, int nf_max,
                                                                  int frame_length, int hop_length, int reflect, float* __restrict__ ws) {
    __shared__ float red[TRIM_THREADS / UNAST_WAVE];
    const int b = blockIdx.y, i = blockIdx.x, tid = threadIdx.x;
    const int n = lens[b];
    if (n < 1 || i >= 1 + n / hop_length) return;
    const float* yb = y + (size_t)b * ld_y;
    float acc = 0.f;
    for (int k = tid; k < frame_length; k += TRIM_THREADS) {
        const float v = padded_sample(yb, n, i * hop_length + k, frame_length >> 1, reflect);
        acc = __builtin_fmaf(v, v, acc);
    }
    acc = wave_sum(acc);
    if ((tid & (UNAST_WAVE - 1)) == 0) red[tid / UNAST_WAVE] = acc;
    __syncthreads();
    if (tid == 0) {
        float tot = 0.f;
        for (int w = 0; w < TRIM_THREADS / UNAST_WAVE; ++w) tot += red[w];
        ws[(size_t)b * nf_max + i] = tot / (float)frame_length;
    }
}

// out[b] = {start, end} of librosa.effects.trim: frames within top_db of the loudest one are non-silent.
__global__ __launch_bounds__(TRIM_THREADS) void trim_bounds_kernel(const float* __restrict__ ws, const int* __restrict__ lens, int nf_max, int hop_length,
                                                                   float top_db, int* __restrict__ out) {
    __shared__ float s_max[TRIM_THREADS];
    __shared__ int s_first[TRIM_THREADS], s_last[TRIM_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = lens[b];
    const int nf = n < 1 ? 0 : 1 + n / hop_length;
    const float* p = ws + (size_t)b * nf_max;
    float mx = 0.f;
    for (int i = tid; i < nf; i += TRIM_THREADS) mx = fmaxf(mx, p[i]);
    s_max[tid] = mx;
    __syncthreads();
    for (int off = TRIM_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) s_max[tid] = fmaxf(s_max[tid], s_max[tid + off]);
        __syncthreads();
    }
    const float ref_db = 10.f * log10f(fmaxf(1e-10f, s_max[0]));
    int first = nf, last = -1;
    for (int i = tid; i < nf; i += TRIM_THREADS) {
        if (10.f * log10f(fmaxf(1e-10f, p[i])) - ref_db > -top_db) {
            first = min(first, i);
            last = max(last, i);
        }
    }
    s_first[tid] = first;
    s_last[tid] = last;
    __syncthreads();
    for (int off = TRIM_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) {
            s_first[tid] = min(s_first[tid], s_first[tid + off]);
            s_last[tid] = max(s_last[tid], s_last[tid + off]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        const bool any = s_last[0] >= 0;
        out[2 * b] = any ? s_first[0] * hop_length : 0;
        out[2 * b + 1] = any ? (int)min((long long)n, (long long)(s_last[0] + 1) * hop_length) : 0;
    }
}

// e[0] = y[0], e[k] = y[k] - c y[k-1] (src/utils.py:251) as numpy forms it on a float32 array: one rounded multiply, one rounded subtract,
// never an FMA (hipcc contracts a * b - c by default, through __fmul_rn / __fsub_rn as well, so contraction is switched off for this
// function's arithmetic).  yb points at the utterance's first sample, k >= 0.
__device__ __forceinline__ float emphasised(const float* __restrict__ yb, int k, float c) {
#pragma clang fp contract(off)
    const float v = yb[k];
    if (k == 0) return v;
    const float prod = c * yb[k - 1];
    return v - prod;
}

// clip((20 log10(max(1e-5, x)) - ref_db + max_db) / max_db, 1e-8, 1) (src/utils.py:267-272)
__device__ __forceinline__ float normalised_db(float x, float ref_db, float max_db) {
    const float v = (20.f * log10f(fmaxf(1e-5f, x)) - ref_db + max_db) / max_db;
    return fminf(fmaxf(v, 1e-8f), 1.f);
}

// get_spectrograms (src/utils.py:251-276) for frame t of utterance b, the samples[b] samples of row b from start[b] on: the windowed frame of
// the emphasised signal (reflect padding by index arithmetic about samples 0 and n - 1; index 0 keeps its raw value), the transform, and in
// its epilogue |S| into the LDS buffer the transform has finished with, the normalised magnitude row, and -- after a barrier -- the mel
// values, one thread per filter summing W[i,k] |S[k]| over the filter's [lo, hi) in ascending k, normalised the same way.  An utterance that
// is not longer than the padding, or does not lie inside its row, is skipped; so are frames at or behind 1 + n / hop.
__global__ __launch_bounds__(FFT_THREADS) void features_kernel(const float* __restrict__ y, long long ld_y, int n_max, const int* __restrict__ start,
                                                               const int* __restrict__ samples, int T_max, int N, int hop, int win, float coef,
                                                               const float* __restrict__ window, const float2* __restrict__ tw,
                                                               const float* __restrict__ basis, const int* __restrict__ ranges, int n_mels, float ref_db,
                                                               float max_db, float* __restrict__ mel, float* __restrict__ magn, float2* __restrict__ spec) {
    __shared__ FftLds s;
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int n = samples[b], st = start ? start[b] : 0, half = N >> 1;
    if (n <= half || st < 0 || n > n_max - st || t >= 1 + n / hop) return;      // uniform over the workgroup
    const int lpad = (N - win) >> 1;
    const float* yb = y + (size_t)b * ld_y + st;
    for (int m = tid; m < N; m += FFT_THREADS) {
        const int j = m - lpad;
        float v = 0.f;
        if (j >= 0 && j < win) {
            int p = t * hop + m - half;
            if (p < 0) p = -p;
            if (p >= n) p = 2 * (n - 1) - p;
            p = max(0, min(p, n - 1));
            v = window[j] * emphasised(yb, p, coef);
        }
        const int pi = padi(m);
        s.re[0][pi] = v;
        s.im[0][pi] = 0.f;
    }
    __syncthreads();
    const int cur = fft_lds<false>(s, tw, N);
    const int F = half + 1;
    const size_t fi = (size_t)b * T_max + t;
    float* absS = s.re[cur ^ 1];                              // the last pass read it; a barrier has passed since
    for (int k = tid; k < F; k += FFT_THREADS) {
        const int pi = padi(k);
        const float re = s.re[cur][pi], im = s.im[cur][pi];
        const float a = sqrtf(__builtin_fmaf(re, re, im * im));
        absS[pi] = a;
        magn[fi * F + k] = normalised_db(a, ref_db, max_db);
        if (spec) spec[fi * F + k] = make_float2(re, im);
    }
    __syncthreads();
    for (int i = tid; i < n_mels; i += FFT_THREADS) {
        const int lo = max(0, ranges[2 * i]), hi = min(F, ranges[2 * i + 1]);
        const float* w = basis + (size_t)i * F;
        float acc = 0.f;
        for (int k = lo; k < hi; ++k) acc = __builtin_fmaf(w[k], absS[padi(k)], acc);
        mel[fi * n_mels + i] = normalised_db(acc, ref_db, max_db);
    }
}

// out[b, start[b] + k] = the emphasised sample k of the utterance x[b, start[b] : start[b] + lens[b]]; nothing else is read or written.
__global__ __launch_bounds__(256) void preemphasis_kernel(const float* __restrict__ x, long long ld_x, float* __restrict__ out, long long ld_out, int n_max,
                                                          const int* __restrict__ start, const int* __restrict__ lens, float coef) {
    const int b = blockIdx.y;
    const int n = lens[b], st = start ? start[b] : 0;
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n < 1 || st < 0 || n > n_max - st || k >= n) return;
    out[(size_t)b * ld_out + st + k] = emphasised(x + (size_t)b * ld_x + st, (int)k, coef);
}

int check_stft_params(const char* who, int B, int T_max, int n_fft, int hop, int win) {
    UNAST_REQUIRE(B >= 1 && B <= 65535 && T_max >= 1, "%s: need 1 <= B <= 65535 and T_max >= 1 (B=%d T_max=%d)", who, B, T_max);
    UNAST_REQUIRE(n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048, "%s: n_fft must be 256, 512, 1024 or 2048 (got %d)", who, n_fft);
    UNAST_REQUIRE(win >= 1 && win <= n_fft, "%s: need 1 <= win <= n_fft (win=%d n_fft=%d)", who, win, n_fft);
    UNAST_REQUIRE(hop >= 1 && (long long)hop * T_max < (1ll << 30), "%s: need hop >= 1 and hop * T_max < 2^30 (hop=%d T_max=%d)", who, hop, T_max);
    return UNAST_OK;
}

// What unast_stft and unast_stft_momentum refuse alike; *min_frames: the shortest utterance the kernel transforms.
int check_stft_call(const char* who, const float* y, int64_t ld_y, const int* frames, int B, int T_max, int n_fft, int hop, int win,
                    const float* window, const float* twiddle, const float* spec, int* min_frames) {
    if (int rc = check_stft_params(who, B, T_max, n_fft, hop, win)) return rc;
    UNAST_REQUIRE(y && frames && window && twiddle && spec, "%s: null pointer", who);
    *min_frames = n_fft / (2 * hop) + 2;
    UNAST_REQUIRE(T_max >= *min_frames, "%s: an utterance needs at least n_fft / (2 hop) + 2 = %d frames: the signal must be longer than the reflect padding (T_max=%d)",
                  who, *min_frames, T_max);
    UNAST_REQUIRE(ld_y >= (int64_t)hop * (T_max - 1), "%s: the row stride %lld is below hop * (T_max - 1) = %lld samples", who, (long long)ld_y, (long long)hop * (T_max - 1));
    UNAST_REQUIRE((((uintptr_t)twiddle) & 7) == 0 && (((uintptr_t)spec) & 7) == 0, "%s: twiddle and spec hold complex values and need 8-byte alignment", who);
    return UNAST_OK;
}

}  // namespace

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------
extern "C" int unast_stft(const float* y, int64_t ld_y, const int* frames, int B, int T_max, int n_fft, int hop, int win, const float* window,
                          const float* twiddle, const float* mag, float* spec, hipStream_t stream) {
    int min_frames = 0;
    if (int rc = check_stft_call("unast_stft", y, ld_y, frames, B, T_max, n_fft, hop, win, window, twiddle, spec, &min_frames)) return rc;
    hipLaunchKernelGGL(stft_kernel<false>, dim3(T_max, B), dim3(FFT_THREADS), 0, stream, y, (long long)ld_y, frames, T_max, n_fft, hop, win, min_frames, window,
                       (const float2*)twiddle, mag, 0.f, (float2*)nullptr, (float2*)spec);
    return unast_check_launch("unast_stft");
}

extern "C" int unast_stft_momentum(const float* y, int64_t ld_y, const int* frames, int B, int T_max, int n_fft, int hop, int win, const float* window,
                                   const float* twiddle, const float* mag, float alpha, float* tprev, float* spec, hipStream_t stream) {
    int min_frames = 0;
    if (int rc = check_stft_call("unast_stft_momentum", y, ld_y, frames, B, T_max, n_fft, hop, win, window, twiddle, spec, &min_frames)) return rc;
    UNAST_REQUIRE(mag && tprev, "unast_stft_momentum: null pointer (mag and tprev are needed)");
    UNAST_REQUIRE(alpha >= 0.f && alpha < 0.5f, "unast_stft_momentum: alpha = momentum / (1 + momentum) must lie in [0, 0.5) (got %g)", (double)alpha);
    UNAST_REQUIRE((((uintptr_t)tprev) & 7) == 0 && tprev != spec, "unast_stft_momentum: tprev holds complex values, needs 8-byte alignment and is not spec");
    hipLaunchKernelGGL(stft_kernel<true>, dim3(T_max, B), dim3(FFT_THREADS), 0, stream, y, (long long)ld_y, frames, T_max, n_fft, hop, win, min_frames, window,
                       (const float2*)twiddle, mag, alpha, (float2*)tprev, (float2*)spec);
    return unast_check_launch("unast_stft_momentum");
}

extern "C" int unast_gl_random_phase(const float* M, const int* frames, const unsigned int* keys, unsigned int seed, int B, int T_max, int n_fft,
                                     const float* twiddle, float* X0, hipStream_t stream) {
    if (int rc = check_stft_params("unast_gl_random_phase", B, T_max, n_fft, 1, n_fft)) return rc;
    UNAST_REQUIRE(M && frames && keys && twiddle && X0, "unast_gl_random_phase: null pointer");
    UNAST_REQUIRE((((uintptr_t)twiddle) & 7) == 0 && (((uintptr_t)X0) & 7) == 0, "unast_gl_random_phase: twiddle and X0 hold complex values and need 8-byte alignment");
    const long long per = (long long)T_max * (n_fft / 2 + 1);
    UNAST_REQUIRE(per < (1ll << 31), "unast_gl_random_phase: T_max * (1 + n_fft / 2) must stay below 2^31 (T_max=%d)", T_max);
    hipLaunchKernelGGL(gl_random_phase_kernel, dim3((unsigned)((per + 255) / 256), B), dim3(256), 0, stream, M, frames, (const uint32_t*)keys, (uint32_t)seed, T_max,
                       n_fft, (const float2*)twiddle, (float2*)X0);
    return unast_check_launch("unast_gl_random_phase");
}

extern "C" int unast_istft_frames(const float* spec, const int* frames, int B, int T_max, int n_fft, int win, const float* window, const float* twiddle,
                                  float* fr, hipStream_t stream) {
    if (int rc = check_stft_params("unast_istft_frames", B, T_max, n_fft, 1, win)) return rc;
    UNAST_REQUIRE(spec && frames && window && twiddle && fr, "unast_istft_frames: null pointer");
    UNAST_REQUIRE((((uintptr_t)twiddle) & 7) == 0 && (((uintptr_t)spec) & 7) == 0, "unast_istft_frames: twiddle and spec hold complex values and need 8-byte alignment");
    hipLaunchKernelGGL(istft_frames_kernel, dim3(T_max, B), dim3(FFT_THREADS), 0, stream, (const float2*)spec, frames, T_max, n_fft, win, window,
                       (const float2*)twiddle, fr);
    return unast_check_launch("unast_istft_frames");
}

extern "C" int unast_overlap_add(const float* fr, const int* frames, int B, int T_max, int n_fft, int hop, int win, const float* window, float* y,
                                 int64_t ld_y, hipStream_t stream) {
    if (int rc = check_stft_params("unast_overlap_add", B, T_max, n_fft, hop, win)) return rc;
    UNAST_REQUIRE(fr && frames && window && y, "unast_overlap_add: null pointer");
    UNAST_REQUIRE(ld_y >= (int64_t)hop * (T_max - 1), "unast_overlap_add: the row stride %lld is below hop * (T_max - 1) = %lld samples", (long long)ld_y,
                  (long long)hop * (T_max - 1));
    const long long n_max = (long long)hop * (T_max - 1);
    if (n_max == 0) return UNAST_OK;
    hipLaunchKernelGGL(overlap_add_kernel, dim3((unsigned)((n_max + 255) / 256), B), dim3(256), 0, stream, fr, frames, T_max, n_fft, hop, win, window, y, (long long)ld_y);
    return unast_check_launch("unast_overlap_add");
}

extern "C" int unast_gl_prepare(const float* mag, int64_t ld_mag, int64_t rows, int F, double max_db, double ref_db, double power, float* M, float* X0,
                                hipStream_t stream) {
    UNAST_REQUIRE(mag && M, "unast_gl_prepare: null pointer");
    UNAST_REQUIRE(rows >= 1 && F >= 1 && ld_mag >= F && rows * (int64_t)F < (1ll << 40), "unast_gl_prepare: need rows >= 1, F >= 1, ld_mag >= F (rows=%lld F=%d ld=%lld)",
                  (long long)rows, F, (long long)ld_mag);
    UNAST_REQUIRE((((uintptr_t)X0) & 7) == 0, "unast_gl_prepare: X0 holds complex values and needs 8-byte alignment");
    const long long total = rows * (long long)F;
    const long long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(gl_prepare_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, stream, mag, (long long)ld_mag, (long long)rows, F,
                       max_db, ref_db, power, M, (float2*)X0);
    return unast_check_launch("unast_gl_prepare");
}

extern "C" int unast_deemphasis(const float* x, int64_t ld_x, float* y, int64_t ld_y, const int* lens, int B, float coef, hipStream_t stream) {
    UNAST_REQUIRE(x && y && lens && B >= 1, "unast_deemphasis: need x, y, lens and B >= 1 (B=%d)", B);
    UNAST_REQUIRE(ld_x >= 0 && ld_y >= 0 && coef > -1.f && coef < 1.f, "unast_deemphasis: need non-negative row strides and |coef| < 1 (coef=%g)", (double)coef);
    hipLaunchKernelGGL(deemphasis_kernel, dim3(B), dim3(DEEMPH_THREADS), 0, stream, x, (long long)ld_x, y, (long long)ld_y, lens, coef);
    return unast_check_launch("unast_deemphasis");
}

extern "C" int unast_trim_bounds(const float* y, int64_t ld_y, const int* lens, int B, int n_max, float top_db, int frame_length, int hop_length, int pad_mode,
                                 float* ws, int64_t ws_floats, int* out, hipStream_t stream) {
    UNAST_REQUIRE(y && lens && out && B >= 1 && B <= 65535 && n_max >= 1, "unast_trim_bounds: need y, lens, out, 1 <= B <= 65535 and n_max >= 1 (B=%d n_max=%d)", B, n_max);
    UNAST_REQUIRE(frame_length >= 2 && hop_length >= 1 && ld_y >= n_max && n_max < (1 << 30), "unast_trim_bounds: need frame_length >= 2, hop_length >= 1, ld_y >= n_max < 2^30");
    UNAST_REQUIRE(pad_mode == 0 || pad_mode == 1, "unast_trim_bounds: pad_mode is 0 (reflect) or 1 (constant), got %d", pad_mode);
    UNAST_REQUIRE(top_db > 0.f, "unast_trim_bounds: top_db must be positive (got %g)", (double)top_db);
    const int nf_max = 1 + n_max / hop_length;
    UNAST_REQUIRE(ws && ws_floats >= (int64_t)B * nf_max, "unast_trim_bounds: the workspace needs B * (1 + n_max / hop_length) = %lld floats", (long long)B * nf_max);
    hipLaunchKernelGGL(trim_power_kernel, dim3(nf_max, B), dim3(TRIM_THREADS), 0, stream, y, (long long)ld_y, lens, nf_max, frame_length, hop_length,
                       pad_mode == 0 ? 1 : 0, ws);
    hipLaunchKernelGGL(trim_bounds_kernel, dim3(B), dim3(TRIM_THREADS), 0, stream, (const float*)ws, lens, nf_max, hop_length, top_db, out);
    return unast_check_launch("unast_trim_bounds");
}

extern "C" int unast_features(const float* y, int64_t ld_y, int n_max, const int* start, const int* samples, int B, int T_max, int n_fft, int hop, int win,
                              float coef, const float* window, const float* twiddle, const float* basis, const int* ranges, int n_mels, float ref_db,
                              float max_db, float* mel, float* mag, float* spec, hipStream_t stream) {
    if (int rc = check_stft_params("unast_features", B, T_max, n_fft, hop, win)) return rc;
    UNAST_REQUIRE(y && samples && window && twiddle && basis && ranges && mel && mag, "unast_features: null pointer");
    UNAST_REQUIRE(hop <= win, "unast_features: hop must not exceed win: a larger hop leaves samples no frame covers (hop=%d win=%d)", hop, win);
    UNAST_REQUIRE(n_mels >= 1 && n_mels <= 4096, "unast_features: need 1 <= n_mels <= 4096 (got %d)", n_mels);
    UNAST_REQUIRE(max_db > 0.f, "unast_features: max_db must be positive (got %g)", (double)max_db);
    const int min_frames = 1 + (n_fft / 2 + 1) / hop;
    UNAST_REQUIRE(T_max >= min_frames, "unast_features: T_max = %d holds no utterance: the shortest one, n_fft / 2 + 1 samples (the signal must be longer than the reflect "
                  "padding), has %d frames", T_max, min_frames);
    UNAST_REQUIRE(n_max > n_fft / 2 && n_max < (1 << 30) && ld_y >= n_max, "unast_features: need n_fft / 2 < n_max < 2^30 and a row stride of at least n_max (n_max=%d ld_y=%lld)",
                  n_max, (long long)ld_y);
    UNAST_REQUIRE((((uintptr_t)twiddle) & 7) == 0 && (((uintptr_t)spec) & 7) == 0, "unast_features: twiddle and spec hold complex values and need 8-byte alignment");
    hipLaunchKernelGGL(features_kernel, dim3(T_max, B), dim3(FFT_THREADS), 0, stream, y, (long long)ld_y, n_max, start, samples, T_max, n_fft, hop, win, coef, window,
                       (const float2*)twiddle, basis, ranges, n_mels, ref_db, max_db, mel, mag, (float2*)spec);
    return unast_check_launch("unast_features");
}

extern "C" int unast_preemphasis(const float* x, int64_t ld_x, float* y, int64_t ld_y, int n_max, const int* start, const int* lens, int B, float coef,
                                 hipStream_t stream) {
    UNAST_REQUIRE(x && y && lens && B >= 1 && B <= 65535, "unast_preemphasis: need x, y, lens and 1 <= B <= 65535 (B=%d)", B);
    UNAST_REQUIRE(x != y, "unast_preemphasis: not in place: sample k reads sample k - 1 of the input");
    UNAST_REQUIRE(n_max >= 1 && n_max < (1 << 30) && ld_x >= n_max && ld_y >= n_max, "unast_preemphasis: need 1 <= n_max < 2^30 and row strides of at least n_max (n_max=%d)", n_max);
    hipLaunchKernelGGL(preemphasis_kernel, dim3((unsigned)((n_max + 255) / 256), B), dim3(256), 0, stream, x, (long long)ld_x, y, (long long)ld_y, n_max, start, lens, coef);
    return unast_check_launch("unast_preemphasis");
}
