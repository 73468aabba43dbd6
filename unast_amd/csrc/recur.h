// Lane-exchange helpers of the persistent recurrent kernels (lstm.hip, vocoder.hip): gate exchange by permlane swaps and
// LDS-free recurrent dot products by DPP row rotations.
#pragma once
#include "common.h"

// Sums / exchanges over the four 16-lane rows of a wave by gfx950's permlane swaps (no LDS crossbar, no barrier).  Fed the same register
// twice, v_permlane16_swap returns (value of the pair's EVEN-row lane, value of its ODD-row lane) in every lane of a {l, l ^ 16} pair, and
// v_permlane32_swap (value of the lower-half lane, value of the upper-half lane) of a {l, l ^ 32} pair.
__device__ __forceinline__ void swap16(float v, float& even_row, float& odd_row) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    even_row = __uint_as_float(a[0]); odd_row = __uint_as_float(a[1]);
}
__device__ __forceinline__ void swap32(float v, float& lower, float& upper) {
    auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    lower = __uint_as_float(a[0]); upper = __uint_as_float(a[1]);
}

// The recurrent dot products without LDS broadcasts (round 4, second pass).  A lane holds ONE value per group of 16 source elements (one
// ds_read_b32: lane c of every 16-lane row has element 16 G + c), and the 16 values of a row reach every lane of it by DPP row rotations
// folded into the multiply-add (v_fmac_f32_dpp row_ror:n, full rate).  The weight a lane multiplies rotation n with belongs to the lane
// that rotation n reads from; that lane index comes from the same DPP operation applied to the lane id at kernel start (RotSrc), so
// nothing here depends on which way the hardware calls "right".
// One asm block per group: hipcc (ROCm 7.2) neither folds a v_mov_b32_dpp into the multiply-add nor schedules 16 separate asm statements
// without an s_nop between every four.  The first multiply-add is the unrotated one and an s_nop follows it: two wait states between
// whatever wrote `v` and the first DPP read of it (the hazard recogniser does not look inside asm).
template <int N>
__device__ __forceinline__ int row_ror_i(int v) { return __builtin_amdgcn_mov_dpp(v, 0x120 + N, 0xf, 0xf, true); }
template <int N>
struct RotSrc { static __device__ __forceinline__ void fill(int c, int (&src)[16]) { src[N] = row_ror_i<N>(c); RotSrc<N + 1>::fill(c, src); } };
template <> struct RotSrc<0> { static __device__ __forceinline__ void fill(int c, int (&src)[16]) { src[0] = c; RotSrc<1>::fill(c, src); } };
template <> struct RotSrc<16> { static __device__ __forceinline__ void fill(int, int (&)[16]) {} };
__device__ __forceinline__ float row_ror8(float v) { return __uint_as_float(__builtin_amdgcn_mov_dpp(__float_as_uint(v), 0x128, 0xf, 0xf, true)); }

// acc[n & 3] += w[n] * (v rotated by n) for n = 0..15: four independent chains.  FIRST: the chains START here (acc = the first four products:
// no zero-initialised accumulators -- every instruction of an in-order wave costs an issue slot of 4 cycles, a v_mov as much as a
// multiply-add).  VALU_SRC: `v` was written by a vector instruction (not an LDS read): the unrotated product first and an s_nop give the two
// wait states a DPP read of it needs.
template <bool FIRST, bool VALU_SRC>
__device__ __forceinline__ void dot16(const float (&w)[16], float v, float (&acc)[4]) {
#define D(n, a, wi) "v_fmac_f32_dpp %" #a ", %4, %" #wi " row_ror:" #n " row_mask:0xf bank_mask:0xf\n\t"
#define M(n, a, wi) "v_mul_f32_dpp %" #a ", %4, %" #wi " row_ror:" #n " row_mask:0xf bank_mask:0xf\n\t"
#define TAIL D(4, 0, 9) D(5, 1, 10) D(6, 2, 11) D(7, 3, 12) D(8, 0, 13) D(9, 1, 14) D(10, 2, 15) D(11, 3, 16) D(12, 0, 17) D(13, 1, 18) D(14, 2, 19) D(15, 3, 20)
#define OPS : "v"(v), "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]), "v"(w[4]), "v"(w[5]), "v"(w[6]), "v"(w[7]), "v"(w[8]), "v"(w[9]), "v"(w[10]), \
              "v"(w[11]), "v"(w[12]), "v"(w[13]), "v"(w[14]), "v"(w[15])
    if constexpr (FIRST && VALU_SRC)
        asm("v_mul_f32_e32 %0, %4, %5\n\ts_nop 0\n\t" M(1, 1, 6) M(2, 2, 7) M(3, 3, 8) TAIL : "=&v"(acc[0]), "=&v"(acc[1]), "=&v"(acc[2]), "=&v"(acc[3]) OPS);
    else if constexpr (FIRST)
        asm("v_mul_f32_e32 %0, %4, %5\n\t" M(1, 1, 6) M(2, 2, 7) M(3, 3, 8) TAIL : "=&v"(acc[0]), "=&v"(acc[1]), "=&v"(acc[2]), "=&v"(acc[3]) OPS);
    else if constexpr (VALU_SRC)
        asm("v_fmac_f32_e32 %0, %4, %5\n\ts_nop 0\n\t" D(1, 1, 6) D(2, 2, 7) D(3, 3, 8) TAIL : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]) OPS);
    else
        asm("v_fmac_f32_e32 %0, %4, %5\n\t" D(1, 1, 6) D(2, 2, 7) D(3, 3, 8) TAIL : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]) OPS);
#undef D
#undef M
#undef TAIL
#undef OPS
}
