// f16x3_common.h -- shared by the two kernels that evaluate an f32 product on THREE f16 products (ode_f16x3w.hip: the point-CNF
// sampling solve; gemm_f16x3w.hip: the 128-point x 512-channel pointwise conv): the f16 MFMA on the hand-managed accumulator file,
// the packed conversion, the constants of the two-plane split and the power-of-two scale of a layer's weights.
// tests/f16x3_ref.py is the contract of the split.
#pragma once
#include "x6w_common.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 xh_f16x2 __attribute__((ext_vector_type(2)));

#define XH_ACT_SHIFT 4
#define XH_F16_LIMIT 65520.0f             // the smallest f32 that rounds to inf in f16
#define XH_FLUSH 0x1.ffcp-15f             // 2^-14 - 2^-25: below it rne16 gives a subnormal (at it, a tie, 2^-14)
#define XH_TAIL 64                        // behind a pack: int shift s (weights were multiplied by 2^s), unsigned bits of max |W|

template <int T, bool NOPS>
__device__ __forceinline__ void xh_mfma_a(f16x8 af, f16x8 bf)
{
    if constexpr (NOPS)
        asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 a[%c2:%c3], %0, %1, a[%c2:%c3]" : : "v"(af), "v"(bf), "i"(16 * T), "i"(16 * T + 15) : XW_ACLOB);
    else
        asm volatile("v_mfma_f32_32x32x16_f16 a[%c2:%c3], %0, %1, a[%c2:%c3]" : : "v"(af), "v"(bf), "i"(16 * T), "i"(16 * T + 15) : XW_ACLOB);
}

__device__ __forceinline__ unsigned xh_cvt_pk(float lo, float hi)
{
    const xc_f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, xh_f16x2));
}

// A plane word (two f16) with the halves whose exponent field is 0 -- subnormals and zeros -- set to +0: h * min(e, 1) per half, e the
// half shifted right by 10 (SIGNED: after the sign bits are masked out of it; without, for words whose halves are known non-negative).
// Exponent 31 (inf, NaN) passes.  Three / four single-pass VALU instructions for two values (v_pk_lshrrev_b16, v_pk_min_u16,
// v_pk_mul_lo_u16).  `ones` is 0x00010001 in a register the compiler cannot see through (xh_ones): with a literal it rewrites
// min(e, 1) as e != 0 and the product as a select, i.e. the compare per half this is here to avoid
typedef unsigned short xh_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned xh_ones()
{
    unsigned v = 0x00010001u;
    asm volatile("" : "+v"(v));
    return v;
}
template <bool SIGNED>
__device__ __forceinline__ unsigned xh_flush_word(unsigned w, unsigned ones)
{
    const xh_u16x2 h = __builtin_bit_cast(xh_u16x2, w);
    const xh_u16x2 e = __builtin_bit_cast(xh_u16x2, SIGNED ? (w & 0x7fff7fffu) : w) >> (unsigned short)10;
    return __builtin_bit_cast(unsigned, h * __builtin_elementwise_min(e, __builtin_bit_cast(xh_u16x2, ones)));
}

// the shift s that puts max |W| 2^s in [2^14, 2^15): 14 - floor(log2 max); 0 for an all-zero, subnormal or non-finite layer.  Clamped at
// XH_MAX_SHIFT so that the unscale factors 2^-s and 2^-(4 + s) the kernels fold into their read-out stay NORMAL f32 numbers (a gate times
// a subnormal factor would flush and the layer would put out its bias alone): a layer whose max |W| is below 2^-86 keeps shift 100 and
// loses residual-plane bits instead -- its whole product is below 512 x 4095 x 2^-86 = 3e-20, absolute
#define XH_MAX_SHIFT 100
__device__ __forceinline__ int h3_shift(unsigned maxbits)
{
    const int e = (int)(maxbits >> 23);
    return (e == 0 || e == 255) ? 0 : min(14 - (e - 127), XH_MAX_SHIFT);
}
