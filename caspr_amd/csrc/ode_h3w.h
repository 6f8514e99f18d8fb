// ode_h3w.h -- shared between the two kernels that run the 128-point f16x3 point-CNF evaluation (ode_f16x3w.hip: fixed-step RK4;
// ode_dp5_f16x3w.hip: adaptive Dormand-Prince): the layout of a weight piece, of the ring and of the tables in LDS, and the micro-steps
// of the softplus and of the two-plane split.  The evaluation itself is ode_h3w_setup.inc and ode_h3w_eval.inc.
// The including file defines, before the include, which instruction stream the text compiles to ("the wave's instruction
// stream"; same output bits with either form):
//   XH_OLD_FLUSH     the f32 compare-and-select flush instead of the flush on the f16 word
//   XH_OLD_DMA       an address and an M0 write per LDS-DMA instruction instead of one of each per piece
//   XH_NO_FLUSH1/2   NO flush of plane 1 / plane 2 (an experiment: WRONG results where a plane value is an f16 subnormal)
//   XH_STAMP(i)      a statement: phase stamp i of the stage (empty but in the RK4 kernel's debug build)
#pragma once
#include "f16x3_common.h"

#define XH_PTS 128
#define XH_FRAG 1024                      // one A fragment of v_mfma_f32_32x32x16_f16: 64 lanes x 16 B
#define XH_PIECE (2 * 4 * 2 * XH_FRAG)    // 16 KB: [k-step 2][row tile 4][plane 2][fragment]
#define XH_PACK (4L * 16 * XH_PIECE)      // one hidden layer: [row quarter 4][k chunk 16][piece] = 1 MB
#define XH_RING 8
#define XH_TAB (XH_RING * XH_PIECE)
// tables (floats): hb0[512] w0g[3][512] g1[512] hb1[512] g2[512] hb2[512] w3[3][512] w0[512][3] g3[8]
#define XH_TAB_FLOATS (14 * XC_H + 8)
#define XH_LDS (XH_TAB + XH_TAB_FLOATS * 4)

// ---- softplus on the scaled value X = 16 x, and the two-plane split, in micro-steps (XwPair of x6w_common.h) ----
__device__ __forceinline__ void xh_sp1(XwPair &p)     // u = 2^(-|x| log2 e), x = X / 16
{
    p.u0 = __builtin_amdgcn_exp2f(fabsf(p.x0) * -0.09016844005556021f);
    p.u1 = __builtin_amdgcn_exp2f(fabsf(p.x1) * -0.09016844005556021f);
}
__device__ __forceinline__ void xh_sp3(XwPair &p, float &xmax)     // X = max(X, 0) + 16 ln 2 * u == 16 softplus_fast(x); range tracking
{
    p.x0 = fmaxf(p.x0, 0.0f) + 11.090354888959125f * p.u0;
    p.x1 = fmaxf(p.x1, 0.0f) + 11.090354888959125f * p.u1;
    // (as asm: left to hipcc, the maxima are re-associated and sunk to the end of the stage, every X of the stage kept live for them)
    asm volatile("v_max3_f32 %0, %0, %1, %2" : "+v"(xmax) : "v"(p.x0), "v"(p.x1));
}
// The flush is done on the f16 WORD: x < XH_FLUSH holds exactly when rne16(x) has exponent field 0, so zeroing such a half after the
// conversion (xh_flush_word: packed 16-bit integer operations, no compare, no select, no VCC) gives the plane word that flushing the
// f32 value in front of it gave.  The remainder is taken from the unflushed X: for a flushed half it is X itself, below 2^-14, which
// the second plane's flush zeroes (to +0, whatever its sign) -- tests/test_f16x3_flush_word.py restates both forms on the CPU
__device__ __forceinline__ void xh_split1(XwPair &p, unsigned ones)  // first plane (flushed) + remainder; X >= 0 here
{
    if constexpr (XH_OLD_FLUSH) {
        const float a0 = p.x0 < XH_FLUSH ? 0.0f : p.x0, a1 = p.x1 < XH_FLUSH ? 0.0f : p.x1;
        p.p1 = xh_cvt_pk(a0, a1);
        const xh_f16x2 hv = __builtin_bit_cast(xh_f16x2, p.p1);
        p.r0 = a0 - (float)hv[0];
        p.r1 = a1 - (float)hv[1];
    } else {
        p.p1 = XH_NO_FLUSH1 ? xh_cvt_pk(p.x0, p.x1) : xh_flush_word<false>(xh_cvt_pk(p.x0, p.x1), ones);
        const xh_f16x2 hv = __builtin_bit_cast(xh_f16x2, p.p1);
        p.r0 = p.x0 - (float)hv[0];
        p.r1 = p.x1 - (float)hv[1];
    }
}
__device__ __forceinline__ void xh_split2(XwPair &p, u32x4 (&bw)[2], int q, unsigned ones)
{
    bw[0][q] = p.p1;
    if constexpr (XH_OLD_FLUSH) {
        const float r0 = fabsf(p.r0) < XH_FLUSH ? 0.0f : p.r0, r1 = fabsf(p.r1) < XH_FLUSH ? 0.0f : p.r1;
        bw[1][q] = xh_cvt_pk(r0, r1);
    } else {
        bw[1][q] = XH_NO_FLUSH2 ? xh_cvt_pk(p.r0, p.r1) : xh_flush_word<true>(xh_cvt_pk(p.r0, p.r1), ones);
    }
}
// a plane word (two f16) in / out of the accumulator file, bits untouched
template <int N>
__device__ __forceinline__ unsigned xh_acc_rd_u()
{
    unsigned x;
    asm volatile("v_accvgpr_read_b32 %0, a%c1" : "=v"(x) : "i"(N));
    return x;
}
template <int N>
__device__ __forceinline__ void xh_acc_wr_u(unsigned x)
{
    asm volatile("v_accvgpr_write_b32 a%c1, %0" : : "v"(x), "i"(N) : XW_ACLOB);
}
