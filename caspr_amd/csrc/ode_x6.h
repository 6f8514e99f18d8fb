// ode_x6.h -- shared between the bf16x6 point-CNF kernels (ode_bf16x6.hip and the three files that include its evaluation: 64 points
// per workgroup, 16x16x32 MFMA, sampling + divergence variants; ode_bf16x6w.hip: 128 points per workgroup, 32x32x16 MFMA, sampling).
#pragma once
#include "common.h"

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define XC_H 512

// The frame and the RK4 step count of a sampling workgroup (see CnfX6Args::steps_tab / order).  Both are workgroup-uniform.  A row of
// `order` outside 0 .. gridDim.y - 1 and a table entry outside 0 .. max_steps never reach an address or a loop bound as they are:
// the first skips the workgroup, the second is clamped.
// `on` = false (the divergence kernel): the plain frame and count, as a compile-time fact.
#define XC_FRAME_STEPS(a, bt, S, on)                                                                     \
    const int bt = ((on) && (a).order) ? (a).order[blockIdx.y] : (int)blockIdx.y;                        \
    if ((on) && (unsigned)bt >= gridDim.y) return;                                                       \
    const int S = ((on) && (a).steps_tab) ? min(max((a).steps_tab[bt], 0), (a).max_steps) : (a).steps;  \
    if ((on) && S == 0) return;   /* before anything of the frame is read or written; no DMA is in flight yet */

__device__ __forceinline__ void xc_split(float x, float &h1, float &h2, float &h3)
{
    h1 = __uint_as_float(__float_as_uint(x) & 0xffff0000u);
    const float r1 = x - h1;
    h2 = __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
    const float r2 = r1 - h2;
    h3 = __uint_as_float(__float_as_uint(r2) & 0xffff0000u);
}
// the same exact split for a pair of values with the hardware round-to-nearest conversion (v_cvt_pk_bf16_f32): the three
// packed words are the pair's entries of the three planes.  Exact as well: the remainder after rounding 24 bits to 8 has
// at most 15 significant bits, after the second rounding at most 7.  4.5 VALU operations per value instead of 5.5.
typedef __bf16 xc_bf16x2 __attribute__((ext_vector_type(2)));
typedef float xc_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void xc_split_pair(float x0, float x1, unsigned &p1, unsigned &p2, unsigned &p3)
{
    xc_f32x2 v = {x0, x1};
    p1 = __builtin_bit_cast(unsigned, __builtin_convertvector(v, xc_bf16x2));
    xc_f32x2 h = {__uint_as_float(p1 << 16), __uint_as_float(p1 & 0xffff0000u)};
    v = v - h;
    p2 = __builtin_bit_cast(unsigned, __builtin_convertvector(v, xc_bf16x2));
    h = (xc_f32x2){__uint_as_float(p2 << 16), __uint_as_float(p2 & 0xffff0000u)};
    v = v - h;
    p3 = __builtin_bit_cast(unsigned, __builtin_convertvector(v, xc_bf16x2));
}
__device__ __forceinline__ unsigned xc_pack(float lo, float hi) { return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u); }

struct CnfX6Args {
    const float *y_in, *hyper, *tcol, *w0, *b0, *b1, *b2, *w3, *b3, *mbn_in, *mbn_out;
    const float *e, *logp_in;     // DIV only: Hutchinson noise (BT,n,3), initial log-density (BT,n) or NULL
    float *logp_out;              // DIV only
    const unsigned char *w1x, *w2x;
    float *y_out;
    int ldh, n, steps, reverse;
    float t_end;
    // sampling kernels only (the *_frames_* entries; all NULL / 0 otherwise): a step count per frame and a launch order
    const int *steps_tab;         // (BT) or NULL: frame bt takes min(max(steps_tab[bt], 0), max_steps) steps, 0 = the frame is skipped
    int max_steps;
    const int *order;             // (BT) or NULL: workgroup row blockIdx.y works on frame order[blockIdx.y]
    unsigned long long *trace;   // debug build: s_memtime stamps of workgroup (0,0), thread 0, RK4 step 0 / stage 1
    int diag;                    // debug build: timing experiments (CASPR_X6_DIAG)
};

// ---- the 64-point kernels (ode_bf16x6.hip, ode_dp5.hip, ode_train_fwd.hip, ode_sample_tape.hip): LDS layout, the value <-> tangent
// column exchange and the scheduling regions of the evaluation they share as text (ode_x6_setup.inc, ode_x6_eval.inc)
#define XC_COLS 64
#define XC_PA (256 * 64)          // one plane of a piece
#define XC_PIECE (3 * XC_PA)      // 48 KB: 256 rows x 32 k x 3 planes
#define XC_NPIECE 32              // per layer: 16 k chunks x 2 row halves
#define XC_RING 2                 // LDS double buffer of pieces
#define XC_LDS (XC_RING * XC_PIECE + (6 * XC_H + 3 * XC_H + 3 * XC_H + 8) * 4)

// value of lane (l ^ 8) inside its 16-lane row: the partner column (value <-> tangent) of the same hidden-unit rows
__device__ __forceinline__ float xc_partner(float v) { return dpp_mov<0x128>(v); }   // row_ror:8
// tangent lanes (j >= 8 = DPP banks 2, 3 of every row) take the partner's value, value lanes keep their own: ONE
// v_mov_b32_dpp row_ror:8 bank_mask:0xC in place -- no select, no second register
__device__ __forceinline__ float xc_value_pre(float v)
{
    const int b = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(b, b, 0x128, 0xf, 0xC, false));
}

// The scheduling regions of a layer pass (ode_x6_eval.inc explains them where it uses them): sched_group_barrier builds the
// patterns, sched_barrier(0) closes a region.  Masks: 0x100 = LDS read, 0x008 = MFMA, 0x002 = VALU.
#define XC_SGB(mask, n) __builtin_amdgcn_sched_group_barrier(mask, n, 0);
#define XC_RM6 XC_SGB(0x100, 2) XC_SGB(0x008, 1) XC_SGB(0x100, 2) XC_SGB(0x008, 1) XC_SGB(0x100, 2) XC_SGB(0x008, 1) XC_SGB(0x100, 2) \
    XC_SGB(0x008, 1) XC_SGB(0x100, 2) XC_SGB(0x008, 1) XC_SGB(0x100, 2) XC_SGB(0x008, 1)
#define XC_VM4 XC_SGB(0x002, 2) XC_SGB(0x008, 1) XC_SGB(0x002, 2) XC_SGB(0x008, 1) XC_SGB(0x002, 2) XC_SGB(0x008, 1) XC_SGB(0x002, 2) XC_SGB(0x008, 1)
#define XC_REGION_PLAIN XC_RM6 XC_SGB(0x008, 18) __builtin_amdgcn_sched_barrier(0);
#define XC_REGION_TAB XC_RM6 XC_SGB(0x100, 5) XC_SGB(0x008, 18) __builtin_amdgcn_sched_barrier(0);
#define XC_REGION_VALU_S XC_RM6 XC_VM4 XC_VM4 XC_VM4 XC_VM4 XC_SGB(0x002, 2) XC_SGB(0x008, 2) __builtin_amdgcn_sched_barrier(0);
// DIV carries ~1.7x the producer VALU (value + tangent forms of the gated softplus): the reads are pinned as in the sampling
// variant, the VALU is left to the scheduler between the remaining MFMAs (a fixed 2-per-MFMA pattern strands the rest
// behind the region's last MFMA and sends ~450 registers to scratch)
#define XC_VM3 XC_SGB(0x002, 3) XC_SGB(0x008, 1) XC_SGB(0x002, 3) XC_SGB(0x008, 1) XC_SGB(0x002, 3) XC_SGB(0x008, 1) XC_SGB(0x002, 3) XC_SGB(0x008, 1)
#define XC_REGION_VALU_D XC_RM6 XC_VM3 XC_VM3 XC_VM3 XC_VM3 XC_SGB(0x002, 8) XC_SGB(0x008, 2) __builtin_amdgcn_sched_barrier(0);
#define XC_REGION_VALU if constexpr (DIV) { XC_REGION_VALU_D } else { XC_REGION_VALU_S }   // DIV: a compile-time bool of the including kernel

// ---- the 128-point kernel (ode_bf16x6w.hip)
#define XW_PTS 128
#define XW_FRAG 1024                      // one A fragment of v_mfma_f32_32x32x16_bf16: 64 lanes x 16 B
#define XW_PIECE (2 * 4 * 3 * XW_FRAG)    // 24 KB: [k-step 2][row tile 4][plane 3][fragment]
#define XW_PACK (4L * 16 * XW_PIECE)      // one hidden layer: [row quarter 4][k chunk 16][piece] = 1.5 MB
int caspr_cnf_x6w_launch(const CnfX6Args &a, int BT, hipStream_t stream) __attribute__((visibility("hidden")));
int caspr_cnf_x6w_pack(const float *w, int ldw, unsigned char *out, hipStream_t stream) __attribute__((visibility("hidden")));
