// ode_f16x3w.hip -- the point-CNF SAMPLING solve on THREE f16 products per f32 product (config.cnf_split = "f16x3"): the geometry of
// ode_bf16x6w.hip (128 points per workgroup, a wave owns 32 points and all 512 units, layer 1's 256 accumulators in the hand-managed
// accumulator file, layer 2 in four passes, weights through an LDS ring by LDS-DMA, MovingBatchNorm prologue / epilogue, layers 0 and
// 3 in f32) with half the matrix-pipe instructions.  The body is a copy of that kernel's on purpose (as ode_dp5.hip's and
// ode_train_fwd.hip's are of the 64-point kernel); read its header first, this one lists the differences.
//
//  * the scheme: an f32 operand x 2^k is split into two f16 planes by round-to-nearest (p1 = rne16(x), p2 = rne16(x - p1): 22
//    significant bits), and  a . b ~ a2 b1 + a1 b2 + a1 b1  on v_mfma_f32_32x32x16_f16, smallest terms first.  The dropped a2 b2 is
//    about 2^-24 |a| |b|.  tests/f16x3_ref.py is the contract, tests/test_f16x3_emulation.py its error against f64;
//  * the exponent range: hidden activations come out of a softplus and are scaled by 2^4 (|x| < 4094 stays finite in f16; anything
//    above 2^-7 keeps both planes normal), a layer's weights by the power of two that puts max |W| in [2^14, 2^15) -- computed ON THE
//    DEVICE at pack time (max-reduction, no host round trip) and stored behind the pack, where this kernel reads it.  Both scales are
//    exact; they are undone in the stage's gate tables (g1 2^-s1 with the next layer's 2^4 folded in, g2 2^-(4 + s2)), at no cost;
//  * the kernel carries the SCALED activation X = 16 softplus(x): the 2^4 sits in the tables of the producing layer, and
//    softplus works on X directly (exp2 of |X| log2 e / 16, 16 ln 2 outside): the same roundings as on x, no extra instruction;
//  * the accumulator file in layer 2 holds the two f16 PLANES of hidden layer 1's activations, not X: pass 0 splits a group of four
//    values once and writes its four plane words over the four sums; passes 1-3 read them back as B operands and do no arithmetic
//    (the bf16x6 kernel has to keep X: three bf16 planes are 48 bits a value);
//  * plane values below 2^-14 (f16 subnormals) are flushed to zero explicitly, so nothing depends on the pipe's subnormal handling;
//  * range guard: a lane tracks the maximum of the X it splits; a point whose maximum is not below 65520 (not finite in f16) gets NaN
//    in all three outputs and the launch's status word is set (ops.check_deferred_errors reports it and names cnf_split="bf16x6");
//  * weights: 16 KB pieces [k-step 2][row tile 4][plane 2][1 KB fragment], 24 MFMAs (768 matrix-pipe cycles) each, through an
//    EIGHT-deep ring: a piece lasts half as long as the bf16x6 kernel's, so the same flight time needs twice the pieces in flight.
//    Piece s + 7 is issued (4 LDS-DMA instructions per wave) while piece s is multiplied, into the slot piece s - 1 left at the
//    barrier in its last region; that barrier waits with vmcnt(24): the six younger pieces may still be in flight;
//  * a region is one k-step x two row tiles = 6 MFMAs, one scheduling slot each; slots 0-3 read the next region's four fragments; the
//    producers run two micro-steps per slot in pass 0 of layer 2 (the same work per k-step under half the MFMAs).
#include "f16x3_common.h"

// XW_EXP (debug flavours only, build.py CASPR_XW_EXP): 16 = no phase stamps; 65536 / 131072 = the instruction stream of the parent for
// ONE item of "the wave's instruction stream" (DESIGN.md 3): the f32 compare-and-select flush, an address and an M0 write per LDS-DMA
// instruction.  Same output bits with either set.  1048576 / 2097152 = NO flush of plane 1 / plane 2 (WRONG results where a plane
// value is an f16 subnormal: what tests/test_cnf_f16x3_flush_band.py must notice).
#ifndef XW_EXP
#define XW_EXP 0
#endif
#define XH_OLD_FLUSH ((XW_EXP & 65536) != 0)
#define XH_OLD_DMA ((XW_EXP & 131072) != 0)
#define XH_NO_FLUSH1 ((XW_EXP & 1048576) != 0)
#define XH_NO_FLUSH2 ((XW_EXP & 2097152) != 0)
// debug build (tools/cnf_h3w_trace.py): s_memtime stamps of workgroup (0,0), thread 0, RK4 step 0, sixteen slots per stage: 0 stage head,
// 1 tables built, 2 chunk 0 of the input layer done, 3 layer 1 done, 4 + 2 q the K loop of pass q done, 5 + 2 q its epilogue, 12 stage end.
// The stamped kernel does NOT fit its registers (115 VGPRs spilled with the tested compiler, as the bf16x6 kernel's stamped flavour spills
// 134): its scratch traffic shares vmcnt with the weight ring, so the split is indicative and a stamped stage is far slower than a real one
#if defined(CASPR_DEBUG_HOOKS) && !(XW_EXP & 16)
#define XH_STAMP(i) if (a.trace && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0 && step == 0) a.trace[16 * stage + (i)] = __builtin_amdgcn_s_memtime();
#else
#define XH_STAMP(i)
#endif

#define XH_PTS 128
#define XH_FRAG 1024                      // one A fragment of v_mfma_f32_32x32x16_f16: 64 lanes x 16 B
#define XH_PIECE (2 * 4 * 2 * XH_FRAG)    // 16 KB: [k-step 2][row tile 4][plane 2][fragment]
#define XH_PACK (4L * 16 * XH_PIECE)      // one hidden layer: [row quarter 4][k chunk 16][piece] = 1 MB
#define XH_RING 8
#define XH_TAB (XH_RING * XH_PIECE)
// tables (floats): hb0[512] w0g[3][512] g1[512] hb1[512] g2[512] hb2[512] w3[3][512] w0[512][3] g3[8]
#define XH_TAB_FLOATS (14 * XC_H + 8)
#define XH_LDS (XH_TAB + XH_TAB_FLOATS * 4)

struct CnfH3Args : CnfX6Args {
    unsigned *status;                     // one word per launch, zeroed in front of it: != 0 <-> the range guard tripped
};

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

__global__ __launch_bounds__(256, 1) void cnf_rk4_h3w_kernel(CnfH3Args a)
{
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    unsigned char *wbuf = lds;                      // [XH_RING][XH_PIECE]
    float *s_hb0 = (float *)(lds + XH_TAB);         // [512]     layer 0: (bias * gate + hyper bias) * 16
    float *s_w0g = s_hb0 + XC_H;                    // [3][512]  layer 0: weight column d * gate * 16
    float *s_g1 = s_w0g + 3 * XC_H;                 // [512]     sigmoid gate of hidden layer 1 * 2^-s1 (= gate * 2^-(4 + s1) * 16)
    float *s_hb1 = s_g1 + XC_H;                     //           ... its bias * 16
    float *s_g2 = s_hb1 + XC_H;                     // [512]     gate of hidden layer 2 * 2^-(4 + s2)
    float *s_hb2 = s_g2 + XC_H;
    float *s_w3 = s_hb2 + XC_H;                     // [3][512]  output layer
    float *s_w0 = s_w3 + 3 * XC_H;                  // [512][3]  input layer (raw)
    float *s_g3 = s_w0 + 3 * XC_H;                  // [8]: gate3[3], pad, hb3[3]

    const int tid = threadIdx.x, lane0 = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    XC_FRAME_STEPS(a, bt, S, true)
    const float *hy = a.hyper + (long)bt * a.ldh;
    constexpr int BOFF = 3 * XC_H + 3;

    for (int i = tid; i < 3 * XC_H; i += 256) {
        s_w0[i] = a.w0[i];
        s_w3[i] = a.w3[i];
    }
    // the weight scales the pack kernel chose: W1 2^s1, W2 2^s2 are what the planes hold
    const int sh1 = *(const int *)(a.w1x + XH_PACK), sh2 = *(const int *)(a.w2x + XH_PACK);
    const float act = (float)(1 << XH_ACT_SHIFT), un1 = ldexpf(1.0f, -sh1), un2 = ldexpf(1.0f, -(XH_ACT_SHIFT + sh2));

    const int col = blockIdx.x * XH_PTS + 32 * wave + (lane0 & 31);
    const bool cvalid = col < a.n;
    const int ccol = cvalid ? col : a.n - 1;
    float y[3], kacc[3] = {0.f, 0.f, 0.f}, kprev[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        float v = a.y_in[((long)bt * a.n + ccol) * 3 + d];
        if (a.mbn_in) {
            const float w = a.mbn_in[d], bb = a.mbn_in[3 + d], mean = a.mbn_in[6 + d], var = a.mbn_in[9 + d];
            if (a.reverse) v = (v - bb) * expf(-w) * expf(0.5f * logf(var + 1e-4f)) + mean;   // normalization.py:92-94
            else v = (v - mean) * expf(-0.5f * logf(var + 1e-4f)) * expf(w) + bb;             // normalization.py:70-74
        }
        y[d] = v;
    }

    float kc_g[2][3], kc_hb[2][3], kc_tg[2][3], kc_tb[2][3], kc_b[2][3];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            const int i = l * XC_H + tid + 256 * u;
            kc_g[u][l] = hy[i];
            kc_hb[u][l] = hy[BOFF + i];
            kc_tg[u][l] = a.tcol[i];
            kc_tb[u][l] = a.tcol[BOFF + i];
            kc_b[u][l] = (l == 0 ? a.b0 : (l == 1 ? a.b1 : a.b2))[tid + 256 * u];
        }
    const int t3 = tid < 3 ? tid : 0;
    const float k3_g = hy[3 * XC_H + t3], k3_hb = hy[BOFF + 3 * XC_H + t3], k3_tg = a.tcol[3 * XC_H + t3], k3_tb = a.tcol[BOFF + 3 * XC_H + t3], k3_b = a.b3[t3];

    // The weight stream of one stage: 128 pieces, layer 1 chunk-major (s = 4 kc + rq), then layer 2 pass-major (s = 64 + 16 q + kc);
    // piece (rq, kc) of a layer's pack sits at (rq * 16 + kc) * XH_PIECE.  Ring slot s & 7.
    auto piece_src = [&](int s_) -> const unsigned char * {
        s_ &= 127;
        const int l2 = s_ >> 6, t_ = s_ & 63;
        const int rq = l2 ? (t_ >> 4) : (t_ & 3), kc = l2 ? (t_ & 15) : (t_ >> 2);
        return (l2 ? a.w2x : a.w1x) + (long)(rq * 16 + kc) * XH_PIECE;
    };
    // LDS-DMA of kilobyte i0 (0..3) of this wave's 4 KB share of sequence piece s_: ONE global_load_lds_dwordx4 in the SADDR form (see
    // ode_bf16x6w.hip); M0 has no other user in this kernel (audit.py)
    auto dma1 = [&](int s_, int lane16, int i0) XW_INL {
        const unsigned char *src = piece_src(s_) + (wave * 4 + i0) * 1024;
        const unsigned dst = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)(wbuf + (s_ & (XH_RING - 1)) * XH_PIECE + (wave * 4 + i0) * 1024);
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" : : "s"(dst), "v"(lane16), "s"(src) : "memory");
    };
    // ... and the four of a piece on ONE source address and ONE M0 write: kilobyte i0 is 1024 i0 further on both sides, which is
    // what the instruction's immediate offset adds to the global AND to the LDS address.  dma_open (the wave's share of piece s_:
    // M0 <- its place in the ring, returns its place in the pack) goes into the slot in front of the first dma_kb, so that an MFMA
    // supplies the wait state between the M0 write and the load; M0 then stays put until the next piece's dma_open
    auto dma_open = [&](int s_) XW_INL -> const unsigned char * {
        const unsigned dst = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)(wbuf + (s_ & (XH_RING - 1)) * XH_PIECE + wave * 4096);
        asm volatile("s_mov_b32 m0, %0" : : "s"(dst) : "memory");
        return piece_src(s_) + wave * 4096;
    };
    auto dma_kb = [&](const unsigned char *src, int lane16, auto I0) XW_INL {
        asm volatile("global_load_lds_dwordx4 %0, %1 offset:%c2" : : "v"(lane16), "s"(src), "i"(1024 * decltype(I0)::value) : "memory");
    };
    const double t0 = a.reverse ? (double)a.t_end : 0.0, t1 = a.reverse ? 0.0 : (double)a.t_end;
    const double h = (t1 - t0) / (double)S;
    const float hh = (float)h, h2 = (float)(0.5 * h), h6 = (float)(h / 6.0);

    // pieces 0..6 in flight before the first one is consumed
#pragma unroll
    for (int s_ = 0; s_ < XH_RING - 1; ++s_) {
        if constexpr (XH_OLD_DMA) {
#pragma unroll
            for (int i0 = 0; i0 < 4; ++i0) dma1(s_, lane0 * 16, i0);
        } else {
            const unsigned char *src = dma_open(s_);
            asm volatile("s_nop 0" ::: "memory");      // M0 write -> LDS-DMA: one wait state (no MFMA in between here)
            xw_for<0, 4>([&](auto I0) XW_INL { dma_kb(src, lane0 * 16, I0); });
        }
    }

    f32x16 acc2[4];               // layer 2: the 128 rows of the running pass
    f16x8 fX[2][2], fY[2][2];     // A fragments: two sets of two row tiles x two planes
    u32x4 b1w[2][2][2];           // layer 1 B planes [chunk parity][k-step of the chunk][plane]
    u32x4 b2w[2][2];              // layer 2 B planes [k-step parity][plane]
    float xmax = 0.0f;            // range guard: the largest scaled activation this lane has split
    const unsigned ones = xh_ones();   // for the flush of the plane words

    // fragments of region 0 of piece 0 (k-step 0, row tiles 0, 1): the only exposed fragment read of the kernel
    asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    {
        const unsigned char *A0 = wbuf + lane0 * 16;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) fX[u][pl] = *(const f16x8 *)(A0 + (u * 2 + pl) * XH_FRAG);
    }

    for (int step = 0; step < S; ++step) {
#pragma unroll 1
        for (int stage = 0; stage < 4; ++stage) {
            const double tc = (stage == 0) ? 0.0 : (stage == 3 ? 1.0 : 0.5);
            const float t = (float)(t0 + (double)step * h + tc * h);
            const float aw = (stage == 0) ? 0.f : (stage == 3 ? hh : h2);
            int lane = lane0;
            asm volatile("" : "+v"(lane));     // opaque: nothing derived from the lane id is hoisted out of the stage loop
            const int hq = (lane >> 5) * 4, lane16 = lane * 16;
            // layer 1 accumulates from zero (issued before the barrier: overlaps the other waves' arrival)
            XH_STAMP(0)
            xw_for<0, 256>([&](auto N) XW_INL { xw_acc_zero<decltype(N)::value>(); });
            __syncthreads();   // the previous stage's epilogues are done with the tables
            // (RK4 stages 1 and 2 both sit at t + h / 2 and build the same tables; skipping the second build and its barrier was measured and
            // is not worth a branch here: the launch is as fast with it)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int i = tid + 256 * u;
                const float g0 = sigmoid_fast(fmaf(t, kc_tg[u][0], kc_g[u][0]));
                s_hb0[i] = fmaf(kc_b[u][0], g0, fmaf(t, kc_tb[u][0], kc_hb[u][0])) * act;
                s_w0g[i] = s_w0[3 * i] * g0 * act;
                s_w0g[XC_H + i] = s_w0[3 * i + 1] * g0 * act;
                s_w0g[2 * XC_H + i] = s_w0[3 * i + 2] * g0 * act;
                const float g1 = sigmoid_fast(fmaf(t, kc_tg[u][1], kc_g[u][1]));
                s_g1[i] = g1 * un1;
                s_hb1[i] = fmaf(kc_b[u][1], g1, fmaf(t, kc_tb[u][1], kc_hb[u][1])) * act;
                const float g2 = sigmoid_fast(fmaf(t, kc_tg[u][2], kc_g[u][2]));
                s_g2[i] = g2 * un2;
                s_hb2[i] = fmaf(kc_b[u][2], g2, fmaf(t, kc_tb[u][2], kc_hb[u][2]));
            }
            if (tid < 3) {
                const float gt = sigmoid_fast(fmaf(t, k3_tg, k3_g));
                s_g3[tid] = gt;
                s_g3[4 + tid] = fmaf(k3_b, gt, fmaf(t, k3_tb, k3_hb));
            }
            __syncthreads();
            XH_STAMP(1)

            float ys[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) ys[d] = (stage == 0) ? y[d] : y[d] + aw * kprev[d];

            // barrier in front of the next sequence piece (placed in the last region of a piece): this wave's share of it has
            // landed once at most the 24 DMA instructions of the six younger pieces are outstanding; lgkmcnt: this wave's
            // reads of the ring slot that the DMA issued in the next piece refills
            auto piece_head = [&]() XW_INL {
                asm volatile("s_waitcnt vmcnt(24) lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
            };
            // one scheduling slot per MFMA: MFMA i of a region multiplies term i >> 1 (smallest first: a2 b1, a1 b2, a1 b1) into
            // row tile i & 1 of the pair; slots 0-3 also read the four fragments of the NEXT region, `fill` adds the slot's
            // producer micro-steps.  The MFMA goes first, fenced (see ode_bf16x6w.hip)
            constexpr int TA[3] = {1, 0, 0}, TB[3] = {0, 1, 0};
            auto region_a = [&](auto T0C, const f16x8 (&fc)[2][2], const u32x4 (&b)[2], f16x8 (&fn)[2][2], const unsigned char *An_, auto &&fill) XW_INL {
                constexpr int T0 = decltype(T0C)::value;
                const f16x8 bb[2] = {__builtin_bit_cast(f16x8, b[0]), __builtin_bit_cast(f16x8, b[1])};
                xw_for<0, 6>([&](auto I) XW_INL {
                    constexpr int i = decltype(I)::value;
                    xh_mfma_a<T0 + (i & 1), (i < 2)>(fc[i & 1][TA[i >> 1]], bb[TB[i >> 1]]);
                    XW_FENCE;
                    if constexpr (i < 4) fn[i >> 1][i & 1] = *(const f16x8 *)(An_ + i * XH_FRAG);
                    fill(I);
                    XW_FENCE;
                });
            };
            // ... the last region of a piece: the next piece's barrier after the first two MFMAs, its first fragments after it
            auto region_a_last = [&](auto T0C, const f16x8 (&fc)[2][2], const u32x4 (&b)[2], f16x8 (&fn)[2][2], const unsigned char *An_, auto &&fill) XW_INL {
                constexpr int T0 = decltype(T0C)::value;
                const f16x8 bb[2] = {__builtin_bit_cast(f16x8, b[0]), __builtin_bit_cast(f16x8, b[1])};
                xw_for<0, 6>([&](auto I) XW_INL {
                    constexpr int i = decltype(I)::value;
                    if constexpr (i == 2) {
                        piece_head();
                        XW_FENCE;
                    }
                    xh_mfma_a<T0 + (i & 1), (i < 2)>(fc[i & 1][TA[i >> 1]], bb[TB[i >> 1]]);
                    XW_FENCE;
                    if constexpr (i >= 2) fn[(i - 2) >> 1][(i - 2) & 1] = *(const f16x8 *)(An_ + (i - 2) * XH_FRAG);
                    fill(I);
                    XW_FENCE;
                });
            };
            // layer 2: row tiles c0, c1 in hipcc's registers
            auto region_v = [&](f32x16 &c0, f32x16 &c1, const f16x8 (&fc)[2][2], const u32x4 (&b)[2], f16x8 (&fn)[2][2], const unsigned char *An_, auto &&fill) XW_INL {
                const f16x8 bb[2] = {__builtin_bit_cast(f16x8, b[0]), __builtin_bit_cast(f16x8, b[1])};
                xw_for<0, 6>([&](auto I) XW_INL {
                    constexpr int i = decltype(I)::value;
                    if constexpr ((i & 1) == 0) c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fc[0][TA[i >> 1]], bb[TB[i >> 1]], c0, 0, 0, 0);
                    else c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fc[1][TA[i >> 1]], bb[TB[i >> 1]], c1, 0, 0, 0);
                    XW_FENCE;
                    if constexpr (i < 4) fn[i >> 1][i & 1] = *(const f16x8 *)(An_ + i * XH_FRAG);
                    fill(I);
                    XW_FENCE;
                });
            };
            auto region_v_last = [&](f32x16 &c0, f32x16 &c1, const f16x8 (&fc)[2][2], const u32x4 (&b)[2], f16x8 (&fn)[2][2], const unsigned char *An_, auto &&fill) XW_INL {
                const f16x8 bb[2] = {__builtin_bit_cast(f16x8, b[0]), __builtin_bit_cast(f16x8, b[1])};
                xw_for<0, 6>([&](auto I) XW_INL {
                    constexpr int i = decltype(I)::value;
                    if constexpr (i == 2) {
                        piece_head();
                        XW_FENCE;
                    }
                    if constexpr ((i & 1) == 0) c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fc[0][TA[i >> 1]], bb[TB[i >> 1]], c0, 0, 0, 0);
                    else c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fc[1][TA[i >> 1]], bb[TB[i >> 1]], c1, 0, 0, 0);
                    XW_FENCE;
                    if constexpr (i >= 2) fn[(i - 2) >> 1][(i - 2) & 1] = *(const f16x8 *)(An_ + (i - 2) * XH_FRAG);
                    fill(I);
                    XW_FENCE;
                });
            };

            // ================= layer 1: 16 chunks x 4 row quarters, sequence pieces 0..63 =================
            // B fragment of k-step t (T = t >> 1, u = t & 1), lane (j, h): slot s <-> unit 32 T + 16 u + (s & 3) + 8 (s >> 2) + 4 h:
            // group 0 (slots 0-3, words 0, 1) = four consecutive units from ub = 16 t + 4 h, group 1 (words 2, 3) from ub + 8
            f32x4 tin[4];         // input-layer tables of the group being produced: hb0, w0g x / y / z (all x 16)
            XwPair pa, pb;
            auto l1_tab = [&](int ub) XW_INL {
                tin[0] = ld4(s_hb0 + ub);
                tin[1] = ld4(s_w0g + ub);
                tin[2] = ld4(s_w0g + XC_H + ub);
                tin[3] = ld4(s_w0g + 2 * XC_H + ub);
            };
            auto l1_pre = [&](XwPair &p, int pr) XW_INL {      // units 2 pr, 2 pr + 1 of the group
                p.x0 = fmaf(tin[1][2 * pr], ys[0], fmaf(tin[2][2 * pr], ys[1], fmaf(tin[3][2 * pr], ys[2], tin[0][2 * pr])));
                p.x1 = fmaf(tin[1][2 * pr + 1], ys[0], fmaf(tin[2][2 * pr + 1], ys[1], fmaf(tin[3][2 * pr + 1], ys[2], tin[0][2 * pr + 1])));
            };
            // the six micro-steps of pair pr of a group, one per slot of a region
            auto l1_pair_step = [&](auto I, u32x4 (&bw)[2], int grp, int pr) XW_INL {
                constexpr int i = decltype(I)::value;
                if constexpr (i == 0) l1_pre(pa, pr);
                if constexpr (i == 1) xh_sp1(pa);
                if constexpr (i == 2) xw_sp2(pa);
                if constexpr (i == 3) xh_sp3(pa, xmax);
                if constexpr (i == 4) xh_split1(pa, ones);
                if constexpr (i == 5) xh_split2(pa, bw, 2 * grp + pr, ones);
            };
            // chunk 0 of the input layer up front (exposed: 1/16 of the input layer)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int grp = 0; grp < 2; ++grp) {
                    l1_tab(16 * ks + 8 * grp + hq);
#pragma unroll
                    for (int pr = 0; pr < 2; ++pr) {
                        l1_pre(pa, pr);
                        xh_sp1(pa);
                        xw_sp2(pa);
                        xh_sp3(pa, xmax);
                        xh_split1(pa, ones);
                        xh_split2(pa, b1w[0][ks], 2 * grp + pr, ones);
                    }
                }
            XW_FENCE;
            XH_STAMP(2)
#pragma unroll 1
            for (int it = 0; it < 8; ++it) {
                xw_for<0, 8>([&](auto PC) XW_INL {
                    constexpr int pc = decltype(PC)::value, par = pc >> 2, rq = pc & 3;   // chunk kc = 2 it + par, ring slot = pc
                    const int s1 = 8 * it + pc;                                            // sequence piece
                    const unsigned char *A = wbuf + pc * XH_PIECE + lane16;
                    const unsigned char *An = wbuf + ((pc + 1) & (XH_RING - 1)) * XH_PIECE + lane16;
                    // producers of chunk kc + 1 (B set par ^ 1): piece rq makes group (ks = rq >> 1, grp = rq & 1): tables in
                    // region 0, one pair in regions 1 and 2 each.  (Chunk 16 does not exist: the last pass produces chunk 0 once
                    // more -- values the range guard has already seen -- into a B set nobody multiplies.  Skipping it takes a uniform
                    // branch in each of the 13 producer slots of pieces 4-7: hipcc turns those into more instructions in the seven
                    // passes that produce than the eighth saves)
                    const int ubn = 32 * ((2 * it + par + 1) & 15) + 16 * (rq >> 1) + 8 * (rq & 1) + hq;
                    u32x4 (&bn)[2] = b1w[par ^ 1][rq >> 1];
                    const unsigned char *dsrc = nullptr;     // this wave's share of piece s1 + 7 in the pack (dma_open)
                    auto dma = [&](auto I0) XW_INL {
                        if constexpr (XH_OLD_DMA) dma1(s1 + 7, lane16, decltype(I0)::value);
                        else dma_kb(dsrc, lane16, I0);
                    };
                    // region 0: k-step 0, row tiles 0, 1 (fX) | reads k-step 0, row tiles 2, 3 -> fY
                    region_a(std::integral_constant<int, 4 * rq>{}, fX, b1w[par][0], fY, A + 4 * XH_FRAG, [&](auto I) XW_INL {
                        constexpr int i = decltype(I)::value;
                        if constexpr (i == 0) l1_tab(ubn);
                        if constexpr (i == 3 && !XH_OLD_DMA) dsrc = dma_open(s1 + 7);
                        if constexpr (i == 4) dma(std::integral_constant<int, 0>{});
                    });
                    // region 1: k-step 0, row tiles 2, 3 (fY) | reads k-step 1, row tiles 0, 1 -> fX
                    region_a(std::integral_constant<int, 4 * rq + 2>{}, fY, b1w[par][0], fX, A + 8 * XH_FRAG, [&](auto I) XW_INL {
                        constexpr int i = decltype(I)::value;
                        l1_pair_step(I, bn, rq & 1, 0);
                        if constexpr (i == 3) dma(std::integral_constant<int, 1>{});
                    });
                    // region 2: k-step 1, row tiles 0, 1 (fX) | reads k-step 1, row tiles 2, 3 -> fY
                    region_a(std::integral_constant<int, 4 * rq>{}, fX, b1w[par][1], fY, A + 12 * XH_FRAG, [&](auto I) XW_INL {
                        constexpr int i = decltype(I)::value;
                        l1_pair_step(I, bn, rq & 1, 1);
                        if constexpr (i == 3) dma(std::integral_constant<int, 2>{});
                    });
                    // region 3: the last kilobyte of piece s1 + 7 | barrier of the next piece | k-step 1, row tiles 2, 3 (fY) | reads
                    // the next piece's k-step 0, row tiles 0, 1 -> fX
                    region_a_last(std::integral_constant<int, 4 * rq + 2>{}, fY, b1w[par][1], fX, An, [&](auto I) XW_INL {
                        constexpr int i = decltype(I)::value;
                        if constexpr (i == 1) dma(std::integral_constant<int, 3>{});
                    });
                });
            }
            XH_STAMP(3)

            // ================= layer 2: four passes of 16 pieces, sequence pieces 64 + 16 q + kc =================
            float part[3] = {0.f, 0.f, 0.f};
            f32x4 tt[2][2];       // gate1 / hb1 of a group, [region parity][gate | bias], read one region ahead
            float qv[4];
            auto l2_tab = [&](int set, int t_, int grp) XW_INL {
                const int c = 16 * t_ + 8 * grp + hq;
                tt[set][0] = ld4(s_g1 + c);
                tt[set][1] = ld4(s_hb1 + c);
            };
            // Producer of group GRP of k-step T_ (registers a[16 (T_ >> 1) + 8 (T_ & 1) + 4 GRP + r], r = 0..3), by slot.  FIRST
            // pass: gate / bias / softplus / split, and the group's four plane words (p1, p2 of pair a, p1, p2 of pair b: two f16
            // planes of a value pair are exactly two 32-bit words) take the place of the four sums in the accumulator file; later
            // passes: four reads straight into the B planes, no arithmetic (the range guard has seen every X in pass 0).
            auto l2_step = [&](auto I, auto TC, auto GC, auto FC, u32x4 (&bw)[2], int set) XW_INL {
                constexpr int i = decltype(I)::value, t_ = decltype(TC)::value, grp = decltype(GC)::value;
                constexpr bool first = decltype(FC)::value;
                constexpr int base = 16 * (t_ >> 1) + 8 * (t_ & 1) + 4 * grp;
                if constexpr (first) {
                    if constexpr (i == 0) {
                        qv[0] = xw_acc_rd<base>();
                        qv[1] = xw_acc_rd<base + 1>();
                        qv[2] = xw_acc_rd<base + 2>();
                        qv[3] = xw_acc_rd<base + 3>();
                        pa.x0 = fmaf(qv[0], tt[set][0][0], tt[set][1][0]);
                        pa.x1 = fmaf(qv[1], tt[set][0][1], tt[set][1][1]);
                        pb.x0 = fmaf(qv[2], tt[set][0][2], tt[set][1][2]);
                        pb.x1 = fmaf(qv[3], tt[set][0][3], tt[set][1][3]);
                    }
                    if constexpr (i == 1) {
                        xh_sp1(pa);
                        xh_sp1(pb);
                    }
                    if constexpr (i == 2) {
                        xw_sp2(pa);
                        xw_sp2(pb);
                    }
                    if constexpr (i == 3) {
                        xh_sp3(pa, xmax);
                        xh_sp3(pb, xmax);
                    }
                    if constexpr (i == 4) {
                        xh_split1(pa, ones);
                        xh_split1(pb, ones);
                    }
                    if constexpr (i == 5) {
                        xh_split2(pa, bw, 2 * grp, ones);
                        xh_split2(pb, bw, 2 * grp + 1, ones);
                        xh_acc_wr_u<base>(bw[0][2 * grp]);
                        xh_acc_wr_u<base + 1>(bw[1][2 * grp]);
                        xh_acc_wr_u<base + 2>(bw[0][2 * grp + 1]);
                        xh_acc_wr_u<base + 3>(bw[1][2 * grp + 1]);
                    }
                } else {
                    if constexpr (i == 0) {
                        bw[0][2 * grp] = xh_acc_rd_u<base>();
                        bw[1][2 * grp] = xh_acc_rd_u<base + 1>();
                        bw[0][2 * grp + 1] = xh_acc_rd_u<base + 2>();
                        bw[1][2 * grp + 1] = xh_acc_rd_u<base + 3>();
                    }
                }
            };
            auto pass = [&](int q, auto FC) XW_INL {
                constexpr bool first = decltype(FC)::value;
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc2[mi][r] = 0.f;
                // k-step 0 of this pass up front (exposed); the tables of (k-step 1, group 0) for region 0
                if constexpr (first) {
                    l2_tab(0, 0, 0);
                    l2_tab(1, 0, 1);
                }
                xw_for<0, 6>([&](auto I) XW_INL { l2_step(I, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, FC, b2w[0], 0); });
                xw_for<0, 6>([&](auto I) XW_INL { l2_step(I, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{}, FC, b2w[0], 1); });
                if constexpr (first) l2_tab(0, 1, 0);
                // passes 1-3: the plane words go from the accumulator read straight into hipcc's first MFMA, which does not see a
                // VALU write in the asm statement and pads nothing: the two wait states by hand
                else asm volatile("s_nop 1");
                XW_FENCE;
                xw_for<0, 16>([&](auto KC) XW_INL {
                    constexpr int kc = decltype(KC)::value;
                    const int sq = 64 + 16 * q + kc;
                    const unsigned char *A = wbuf + (kc & (XH_RING - 1)) * XH_PIECE + lane16;            // sq & 7 == kc & 7
                    const unsigned char *An = wbuf + ((kc + 1) & (XH_RING - 1)) * XH_PIECE + lane16;
                    constexpr int tb = 2 * kc + 1, tn = (kc < 15 ? 2 * kc + 2 : 0);
                    const unsigned char *dsrc = nullptr;     // this wave's share of piece sq + 7 in the pack (dma_open)
                    auto dma = [&](auto I0) XW_INL {
                        if constexpr (XH_OLD_DMA) dma1(sq + 7, lane16, decltype(I0)::value);
                        else dma_kb(dsrc, lane16, I0);
                    };
                    // k-step t + 1 is produced during k-step t: group 0 in the region of row tiles 0, 1 (tables in tt[0]), group 1 in
                    // the region of row tiles 2, 3 (tt[1]); slot 3 of a region reads the tables of the next region's group
                    // region 0: k-step 2 kc, row tiles 0, 1 (fX) | reads row tiles 2, 3 -> fY | group 0 of k-step tb
                    region_v(acc2[0], acc2[1], fX, b2w[0], fY, A + 4 * XH_FRAG, [&](auto I) XW_INL {
                        constexpr int i = decltype(I)::value;
                        l2_step(I, std::integral_constant<int, tb>{}, std::integral_constant<int, 0>{}, FC, b2w[1], 0);
                        if constexpr (first && i == 3) l2_tab(1, tb, 1);
                        if constexpr (i == 3 && !XH_OLD_DMA) dsrc = dma_open(sq + 7);
                        if constexpr (i == 4) dma(std::integral_constant<int, 0>{});
                    });
                    // region 1: k-step 2 kc, row tiles 2, 3 (fY) | reads tb, row tiles 0, 1 -> fX | group 1 of tb
                    region_v(acc2[2], acc2[3], fY, b2w[0], fX, A + 8 * XH_FRAG, [&](auto I) XW_INL {
                        constexpr int i = decltype(I)::value;
                        l2_step(I, std::integral_constant<int, tb>{}, std::integral_constant<int, 1>{}, FC, b2w[1], 1);
                        if constexpr (first && kc < 15 && i == 3) l2_tab(0, tn, 0);
                        if constexpr (i == 4) dma(std::integral_constant<int, 1>{});
                    });
                    // region 2: k-step tb, row tiles 0, 1 (fX) | reads tb, row tiles 2, 3 -> fY | group 0 of k-step tb + 1
                    region_v(acc2[0], acc2[1], fX, b2w[1], fY, A + 12 * XH_FRAG, [&](auto I) XW_INL {
                        constexpr int i = decltype(I)::value;
                        if constexpr (kc < 15) l2_step(I, std::integral_constant<int, tn>{}, std::integral_constant<int, 0>{}, FC, b2w[0], 0);
                        if constexpr (first && kc < 15 && i == 3) l2_tab(1, tn, 1);
                        if constexpr (i == 4) dma(std::integral_constant<int, 2>{});
                    });
                    // region 3: the last kilobyte of piece sq + 7 | barrier of the next piece | k-step tb, row tiles 2, 3 (fY) | reads
                    // the next piece's first fragments -> fX | group 1 of k-step tb + 1
                    region_v_last(acc2[2], acc2[3], fY, b2w[1], fX, An, [&](auto I) XW_INL {
                        constexpr int i = decltype(I)::value;
                        if constexpr (kc < 15) l2_step(I, std::integral_constant<int, tn>{}, std::integral_constant<int, 1>{}, FC, b2w[0], 1);
                        if constexpr (first && kc < 15 && i == 3) l2_tab(0, tn + 1, 0);
                        if constexpr (i == 1) dma(std::integral_constant<int, 3>{});
                    });
                });
                XH_STAMP(4 + 2 * q)
                // ---- epilogue of hidden layer 2 for rows 128 q .. 128 q + 127 + their share of the 512 -> 3 output layer:
                // acc2[rt] register r <-> unit 128 q + 32 rt + 8 (r >> 2) + 4 h + (r & 3); s_g2 carries the unscale 2^-(4 + s2)
                int le = lane;   // opaque again: the table addresses must not be hoisted above the product loop
                asm volatile("" : "+v"(le));
                const int cq = 128 * q + (le >> 5) * 4;
#pragma unroll
                for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int c = cq + 32 * rt + 8 * rr;
                        const f32x4 gt = ld4(s_g2 + c), hb = ld4(s_hb2 + c);
                        const f32x4 wx3 = ld4(s_w3 + c), wy3 = ld4(s_w3 + XC_H + c), wz3 = ld4(s_w3 + 2 * XC_H + c);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float hv = softplus_fast(fmaf(acc2[rt][4 * rr + r], gt[r], hb[r]));
                            part[0] = fmaf(wx3[r], hv, part[0]);
                            part[1] = fmaf(wy3[r], hv, part[1]);
                            part[2] = fmaf(wz3[r], hv, part[2]);
                        }
                    }
                XW_FENCE;
                XH_STAMP(5 + 2 * q)
            };
            int q0 = 0;
            asm volatile("" : "+s"(q0));     // opaque: the piece addresses of pass 0 are computed like those of passes 1-3 (SALU)
            pass(q0, std::true_type{});
#pragma unroll 1
            for (int q = 1; q < 4; ++q) pass(q, std::false_type{});

            // ---- output ConcatSquash (no softplus: odefunc.py:103): the two halves of a column hold disjoint rows
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                float v = part[d];
                v += __shfl_xor(v, 32);
                const float od = fmaf(v, s_g3[d], s_g3[4 + d]);
                kprev[d] = od;
                kacc[d] = (stage == 0) ? od : ((stage == 3) ? kacc[d] + od : kacc[d] + 2.0f * od);
            }
            XH_STAMP(12)
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) y[d] = y[d] + h6 * kacc[d];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the pieces left in flight by the last stage

    // range guard: the two halves of a column split disjoint units of the same point
    xmax = fmaxf(xmax, __shfl_xor(xmax, 32));
    const bool bad = !(xmax < XH_F16_LIMIT);
    if (cvalid && lane0 < 32) {
        if (bad) atomicOr(a.status, 1u);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            float v = y[d];
            if (a.mbn_out) {
                const float w = a.mbn_out[d], bb = a.mbn_out[3 + d], mean = a.mbn_out[6 + d], var = a.mbn_out[9 + d];
                if (a.reverse) v = (v - bb) * expf(-w) * expf(0.5f * logf(var + 1e-4f)) + mean;
                else v = (v - mean) * expf(-0.5f * logf(var + 1e-4f)) * expf(w) + bb;
            }
            a.y_out[((long)bt * a.n + col) * 3 + d] = bad ? __uint_as_float(0x7fc00000u) : v;
        }
    }
}

// ---- pack: (512, ldw) f32 -> [row quarter 4][k chunk 16][k-step 2][row tile 4][plane 2][lane 64][8 f16] + tail ----------------------
// lane (i = l & 31, h = l >> 5) of fragment (rq, kc, ks, rt) holds row 128 rq + 32 rt + i, k slots s = 0..7 <-> k = 32 kc + 16 ks +
// (s & 3) + 8 (s >> 2) + 4 h (the D-fragment order of the producing layer, as the bf16x6 wide pack)
__global__ void h3_weight_max_kernel(const float *__restrict__ w, int ldw, unsigned *__restrict__ tail)
{
    unsigned m = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < XC_H * XC_H; i += gridDim.x * blockDim.x)
        m = max(m, __float_as_uint(w[(long)(i >> 9) * ldw + (i & 511)]) & 0x7fffffffu);      // |w|: non-negative floats order as their bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0) atomicMax(tail + 1, m);
}
// (h3_shift: f16x3_common.h)
__global__ void pack_weight_cnf_h3_kernel(const float *__restrict__ w, int ldw, unsigned char *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // ((rq * 16 + kc) * 8 + ks * 4 + rt) * 64 + lane
    if (i >= 4 * 16 * 8 * 64) return;
    unsigned *tail = (unsigned *)(out + XH_PACK);
    const int sh = h3_shift(tail[1]);
    if (i == 0) ((int *)tail)[0] = sh;
    const int l = i & 63, fr = (i >> 6) & 7, ck = i >> 9;
    const int rt = fr & 3, ks = fr >> 2, kc = ck & 15, rq = ck >> 4;
    const int row = 128 * rq + 32 * rt + (l & 31), hh = l >> 5;
    float p1[8], p2[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int k = 32 * kc + 16 * ks + (s & 3) + 8 * (s >> 2) + 4 * hh;
        float x = ldexpf(w[(long)row * ldw + k], sh);
        if (fabsf(x) < XH_FLUSH) x = 0.0f;
        p1[s] = (float)(_Float16)x;
        float r = x - p1[s];
        if (fabsf(r) < XH_FLUSH) r = 0.0f;
        p2[s] = r;
    }
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        u32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = pl ? xh_cvt_pk(p2[2 * q], p2[2 * q + 1]) : xh_cvt_pk(p1[2 * q], p1[2 * q + 1]);
        *(u32x4 *)(out + (long)ck * XH_PIECE + ((long)(fr * 2 + pl) * 64 + l) * 16) = v;
    }
}

extern "C" long caspr_cnf_h3_packed_bytes(void) { return XH_PACK + XH_TAIL; }

extern "C" int caspr_pack_weight_cnf_h3(const float *w, int ldw, void *packed, void *stream)
{
    CASPR_REQUIRE(w && packed && ldw >= XC_H, "pack_weight_cnf_h3: bad arguments");
    CASPR_REQUIRE(((uintptr_t)packed % 16) == 0, "pack_weight_cnf_h3: packed must be 16-byte aligned");
    unsigned char *out = (unsigned char *)packed;
    const hipError_t err = hipMemsetAsync(out + XH_PACK, 0, XH_TAIL, (hipStream_t)stream);
    if (err != hipSuccess) {
        caspr_set_error("pack_weight_cnf_h3: hipMemsetAsync failed: %s", hipGetErrorString(err));
        return CASPR_ELAUNCH;
    }
    h3_weight_max_kernel<<<64, 256, 0, (hipStream_t)stream>>>(w, ldw, (unsigned *)(out + XH_PACK));
    pack_weight_cnf_h3_kernel<<<4 * 16 * 8 * 64 / 256, 256, 0, (hipStream_t)stream>>>(w, ldw, out);
    CASPR_CHECK_LAUNCH("pack_weight_cnf_h3");
    return CASPR_OK;
}

#ifdef CASPR_DEBUG_HOOKS
static unsigned long long *g_h3_trace = nullptr;
// 64 words; see XH_STAMP
extern "C" void caspr_debug_set_h3_trace(unsigned long long *dev_buf) { g_h3_trace = dev_buf; }
#endif

// steps_tab / max_steps / order: the per-frame table of caspr_cnf_rk4_h3_frames_f32, NULL / 0 / NULL from the plain entry
static int cnf_rk4_h3_run(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0,
                          const float *b0, const void *w1h, const float *b1, const void *w2h, const float *b2,
                          const float *w3, const float *b3, int H, float t_end, int steps, int reverse,
                          const float *mbn_in, const float *mbn_out, unsigned *status, float *y_out, int BT, int n,
                          const int *steps_tab, int max_steps, const int *order, void *stream)
{
    CASPR_REQUIRE(y_in && hyper && tcol && w0 && b0 && w1h && b1 && w2h && b2 && w3 && b3 && y_out && status, "cnf_rk4_h3: null pointer");
    CASPR_REQUIRE(H == XC_H, "cnf_rk4_h3: hidden width %d unsupported (kernel is built for 512-512-512, flow.py:89)", H);
    CASPR_REQUIRE(BT > 0 && BT <= 65535 && n > 0 && steps > 0 && ldh >= 2 * (3 * H + 3), "cnf_rk4_h3: bad sizes");
    CASPR_REQUIRE(((uintptr_t)w1h % 16) == 0 && ((uintptr_t)w2h % 16) == 0 && ((uintptr_t)w0 % 16) == 0 && ((uintptr_t)w3 % 16) == 0,
                  "cnf_rk4_h3: weights must be 16-byte aligned");
    CnfH3Args a;
    a.y_in = y_in; a.hyper = hyper; a.tcol = tcol; a.w0 = w0; a.b0 = b0; a.b1 = b1; a.b2 = b2; a.w3 = w3; a.b3 = b3;
    a.mbn_in = mbn_in; a.mbn_out = mbn_out; a.w1x = (const unsigned char *)w1h; a.w2x = (const unsigned char *)w2h;
    a.e = nullptr; a.logp_in = nullptr; a.logp_out = nullptr; a.trace = nullptr; a.diag = 0;
    CASPR_IF_DEBUG(a.trace = g_h3_trace;)
    a.y_out = y_out; a.ldh = ldh; a.n = n; a.steps = steps; a.reverse = reverse & 1; a.t_end = t_end;
    a.status = status;
    a.steps_tab = steps_tab; a.max_steps = max_steps; a.order = order;
    static CasprLdsOptIn optin;
    hipError_t err = caspr_lds_opt_in(optin, (const void *)cnf_rk4_h3w_kernel, XH_LDS);
    if (err != hipSuccess) {
        caspr_set_error("cnf_rk4_h3: hipFuncSetAttribute failed: %s", hipGetErrorString(err));
        return CASPR_ELAUNCH;
    }
    err = hipMemsetAsync(status, 0, sizeof(unsigned), (hipStream_t)stream);
    if (err != hipSuccess) {
        caspr_set_error("cnf_rk4_h3: hipMemsetAsync failed: %s", hipGetErrorString(err));
        return CASPR_ELAUNCH;
    }
    cnf_rk4_h3w_kernel<<<dim3(ceil_div(n, XH_PTS), BT), dim3(256), XH_LDS, (hipStream_t)stream>>>(a);
    CASPR_CHECK_LAUNCH("cnf_rk4_h3");
    return CASPR_OK;
}

extern "C" int caspr_cnf_rk4_h3_f32(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0,
                                    const float *b0, const void *w1h, const float *b1, const void *w2h, const float *b2,
                                    const float *w3, const float *b3, int H, float t_end, int steps, int reverse,
                                    const float *mbn_in, const float *mbn_out, unsigned *status, float *y_out, int BT, int n, void *stream)
{
    return cnf_rk4_h3_run(y_in, hyper, ldh, tcol, w0, b0, w1h, b1, w2h, b2, w3, b3, H, t_end, steps, reverse, mbn_in, mbn_out, status, y_out,
                          BT, n, nullptr, 0, nullptr, stream);
}

// the f16x3 sampling solve with a step count per frame (cnf.py:70-128 with logpx = None; flow.py:96-99)
extern "C" int caspr_cnf_rk4_h3_frames_f32(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0,
                                           const float *b0, const void *w1h, const float *b1, const void *w2h, const float *b2,
                                           const float *w3, const float *b3, int H, float t_end, int reverse,
                                           const float *mbn_in, const float *mbn_out, unsigned *status, float *y_out, int BT, int n,
                                           const int *steps_tab, int max_steps, const int *order, void *stream)
{
    CASPR_REQUIRE(steps_tab, "cnf_rk4_h3_frames: null step table");
    CASPR_REQUIRE(max_steps >= 1 && max_steps <= 4096, "cnf_rk4_h3_frames: max_steps %d outside 1..4096", max_steps);
    return cnf_rk4_h3_run(y_in, hyper, ldh, tcol, w0, b0, w1h, b1, w2h, b2, w3, b3, H, t_end, max_steps, reverse, mbn_in, mbn_out, status,
                          y_out, BT, n, steps_tab, max_steps, order, stream);
}
