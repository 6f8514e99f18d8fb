// ode_sample_tape.hip -- the SAMPLING solve of one point-CNF block (cnf.py:70-128 with reverse = True and logpx = None, as
// caspr.py:262 calls it from decode()) as one launch that also writes the tape its gradient needs (train/flow_grad.py:
// CnfSampleSolve): fixed-step RK4 from t_end down to 0, no divergence, and no layer product ever leaves the chip.
//
// The ODE function evaluation is the 64-point sampling evaluation of ode_bf16x6.hip (cnf_rk4_x6_kernel<false>), copied as
// ode_dp5.hip and ode_train_fwd.hip copied theirs: a wave owns 16 points and all 512 hidden units, both hidden layers on the bf16
// matrix pipe (v_mfma_f32_16x16x32_bf16) in the exact three-way split with f32 accumulation, weight pieces by LDS-DMA into a
// double buffer.  What differs is what is written:
//  * besides x(0) every evaluation's point state goes to memory: the stage input (S, 4, BT, n, 3) that the reverse sweep rebuilds
//    ONE evaluation's tape from, and the stage output dy/dt (S, 4, BT, n, 3) that the gradient with respect to the step size needs.
//    12 + 12 bytes per point and evaluation: the only thing that grows with S;
//  * the end time is read from device memory (the differentiable route holds sqrt_end_time^2 as a tensor: no host read-back);
//  * no MovingBatchNorm at either end (autograd keeps those), reverse direction only.
// Every store is a plain vector store by the lane that owns the value; no atomics; a point's result depends on its frame's gates
// and its own column only, never on the batch around it.  The columns of a partial workgroup (n % 64 != 0) read the frame's last
// point and write nothing.
#include "ode_x6.h"

#define XC_COLS 64
#define XC_PA (256 * 64)          // one plane of a piece
#define XC_PIECE (3 * XC_PA)      // 48 KB: 256 rows x 32 k x 3 planes
#define XC_NPIECE 32              // per layer: 16 k chunks x 2 row halves
#define XC_RING 2                 // LDS double buffer of pieces
#define XC_LDS (XC_RING * XC_PIECE + (6 * XC_H + 3 * XC_H + 3 * XC_H + 8) * 4)

struct CnfSampleTapeArgs {
    const float *y_in, *hyper, *tcol, *w0, *b0, *b1, *b2, *w3, *b3;
    const float *t_end;           // one float in device memory
    const unsigned char *w1x, *w2x;
    float *y_out;                 // (BT,n,3)
    float *ys, *ka;               // [steps][4][BT][n][3] stage inputs, stage outputs
    int ldh, n, steps;
};

__global__ __launch_bounds__(256, 1) void cnf_sample_tape_kernel(CnfSampleTapeArgs a)
{
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    unsigned char *wbuf = lds;                                  // [XC_RING][XC_PIECE]
    float *s_gate = (float *)(lds + XC_RING * XC_PIECE);              // [3][512] sigmoid gates of layers 0,1,2
    float *s_hb = s_gate + 3 * XC_H;                            // [3][512] layer bias * gate + hyper bias
    float *s_w0 = s_hb + 3 * XC_H;                              // [512][3]
    float *s_w3 = s_w0 + 3 * XC_H;                              // [3][512] output layer
    float *s_g3 = s_w3 + 3 * XC_H;                              // [8]: gate3[3], hb3[3]

    const int tid = threadIdx.x, lane0 = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g0 = lane0 >> 4;
    const int bt = blockIdx.y;
    // a wave's 16 columns are 16 points; the workgroup owns 64 points of frame bt
    const int col = blockIdx.x * XC_COLS + 16 * wave + (lane0 & 15);
    const bool cvalid = col < a.n;
    const int ccol = cvalid ? col : a.n - 1;
    const float *hy = a.hyper + (long)bt * a.ldh;
    constexpr int GOFF = 0, BOFF = 3 * XC_H + 3;
    const int sd = g0 < 3 ? g0 : 0;   // state component of this lane (lanes g == 3 carry a copy of component 0, never stored)

    for (int i = tid; i < 3 * XC_H; i += 256) {
        s_w0[i] = a.w0[i];
        s_w3[i] = a.w3[i];
    }

    float y = a.y_in[((long)bt * a.n + ccol) * 3 + sd], kacc = 0.f, kprev = 0.f;

    // LDS-DMA of piece p (k chunk p >> 1, row half p & 1) of a layer's pack [row half][k chunk][48 KB image] into
    // buffer p & 1: scalar base + one 32-bit lane offset (anything lane-dependent that is hoisted out of the stage
    // loop ends up in scratch).  12 wave-instructions of 1 KB per wave, issued in three parts.
    auto dma = [&](const unsigned char *wx, int p, int lane16, int s0 = 0, int s1 = 12) {
        const unsigned char *src = wx + (long)((p & 1) * 16 + (p >> 1)) * XC_PIECE + (wave * 12) * 1024;
#pragma unroll
        for (int s = s0; s < s1; ++s)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + s * 1024 + lane16),
                                             (__attribute__((address_space(3))) void *)(wbuf + (p & 1) * XC_PIECE + (wave * 12 + s) * 1024), 16, 0, 0);
    };
    // reversed time axis: from t_end down to 0 (cnf.py:92-93 flips the integration times), h < 0
    const double t0 = (double)a.t_end[0];
    const double h = (0.0 - t0) / (double)a.steps;
    const float hh = (float)h, h2 = (float)(0.5 * h), h6 = (float)(h / 6.0);

    // the first piece of layer 1; every layer pass leaves the NEXT pass's first piece in flight
    dma(a.w1x, 0, lane0 * 16);

    // The B fragments of a layer input are PRODUCED WHILE THE LAYER RUNS: the pieces go k-chunk-major, so chunk kc+1's three
    // planes (12 registers) are only needed when chunk kc's two pieces are done -- its input-layer values (layer 1) or its
    // slice of layer 1's epilogue (layer 2: gate * acc + bias, softplus, split) are computed in quarters inside the
    // MFMA runs of chunk kc, where the VALU work hides behind the matrix pipe.  Two accumulator sets (layer 1's is
    // consumed chunk by chunk while layer 2 fills its own) instead of 192 fragment registers.
    f32x4 acc1[32], acc2[32];
    u32x4 bkw[2][3];              // B-fragment planes of the current / next k chunk, by chunk parity
    f32x4 tg_, tb, tw[3];         // table values of the half chunk being produced (gate, bias, input-layer weights)

    for (int step = 0; step < a.steps; ++step) {
#pragma unroll 1
        for (int stage = 0; stage < 4; ++stage) {
            const double tc = (stage == 0) ? 0.0 : (stage == 3 ? 1.0 : 0.5);
            const float t = (float)(t0 + (double)step * h + tc * h);
            const float aw = (stage == 0) ? 0.f : (stage == 3 ? hh : h2);
            // Opaque copy of the lane id: everything derived from it (LDS offsets, DMA offsets, table addresses) is
            // recomputed per stage instead of being hoisted out of the 32-stage loop and spilled (as in ode.hip).
            int lane = lane0;
            asm volatile("" : "+v"(lane));
            const int g = lane >> 4, j = lane & 15, lane16 = lane * 16;
            // A-fragment read offset inside a plane: row (lane & 15) of a 16-row tile, piece g, swizzled as the pack
            const int aoff = j * 64 + ((g ^ ((0 - (j >> 2)) & 3)) << 4);
            __syncthreads();   // the previous stage's epilogues are done with the gate tables
            for (int i = tid; i < 3 * XC_H; i += 256) {
                const float gt = sigmoid_fast(hy[GOFF + i] + t * a.tcol[GOFF + i]);
                const float hb = hy[BOFF + i] + t * a.tcol[BOFF + i];
                const float bl = i < XC_H ? a.b0[i] : (i < 2 * XC_H ? a.b1[i - XC_H] : a.b2[i - 2 * XC_H]);
                s_gate[i] = gt;
                s_hb[i] = bl * gt + hb;
            }
            if (tid < 3) {
                const float gt = sigmoid_fast(hy[GOFF + 3 * XC_H + tid] + t * a.tcol[GOFF + 3 * XC_H + tid]);
                const float hb = hy[BOFF + 3 * XC_H + tid] + t * a.tcol[BOFF + 3 * XC_H + tid];
                s_g3[tid] = gt;
                s_g3[4 + tid] = a.b3[tid] * gt + hb;
            }
            __syncthreads();

            // ---- stage input of this lane's column, all three components
            const float ystage = (stage == 0) ? y : y + aw * kprev;
            const float y0 = __shfl(ystage, j), y1 = __shfl(ystage, 16 + j), y2 = __shfl(ystage, 32 + j);

            // ---- producers of B fragments, a quarter (two k-slots) at a time; the tables of a half chunk one region earlier
            auto put_pair = [&](int kc, int q, float v0, float v1) __attribute__((always_inline)) {
                unsigned p1, p2, p3;
                xc_split_pair(v0, v1, p1, p2, p3);
                bkw[kc & 1][0][q] = p1;
                bkw[kc & 1][1][q] = p2;
                bkw[kc & 1][2][q] = p3;
            };
            // input layer 3 -> 512 (diffeq_layers.py:83-90 + softplus): slots 2q, 2q+1 of chunk kc = units 32kc + 16h + 4g + r
            auto tab_in = [&](int kc, int hf) __attribute__((always_inline)) {
                const int c = 32 * kc + 16 * hf + 4 * g;
                tg_ = ld4(s_gate + c);
                tb = ld4(s_hb + c);
                tw[0] = ld4(s_w0 + 3 * c);
                tw[1] = ld4(s_w0 + 3 * c + 4);
                tw[2] = ld4(s_w0 + 3 * c + 8);
            };
            auto quad_in = [&](int kc, int q) __attribute__((always_inline)) {
                const float w[12] = {tw[0][0], tw[0][1], tw[0][2], tw[0][3], tw[1][0], tw[1][1], tw[1][2], tw[1][3], tw[2][0], tw[2][1], tw[2][2], tw[2][3]};
                float v[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int r = 2 * (q & 1) + e;
                    const float pre = (w[3 * r] * y0 + w[3 * r + 1] * y1 + w[3 * r + 2] * y2) * tg_[r] + tb[r];
                    v[e] = softplus_fast(pre);
                }
                put_pair(kc, q, v[0], v[1]);
            };
            // epilogue of hidden layer 1 for chunk kc of layer 2: units 32kc + 16h + 4g + r = rows of acc1[2kc + h]
            auto tab_e1 = [&](int kc, int hf) __attribute__((always_inline)) {
                const int c = 32 * kc + 16 * hf + 4 * g;
                tg_ = ld4(s_gate + XC_H + c);
                tb = ld4(s_hb + XC_H + c);
            };
            auto quad_e1 = [&](int kc, int q) __attribute__((always_inline)) {
                float v[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int r = 2 * (q & 1) + e;
                    v[e] = softplus_fast(acc1[2 * kc + (q >> 1)][r] * tg_[r] + tb[r]);
                }
                put_pair(kc, q, v[0], v[1]);
            };

            // 4 / 20 MFMAs of four row tiles: smallest terms first; term-major, i.e. four independent accumulators between
            // dependent MFMAs
            auto mma_head = [&](f32x4 (&acc)[32], const bf16x8 (&af)[4][3], const u32x4 (&b)[3], int m0) __attribute__((always_inline)) {
                const bf16x8 b0 = __builtin_bit_cast(bf16x8, b[0]);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[m0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u][2], b0, acc[m0 + u], 0, 0, 0);
            };
            auto mma_tail = [&](f32x4 (&acc)[32], const bf16x8 (&af)[4][3], const u32x4 (&b)[3], int m0) __attribute__((always_inline)) {
                const bf16x8 b0 = __builtin_bit_cast(bf16x8, b[0]), b1 = __builtin_bit_cast(bf16x8, b[1]), b2 = __builtin_bit_cast(bf16x8, b[2]);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[m0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u][1], b1, acc[m0 + u], 0, 0, 0);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[m0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u][0], b2, acc[m0 + u], 0, 0, 0);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[m0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u][1], b0, acc[m0 + u], 0, 0, 0);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[m0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u][0], b1, acc[m0 + u], 0, 0, 0);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[m0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u][0], b0, acc[m0 + u], 0, 0, 0);
            };

            // One layer pass.  A piece (48 KB, k chunk p >> 1, row half p & 1) is four groups of four row tiles (24 MFMAs each),
            // read into two fragment sets alternately and skewed by one group: a scheduling region = the 12 reads of group
            // G+1, interleaved two per MFMA with the first MFMAs of the 20 that remain of group G ("tail"), then the first
            // four MFMAs of group G+1 ("head") -- hipcc waits with lgkmcnt(0), never a counted wait, before the first use of
            // a set, and at the head that wait is free.  Six of the eight regions of a k chunk also carry a quarter of the
            // next chunk's B fragments (VALU) or the table reads for it.  sched_group_barrier builds the patterns,
            // sched_barrier(0) closes a region (hipcc otherwise sinks every read to just before its use).  The last group of
            // piece p-1 finishes after the barrier of piece p.
#define XC_SGB(mask, n) __builtin_amdgcn_sched_group_barrier(mask, n, 0);
#define XC_RM6 XC_SGB(0x100, 2) XC_SGB(0x008, 1) XC_SGB(0x100, 2) XC_SGB(0x008, 1) XC_SGB(0x100, 2) XC_SGB(0x008, 1) XC_SGB(0x100, 2) \
    XC_SGB(0x008, 1) XC_SGB(0x100, 2) XC_SGB(0x008, 1) XC_SGB(0x100, 2) XC_SGB(0x008, 1)
#define XC_VM4 XC_SGB(0x002, 2) XC_SGB(0x008, 1) XC_SGB(0x002, 2) XC_SGB(0x008, 1) XC_SGB(0x002, 2) XC_SGB(0x008, 1) XC_SGB(0x002, 2) XC_SGB(0x008, 1)
#define XC_REGION_PLAIN XC_RM6 XC_SGB(0x008, 18) __builtin_amdgcn_sched_barrier(0);
#define XC_REGION_TAB XC_RM6 XC_SGB(0x100, 5) XC_SGB(0x008, 18) __builtin_amdgcn_sched_barrier(0);
#define XC_REGION_VALU XC_RM6 XC_VM4 XC_VM4 XC_VM4 XC_VM4 XC_SGB(0x002, 2) XC_SGB(0x008, 2) __builtin_amdgcn_sched_barrier(0);
            auto layer = [&](const unsigned char *wx, const unsigned char *wnext, f32x4 (&acc)[32], auto tab, auto quad) __attribute__((always_inline)) {
#pragma unroll
                for (int mi = 0; mi < 32; ++mi) acc[mi] = (f32x4){0.f, 0.f, 0.f, 0.f};
                bf16x8 af0[4][3], af1[4][3];
                auto rd = [&](bf16x8 (&af)[4][3], const unsigned char *A, int G) __attribute__((always_inline)) {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int pl = 0; pl < 3; ++pl) af[u][pl] = *(const bf16x8 *)(A + pl * XC_PA + (4 * G + u) * 1024);
                };
#pragma unroll
                for (int p = 0; p < XC_NPIECE; ++p) {
                    // piece p (its DMA was issued one piece ago) has landed once nothing is outstanding; lgkmcnt: this wave's
                    // reads of the buffer about to be refilled.  Raw barrier: no compiler-added waits.
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();   // piece p is there for every wave; everybody is done with buffer (p + 1) & 1
                    asm volatile("" ::: "memory");
                    const int kc = p >> 1, mt = p & 1;
                    const int kcp = (p - 1) >> 1, mtp = (p - 1) & 1;
                    const bool more = kc + 1 < 16;   // a next chunk to produce
                    const unsigned char *wq = p + 1 < XC_NPIECE ? wx : wnext;
                    const int pn = p + 1 < XC_NPIECE ? p + 1 : 0;
                    const unsigned char *A = wbuf + (p & 1) * XC_PIECE + aoff;
                    // region 0: read group 0 | the rest of the previous piece's group 3 | first MFMAs of group 0
                    __builtin_amdgcn_sched_barrier(0);
                    rd(af0, A, 0);
                    dma(wq, pn, lane16, 0, 4);
                    if (p > 0) mma_tail(acc, af1, bkw[kcp & 1], 16 * mtp + 12);
                    mma_head(acc, af0, bkw[kc & 1], 16 * mt);
                    if (more && mt == 0) {
                        tab(kc + 1, 0);
                        XC_REGION_TAB
                    } else if (more) {
                        quad(kc + 1, 2);
                        XC_REGION_VALU
                    } else {
                        XC_REGION_PLAIN
                    }
                    // region 1
                    rd(af1, A, 1);
                    dma(wq, pn, lane16, 4, 8);
                    mma_tail(acc, af0, bkw[kc & 1], 16 * mt);
                    mma_head(acc, af1, bkw[kc & 1], 16 * mt + 4);
                    if (more) {
                        quad(kc + 1, mt == 0 ? 0 : 3);
                        XC_REGION_VALU
                    } else {
                        XC_REGION_PLAIN
                    }
                    // region 2
                    rd(af0, A, 2);
                    dma(wq, pn, lane16, 8, 12);
                    mma_tail(acc, af1, bkw[kc & 1], 16 * mt + 4);
                    mma_head(acc, af0, bkw[kc & 1], 16 * mt + 8);
                    if (more && mt == 0) {
                        quad(kc + 1, 1);
                        XC_REGION_VALU
                    } else {
                        XC_REGION_PLAIN
                    }
                    // region 3
                    rd(af1, A, 3);
                    mma_tail(acc, af0, bkw[kc & 1], 16 * mt + 8);
                    mma_head(acc, af1, bkw[kc & 1], 16 * mt + 12);
                    if (more && mt == 0) {
                        tab(kc + 1, 1);
                        XC_REGION_TAB
                    } else {
                        XC_REGION_PLAIN
                    }
                }
                mma_tail(acc, af1, bkw[((XC_NPIECE - 1) >> 1) & 1], 16 * ((XC_NPIECE - 1) & 1) + 12);
            };

            float part[3] = {0.f, 0.f, 0.f};
            {
                // chunk 0 of layer 1 up front (exposed: 1/16 of the input layer)
                tab_in(0, 0);
                quad_in(0, 0);
                quad_in(0, 1);
                tab_in(0, 1);
                quad_in(0, 2);
                quad_in(0, 3);
                layer(a.w1x, a.w2x, acc1, tab_in, quad_in);
                // chunk 0 of layer 2
                tab_e1(0, 0);
                quad_e1(0, 0);
                quad_e1(0, 1);
                tab_e1(0, 1);
                quad_e1(0, 2);
                quad_e1(0, 3);
                layer(a.w2x, a.w1x, acc2, tab_e1, quad_e1);
            }
            {
                // ---- epilogue of hidden layer 2 + the 512 -> 3 output layer as a per-lane partial dot product (tables one
                // row tile ahead)
                int le = lane;   // opaque again: the table addresses must not be hoisted above the product loop
                asm volatile("" : "+v"(le));
                const int ge = le >> 4;
                f32x4 tq[2][5];
                auto ld_e2 = [&](int set, int mi) __attribute__((always_inline)) {
                    const int c = 16 * mi + 4 * ge;
                    tq[set][0] = ld4(s_gate + 2 * XC_H + c);
                    tq[set][1] = ld4(s_hb + 2 * XC_H + c);
                    tq[set][2] = ld4(s_w3 + c);
                    tq[set][3] = ld4(s_w3 + XC_H + c);
                    tq[set][4] = ld4(s_w3 + 2 * XC_H + c);
                };
                ld_e2(0, 0);
#pragma unroll
                for (int mi = 0; mi < 32; ++mi) {
                    if (mi + 1 < 32) ld_e2((mi + 1) & 1, mi + 1);
                    __builtin_amdgcn_sched_barrier(0);
                    const f32x4 gt = tq[mi & 1][0], hb = tq[mi & 1][1], wx3 = tq[mi & 1][2], wy3 = tq[mi & 1][3], wz3 = tq[mi & 1][4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float hv = softplus_fast(acc2[mi][r] * gt[r] + hb[r]);
                        part[0] += wx3[r] * hv;
                        part[1] += wy3[r] * hv;
                        part[2] += wz3[r] * hv;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // ---- output ConcatSquash (no softplus: odefunc.py:103): sum the four lane groups, every lane gets all three
            float o[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                float v = part[d];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                o[d] = v * s_g3[d] + s_g3[4 + d];
            }
            const float od = sd == 0 ? o[0] : (sd == 1 ? o[1] : o[2]);
            kprev = od;
            kacc = (stage == 0) ? od : ((stage == 3) ? kacc + od : kacc + 2.0f * od);
            // ---- what the reverse sweep needs of this evaluation: its input and its output, by the lanes that own them
            // (lane (g, j), g < 3, owns component g of point j; the columns past n and the copies in g == 3 write nothing)
            const int colx = blockIdx.x * XC_COLS + 16 * wave + j;
            if (g < 3 && colx < a.n) {
                const long ev = (((long)(step * 4 + stage) * gridDim.y + bt) * a.n + colx) * 3 + g;
                a.ys[ev] = ystage;
                a.ka[ev] = od;
            }
        }
        y = y + h6 * kacc;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the prefetch left in flight by the last layer pass

    if (cvalid && g0 < 3) a.y_out[((long)bt * a.n + col) * 3 + sd] = y;
}

// cnf.py:70-128 (reverse = True, logpx = None) as caspr.py:262 runs it in decode(), with the tape of train/flow_grad.py: CnfSampleSolve
extern "C" int caspr_cnf_sample_tape_f32(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0, const float *b0,
                                         const void *w1x, const float *b1, const void *w2x, const float *b2, const float *w3, const float *b3,
                                         int H, const float *t_end, int steps, float *y_out, float *ys, float *ka, int BT, int n, void *stream)
{
    CASPR_REQUIRE(y_in && hyper && tcol && w0 && b0 && w1x && b1 && w2x && b2 && w3 && b3 && t_end && y_out && ys && ka, "cnf_sample_tape: null pointer");
    CASPR_REQUIRE(H == XC_H, "cnf_sample_tape: hidden width %d unsupported (kernel is built for 512-512-512, flow.py:89)", H);
    CASPR_REQUIRE(BT > 0 && BT <= 65535 && n > 0 && steps > 0 && steps <= (1 << 20) && ldh >= 2 * (3 * H + 3), "cnf_sample_tape: bad sizes");
    CASPR_REQUIRE(((uintptr_t)w1x % 16) == 0 && ((uintptr_t)w2x % 16) == 0 && ((uintptr_t)w0 % 16) == 0 && ((uintptr_t)w3 % 16) == 0,
                  "cnf_sample_tape: weights must be 16-byte aligned");
    CnfSampleTapeArgs a;
    a.y_in = y_in; a.hyper = hyper; a.tcol = tcol; a.w0 = w0; a.b0 = b0; a.b1 = b1; a.b2 = b2; a.w3 = w3; a.b3 = b3;
    a.t_end = t_end; a.w1x = (const unsigned char *)w1x; a.w2x = (const unsigned char *)w2x;
    a.y_out = y_out; a.ys = ys; a.ka = ka;
    a.ldh = ldh; a.n = n; a.steps = steps;
    static CasprLdsOptIn optin;
    const hipError_t err = caspr_lds_opt_in(optin, (const void *)cnf_sample_tape_kernel, XC_LDS);
    if (err != hipSuccess) {
        caspr_set_error("cnf_sample_tape: hipFuncSetAttribute failed: %s", hipGetErrorString(err));
        return CASPR_ELAUNCH;
    }
    cnf_sample_tape_kernel<<<dim3(ceil_div(n, XC_COLS), BT), dim3(256), XC_LDS, (hipStream_t)stream>>>(a);
    CASPR_CHECK_LAUNCH("cnf_sample_tape");
    return CASPR_OK;
}
