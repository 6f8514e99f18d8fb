// ode_dp5_f16x3w.hip -- the point-CNF SAMPLING solve integrated to a TOLERANCE (adaptive Dormand-Prince 5(4), error control per frame)
// on THREE f16 products per f32 product (config.cnf_dp5_split = "f16x3"): the launch protocol of ode_dp5.hip around the evaluation of
// ode_f16x3w.hip.  Both are copied on purpose (as ode_dp5.hip copies the 64-point body); read their headers first, this one lists
// what is particular to the combination.
//
//  * evaluation: cnf_rk4_h3w_kernel's stage body, unchanged -- 128 points per workgroup, a wave owns 32 points and all 512 units, layer
//    1's 256 accumulators in the hand-managed accumulator file (the f16 planes kept there during layer 2), the 8-deep LDS-DMA weight
//    ring with vmcnt(24) piece barriers, the 2^4 activation scale and the weight shifts behind the pack_cnf_h3 packs, the explicit
//    subnormal flush, v_max3_f32 range tracking.  The stage loop is `#pragma unroll 1` with ONE copy of the body: the accumulator-move
//    and MFMA counts are those of the RK4 kernel (audit.audit_cnf_dp5_h3w).  The piece sequence keeps running across the stages of a
//    launch (128 pieces a stage, a multiple of the ring: the last pieces of a stage prefetch the first of the next).  The INSTRUCTION
//    STREAM has since diverged (same values, same bits): the RK4 kernel now flushes on the f16 word (xh_flush_word) and writes M0 and
//    the source address once per piece; this copy keeps the f32 compare-and-select flush and one M0 write per LDS-DMA instruction
//    (audit_cnf_dp5_h3w still asks for that).  Bringing both over needs this kernel's register budget rechecked (.vgpr_count 488 of
//    512; the word flush holds one more VGPR) and was not timed;
//  * loop: cnf_dp5_kernel<false>'s -- one launch per attempt; launch 0 evaluates f(t0, y0), launch 1 f(t0 + h0, y0 + h0 f0), launch
//    L >= 2 decides attempt L - 3 and runs the six stages of attempt L - 2; a workgroup writes its f64 partial sums of squares to ITS slot
//    (double-buffered by launch parity), the next launch's prologue adds a frame's slots in slot order: every workgroup of the frame
//    takes the identical decision, nobody waits on anybody, no float atomics.  Controller state, tableau, trace and counters as there;
//  * grid (ceil(n / 128), BT): a frame has ceil(n / 128) slots.  Lanes l and l + 32 of a wave hold disjoint hidden units of the SAME
//    point: both carry its state, the lower one owns it (norms, carry-over, output); columns past n repeat the last point and own nothing;
//  * the state is x only (no divergence on this route): three floats per lane, k1..k7 of all three in registers (21 floats; the kernel
//    compiles without scratch -- the audit refuses a build that spills), tableau rows in constant memory;
//  * per-point carry-over between launches (y, f0, y_new, k7, y_mid: 15 floats) in the workspace;
//  * RANGE GUARD: a point whose scaled activation is not below 65520 would poison its frame's norm.  Its owner sets bit 1 of the status
//    word and counts it in the slot's second sum; the next launch finds the count positive in every workgroup of the frame, writes NaN
//    to all of the frame's outputs and retires it (counters[3] = 3: finished | guard; the undecided attempt is traced as rejected with
//    a NaN ratio).  The other frames never see it.  ops.check_deferred_errors reports it and names cnf_dp5_split = "bf16x6".
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

// ---- Dormand-Prince 5(4), Shampine's variant as torchdiffeq 0.0.1 dopri5.py: the tables of ode_dp5.hip.  Rows 0 and 1 are the two
// evaluations of the initial-step selection (y0 itself; y0 + h0 f0), rows 2..7 the six new stages of an attempt (the last: y_new, FSAL).
__constant__ float DPH_BETA[8][6] = {
    {0.f, 0.f, 0.f, 0.f, 0.f, 0.f},
    {1.f, 0.f, 0.f, 0.f, 0.f, 0.f},
    {(float)(1.0 / 5), 0.f, 0.f, 0.f, 0.f, 0.f},
    {(float)(3.0 / 40), (float)(9.0 / 40), 0.f, 0.f, 0.f, 0.f},
    {(float)(44.0 / 45), (float)(-56.0 / 15), (float)(32.0 / 9), 0.f, 0.f, 0.f},
    {(float)(19372.0 / 6561), (float)(-25360.0 / 2187), (float)(64448.0 / 6561), (float)(-212.0 / 729), 0.f, 0.f},
    {(float)(9017.0 / 3168), (float)(-355.0 / 33), (float)(46732.0 / 5247), (float)(49.0 / 176), (float)(-5103.0 / 18656), 0.f},
    {(float)(35.0 / 384), 0.f, (float)(500.0 / 1113), (float)(125.0 / 192), (float)(-2187.0 / 6784), (float)(11.0 / 84)},
};
__constant__ double DPH_ALPHA[8] = {0.0, 1.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
__constant__ float DPH_CERR[7] = {(float)(35.0 / 384 - 1951.0 / 21600), 0.f, (float)(500.0 / 1113 - 22642.0 / 50085), (float)(125.0 / 192 - 451.0 / 720),
                                  (float)(-2187.0 / 6784 - -12231.0 / 42400), (float)(11.0 / 84 - 649.0 / 6300), (float)(-1.0 / 60.0)};
__constant__ float DPH_CMID[7] = {(float)(6025192743.0 / 30085553152.0 / 2), 0.f, (float)(51252292925.0 / 65400821598.0 / 2),
                                  (float)(-2691868925.0 / 45128329728.0 / 2), (float)(187940372067.0 / 1594534317056.0 / 2),
                                  (float)(-1776094331.0 / 19743644256.0 / 2), (float)(11237099.0 / 235043384.0 / 2)};
#define DPH_SAFETY 0.9f
#define DPH_IFACTOR 10.0f
#define DPH_DFACTOR 0.2f

#define DPH_TRACE_HEAD 8     // floats per frame before the attempt rows: d0, d1, d2, h0, first dt, 0, 0, 0
#define DPH_TRACE_ROW 5      // per attempt: t, dt, ratio of x, 0 (the ratio of logp on the other route), accepted (1 / 0)
#define DPH_LDS (XH_LDS + 16 * 8)
#define DPH_GUARD 2u         // the status word's bit of this kernel (cnf_rk4_h3w_kernel sets bit 0)
// carry-over quantities of a point, each [3 components][n]
#define DPH_Y 0
#define DPH_F0 1
#define DPH_YN 2
#define DPH_K7 3
#define DPH_YM 4

struct Dp5H3Frame {          // a frame's controller state (Dp5Frame of ode_dp5.hip), written by its first workgroup, double-buffered by launch parity
    double t;                // solver time (negated when the solve runs in reverse, as upstream)
    float dt, h0, d0, d1, d2, dt0;
    int done, nacc, nrej, nfe;
    int pad[2];
};

struct CnfDp5H3Args {
    const float *y_in, *hyper, *tcol, *w0, *b0, *b1, *b2, *w3, *b3, *mbn_in, *mbn_out;
    const unsigned char *w1x, *w2x;   // the pack_cnf_h3 packs
    float *y_out;
    int ldh, n, reverse;
    float t_end, rtol, atol;
    int launch;                   // 0: f(t0, y0); 1: f(t0 + h0, y0 + h0 f0); L >= 2: decide attempt L - 3, run attempt L - 2
    int last;                     // the attempt budget is used up: decide only
    int max_attempts;
    Dp5H3Frame *frames;           // [2][BT]
    double *part;                 // [2][BT][workgroups of a frame][4]: sum of squares, points the range guard caught, second sum (launch 0), 0
    float *pts;                   // [BT][5][3][n]
    int *running;                 // [launch]: frames that did not retire in that launch
    float *trace;                 // [BT][DPH_TRACE_HEAD + DPH_TRACE_ROW * max_attempts]
    int *counters;                // [BT][4]: accepted, rejected, evaluations, finished (1; 3: retired by the range guard)
    unsigned *status;             // one word per solve, zeroed in front of launch 0: DPH_GUARD set <-> the range guard tripped
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
__device__ __forceinline__ void xh_split1(XwPair &p)  // first plane (flushed) + remainder; X >= 0 here
{
    const float a0 = p.x0 < XH_FLUSH ? 0.0f : p.x0, a1 = p.x1 < XH_FLUSH ? 0.0f : p.x1;
    p.p1 = xh_cvt_pk(a0, a1);
    const xh_f16x2 hv = __builtin_bit_cast(xh_f16x2, p.p1);
    p.r0 = a0 - (float)hv[0];
    p.r1 = a1 - (float)hv[1];
}
__device__ __forceinline__ void xh_split2(XwPair &p, u32x4 (&bw)[2], int q)
{
    const float r0 = fabsf(p.r0) < XH_FLUSH ? 0.0f : p.r0, r1 = fabsf(p.r1) < XH_FLUSH ? 0.0f : p.r1;
    bw[0][q] = p.p1;
    bw[1][q] = xh_cvt_pk(r0, r1);
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

__global__ __launch_bounds__(256, 1) void cnf_dp5_h3w_kernel(CnfDp5H3Args a)
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
    double *s_red = (double *)(s_g3 + 8);           // [4 waves][4] partial sums

    const int tid = threadIdx.x, lane0 = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bt = blockIdx.y, BT = gridDim.y, nwg = gridDim.x;
    const int col = blockIdx.x * XH_PTS + 32 * wave + (lane0 & 31);
    const bool cvalid = col < a.n;
    const int ccol = cvalid ? col : a.n - 1;
    // lanes l and l + 32 hold the same point: the lower one owns it (counts it in the norms, stores its carry-over and its output)
    const bool own = cvalid && lane0 < 32;
    float *pp = a.pts + (long)bt * 15 * a.n + ccol;             // quantity q, component d at pp[q * qs + d * n]
    const long qs = 3L * a.n;

    const int Lc = a.launch, par = Lc & 1;
    const Dp5H3Frame *fprev = a.frames + (long)(par ^ 1) * BT + bt;
    Dp5H3Frame *fnext = a.frames + (long)par * BT + bt;
    const bool lead = blockIdx.x == 0 && tid == 0;
    const double sgn = a.reverse ? -1.0 : 1.0;
    const double tq1 = a.reverse ? 0.0 : (double)a.t_end;       // where the solve ends, in solver time
    Dp5H3Frame st;
    if (Lc > 0) {
        st = *fprev;
        if (st.done) {                                          // retired: carry the state over and leave
            if (lead) *fnext = st;
            return;
        }
    } else {
        st.t = a.reverse ? -(double)a.t_end : 0.0;
        st.dt = st.h0 = st.d0 = st.d1 = st.d2 = st.dt0 = 0.f;
        st.done = st.nacc = st.nrej = st.nfe = 0;
        st.pad[0] = st.pad[1] = 0;
    }

    float s[3], f0[3] = {0.f, 0.f, 0.f};
    if (Lc == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            float v = a.y_in[((long)bt * a.n + ccol) * 3 + d];
            if (a.mbn_in) {
                const float w = a.mbn_in[d], bb = a.mbn_in[3 + d], mean = a.mbn_in[6 + d], var = a.mbn_in[9 + d];
                if (a.reverse) v = (v - bb) * expf(-w) * expf(0.5f * logf(var + 1e-4f)) + mean;   // normalization.py:92-94
                else v = (v - mean) * expf(-0.5f * logf(var + 1e-4f)) * expf(w) + bb;             // normalization.py:70-74
            }
            s[d] = v;
        }
    } else {
        // (A lane that does not own its point -- the upper half of a wave, a column past n clamped to point n - 1 -- may read these two
        // AFTER the point's owner, possibly in another wave, has committed the accepted step to them further down.  Harmless, and only
        // because of what follows: y and f0 matter after a REJECTED attempt, when nobody writes them, or at the interpolant, which the
        // owner alone computes; on accept every lane replaces them by y_new and k7, which this launch only reads.)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            s[d] = pp[DPH_Y * qs + (long)d * a.n];
            f0[d] = pp[DPH_F0 * qs + (long)d * a.n];
        }
    }

    // ---- the frame's sums of the previous launch: its workgroups' slots added in slot order, the same in every workgroup of the frame
    double S[4] = {0.0, 0.0, 0.0, 0.0};
    if (Lc > 0) {
        const double *p = a.part + ((long)(par ^ 1) * BT + bt) * nwg * 4;
        for (int w = 0; w < nwg; ++w)
#pragma unroll
            for (int q = 0; q < 4; ++q) S[q] += p[4 * w + q];
    }
    const double nx = 3.0 * (double)a.n;
    float *trow = a.trace + (long)bt * (DPH_TRACE_HEAD + DPH_TRACE_ROW * a.max_attempts);
    float dt = st.dt, hstep = 0.f;
    if (S[1] > 0.0) {
        // ---- the range guard caught a point of this frame in the previous launch: NaN in all of the frame's outputs, the frame retires
        // (every workgroup of the frame reads the same count; the status word was set by the point's owner)
        if (own) {
#pragma unroll
            for (int d = 0; d < 3; ++d) a.y_out[((long)bt * a.n + col) * 3 + d] = __uint_as_float(0x7fc00000u);
        }
        if (lead) {
            if (Lc >= 3) {                                      // the attempt that was to be decided: traced as rejected, ratio NaN
                float *tr = trow + DPH_TRACE_HEAD + DPH_TRACE_ROW * (Lc - 3);
                tr[0] = (float)(sgn * st.t); tr[1] = dt; tr[2] = __uint_as_float(0x7fc00000u); tr[3] = 0.f; tr[4] = 0.f;
                ++st.nrej;
            }
            st.done = 1;
            *fnext = st;
            int *c = a.counters + 4 * bt;
            c[0] = st.nacc; c[1] = st.nrej; c[2] = st.nfe; c[3] = 3;
        }
        return;
    }
    if (Lc == 1) {
        // _select_initial_step: d0 = rms(y / scale), d1 = rms(f0 / scale)
        const double d0 = sqrt(S[0] / nx), d1 = sqrt(S[2] / nx);
        const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * (d0 / fmax(d1, 1e-300));
        st.d0 = (float)d0;
        st.d1 = (float)d1;
        st.h0 = (float)h0;
        hstep = st.h0;
    } else if (Lc == 2) {
        const float d2 = (float)(sqrt(S[0] / nx) / (double)st.h0);
        const float h1 = (st.d1 <= 1e-15f && d2 <= 1e-15f) ? fmaxf(1e-6f, st.h0 * 1e-3f) : powf(0.01f / fmaxf(st.d1, d2), 0.2f);
        st.d2 = d2;
        dt = fminf(100.f * st.h0, h1);
        st.dt0 = dt;
        if (lead) {
            trow[0] = st.d0; trow[1] = st.d1; trow[2] = d2; trow[3] = st.h0; trow[4] = dt; trow[5] = trow[6] = trow[7] = 0.f;
        }
        hstep = dt;
    } else if (Lc >= 3) {
        // ---- decide attempt Lc - 3: ratio = mean((err / tol)^2), accept iff <= 1
        const float r = (float)(S[0] / nx);
        const bool accept = r <= 1.f;
        float dt_next;
        if (r == 0.f) dt_next = dt * DPH_IFACTOR;
        else {
            const float inv_d = r < 1.f ? 1.f : 1.f / DPH_DFACTOR;
            const float factor = fmaxf(1.f / DPH_IFACTOR, fminf(powf(sqrtf(r), 0.2f) / DPH_SAFETY, inv_d));
            dt_next = dt / factor;
        }
        if (lead) {
            float *tr = trow + DPH_TRACE_HEAD + DPH_TRACE_ROW * (Lc - 3);
            tr[0] = (float)(sgn * st.t); tr[1] = dt; tr[2] = r; tr[3] = 0.f; tr[4] = accept ? 1.f : 0.f;
        }
        if (accept) {
            ++st.nacc;
            const double t1s = st.t + (double)dt;
            float yn[3], k7[3], ym[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                yn[d] = pp[DPH_YN * qs + (long)d * a.n];
                k7[d] = pp[DPH_K7 * qs + (long)d * a.n];
                ym[d] = pp[DPH_YM * qs + (long)d * a.n];
            }
            if (t1s >= tq1) {
                // ---- the step went past the end: the 4th-order interpolant at the end time (y_new itself when it lands on it)
                if (own) {
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        double v = (double)yn[d];
                        if (t1s != tq1) {
                            const double y0d = s[d], y1d = yn[d], ymd = ym[d], fa = f0[d], fb = k7[d], h = dt;
                            const double A = 2.0 * h * (fb - fa) - 8.0 * (y1d + y0d) + 16.0 * ymd;
                            const double B = h * (5.0 * fa - 3.0 * fb) + 18.0 * y0d + 14.0 * y1d - 32.0 * ymd;
                            const double C = h * (fb - 4.0 * fa) - 11.0 * y0d - 5.0 * y1d + 16.0 * ymd;
                            const double D = h * fa;
                            const double xx = (tq1 - st.t) / (t1s - st.t);
                            v = (((A * xx + B) * xx + C) * xx + D) * xx + y0d;
                        }
                        float o = (float)v;
                        if (a.mbn_out) {
                            const float w = a.mbn_out[d], bb = a.mbn_out[3 + d], mean = a.mbn_out[6 + d], var = a.mbn_out[9 + d];
                            if (a.reverse) o = (o - bb) * expf(-w) * expf(0.5f * logf(var + 1e-4f)) + mean;
                            else o = (o - mean) * expf(-0.5f * logf(var + 1e-4f)) * expf(w) + bb;
                        }
                        a.y_out[((long)bt * a.n + col) * 3 + d] = o;
                    }
                }
                if (lead) {
                    st.t = t1s;
                    st.dt = dt_next;
                    st.done = 1;
                    *fnext = st;
                    int *c = a.counters + 4 * bt;
                    c[0] = st.nacc; c[1] = st.nrej; c[2] = st.nfe; c[3] = 1;
                }
                return;
            }
            // commit: (t, y, f0) <- (t + dt, y_new, k7)
            st.t = t1s;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                s[d] = yn[d];
                f0[d] = k7[d];
                if (own) {
                    pp[DPH_Y * qs + (long)d * a.n] = s[d];
                    pp[DPH_F0 * qs + (long)d * a.n] = f0[d];
                }
            }
        } else {
            ++st.nrej;
        }
        dt = dt_next;
        hstep = dt;
        if (a.last) {
            if (lead) {
                st.dt = dt;
                *fnext = st;
                int *c = a.counters + 4 * bt;
                c[0] = st.nacc; c[1] = st.nrej; c[2] = st.nfe; c[3] = 0;
                atomicAdd(a.running + Lc, 1);
            }
            return;
        }
    }
    const int nst = Lc < 2 ? 1 : 6;
    const double tq = st.t;
    // the frame's state after this launch is known here: written before the evaluation, which then carries nothing of it
    if (lead) {
        st.dt = dt;
        st.nfe += nst;
        *fnext = st;
        int *c = a.counters + 4 * bt;
        c[0] = st.nacc; c[1] = st.nrej; c[2] = st.nfe; c[3] = 0;
        atomicAdd(a.running + Lc, 1);
    }

    // ================= the evaluation of cnf_rk4_h3w_kernel (ode_f16x3w.hip) =================
    const float *hy = a.hyper + (long)bt * a.ldh;
    constexpr int BOFF = 3 * XC_H + 3;

    for (int i = tid; i < 3 * XC_H; i += 256) {
        s_w0[i] = a.w0[i];
        s_w3[i] = a.w3[i];
    }
    // the weight scales the pack kernel chose: W1 2^s1, W2 2^s2 are what the planes hold
    const int sh1 = *(const int *)(a.w1x + XH_PACK), sh2 = *(const int *)(a.w2x + XH_PACK);
    const float act = (float)(1 << XH_ACT_SHIFT), un1 = ldexpf(1.0f, -sh1), un2 = ldexpf(1.0f, -(XH_ACT_SHIFT + sh2));

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
    // piece (rq, kc) of a layer's pack sits at (rq * 16 + kc) * XH_PIECE.  Ring slot s & 7.  The index runs on from stage to stage of
    // the launch (& 127: 128 pieces are a multiple of the ring)
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

    // pieces 0..6 in flight before the first one is consumed
#pragma unroll
    for (int s_ = 0; s_ < XH_RING - 1; ++s_)
#pragma unroll
        for (int i0 = 0; i0 < 4; ++i0) dma1(s_, lane0 * 16, i0);

    f32x16 acc2[4];               // layer 2: the 128 rows of the running pass
    f16x8 fX[2][2], fY[2][2];     // A fragments: two sets of two row tiles x two planes
    u32x4 b1w[2][2][2];           // layer 1 B planes [chunk parity][k-step of the chunk][plane]
    u32x4 b2w[2][2];              // layer 2 B planes [k-step parity][plane]
    float xmax = 0.0f;            // range guard: the largest scaled activation this lane has split

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

    float k[7][3];                // k1..k7 of the point's three components (k1 = f0: FSAL)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        k[0][d] = f0[d];
#pragma unroll
        for (int i = 1; i < 7; ++i) k[i][d] = 0.f;
    }
    float ys[3] = {s[0], s[1], s[2]};   // the running stage's input; after the loop the last stage's: y_new of an attempt
    {
#pragma unroll 1
        for (int stage = 0; stage < nst; ++stage) {
            const int row = Lc < 2 ? Lc : 2 + stage;
            // the stage's time, negated back for the gates when the solve runs in reverse
            const float t = (float)(sgn * (tq + DPH_ALPHA[row] * (double)hstep));
            int lane = lane0;
            asm volatile("" : "+v"(lane));     // opaque: nothing derived from the lane id is hoisted out of the stage loop
            const int hq = (lane >> 5) * 4, lane16 = lane * 16;
            // layer 1 accumulates from zero (issued before the barrier: overlaps the other waves' arrival)
            xw_for<0, 256>([&](auto N) XW_INL { xw_acc_zero<decltype(N)::value>(); });
            __syncthreads();   // the previous stage's epilogues are done with the tables
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

            // stage input y + dt * sum_i beta[row][i] k_i
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                float bacc = 0.f;
#pragma unroll
                for (int i = 0; i < 6; ++i) bacc += DPH_BETA[row][i] * k[i][d];
                ys[d] = row == 0 ? s[d] : s[d] + hstep * bacc;
            }

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
                if constexpr (i == 4) xh_split1(pa);
                if constexpr (i == 5) xh_split2(pa, bw, 2 * grp + pr);
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
                        xh_split1(pa);
                        xh_split2(pa, b1w[0][ks], 2 * grp + pr);
                    }
                }
            XW_FENCE;
#pragma unroll 1
            for (int it = 0; it < 8; ++it) {
                xw_for<0, 8>([&](auto PC) XW_INL {
                    constexpr int pc = decltype(PC)::value, par = pc >> 2, rq = pc & 3;   // chunk kc = 2 it + par, ring slot = pc
                    const int s1 = 8 * it + pc;                                            // sequence piece
                    const unsigned char *A = wbuf + pc * XH_PIECE + lane16;
                    const unsigned char *An = wbuf + ((pc + 1) & (XH_RING - 1)) * XH_PIECE + lane16;
                    // producers of chunk kc + 1 (B set par ^ 1): piece rq makes group (ks = rq >> 1, grp = rq & 1): tables in
                    // region 0, one pair in regions 1 and 2 each.  (Chunk 16 does not exist: the last pass produces chunk 0 once
                    // more -- values the range guard has already seen -- into a B set nobody multiplies.)
                    const int ubn = 32 * ((2 * it + par + 1) & 15) + 16 * (rq >> 1) + 8 * (rq & 1) + hq;
                    u32x4 (&bn)[2] = b1w[par ^ 1][rq >> 1];
                    // region 0: k-step 0, row tiles 0, 1 (fX) | reads k-step 0, row tiles 2, 3 -> fY
                    region_a(std::integral_constant<int, 4 * rq>{}, fX, b1w[par][0], fY, A + 4 * XH_FRAG, [&](auto I) XW_INL {
                        constexpr int i = decltype(I)::value;
                        if constexpr (i == 0) l1_tab(ubn);
                        if constexpr (i == 4) dma1(s1 + 7, lane16, 0);
                    });
                    // region 1: k-step 0, row tiles 2, 3 (fY) | reads k-step 1, row tiles 0, 1 -> fX
                    region_a(std::integral_constant<int, 4 * rq + 2>{}, fY, b1w[par][0], fX, A + 8 * XH_FRAG, [&](auto I) XW_INL {
                        constexpr int i = decltype(I)::value;
                        l1_pair_step(I, bn, rq & 1, 0);
                        if constexpr (i == 3) dma1(s1 + 7, lane16, 1);
                    });
                    // region 2: k-step 1, row tiles 0, 1 (fX) | reads k-step 1, row tiles 2, 3 -> fY
                    region_a(std::integral_constant<int, 4 * rq>{}, fX, b1w[par][1], fY, A + 12 * XH_FRAG, [&](auto I) XW_INL {
                        constexpr int i = decltype(I)::value;
                        l1_pair_step(I, bn, rq & 1, 1);
                        if constexpr (i == 3) dma1(s1 + 7, lane16, 2);
                    });
                    // region 3: the last kilobyte of piece s1 + 7 | barrier of the next piece | k-step 1, row tiles 2, 3 (fY) | reads
                    // the next piece's k-step 0, row tiles 0, 1 -> fX
                    region_a_last(std::integral_constant<int, 4 * rq + 2>{}, fY, b1w[par][1], fX, An, [&](auto I) XW_INL {
                        constexpr int i = decltype(I)::value;
                        if constexpr (i == 1) dma1(s1 + 7, lane16, 3);
                    });
                });
            }

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
                        xh_split1(pa);
                        xh_split1(pb);
                    }
                    if constexpr (i == 5) {
                        xh_split2(pa, bw, 2 * grp);
                        xh_split2(pb, bw, 2 * grp + 1);
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
                    // k-step t + 1 is produced during k-step t: group 0 in the region of row tiles 0, 1 (tables in tt[0]), group 1 in
                    // the region of row tiles 2, 3 (tt[1]); slot 3 of a region reads the tables of the next region's group
                    // region 0: k-step 2 kc, row tiles 0, 1 (fX) | reads row tiles 2, 3 -> fY | group 0 of k-step tb
                    region_v(acc2[0], acc2[1], fX, b2w[0], fY, A + 4 * XH_FRAG, [&](auto I) XW_INL {
                        constexpr int i = decltype(I)::value;
                        l2_step(I, std::integral_constant<int, tb>{}, std::integral_constant<int, 0>{}, FC, b2w[1], 0);
                        if constexpr (first && i == 3) l2_tab(1, tb, 1);
                        if constexpr (i == 4) dma1(sq + 7, lane16, 0);
                    });
                    // region 1: k-step 2 kc, row tiles 2, 3 (fY) | reads tb, row tiles 0, 1 -> fX | group 1 of tb
                    region_v(acc2[2], acc2[3], fY, b2w[0], fX, A + 8 * XH_FRAG, [&](auto I) XW_INL {
                        constexpr int i = decltype(I)::value;
                        l2_step(I, std::integral_constant<int, tb>{}, std::integral_constant<int, 1>{}, FC, b2w[1], 1);
                        if constexpr (first && kc < 15 && i == 3) l2_tab(0, tn, 0);
                        if constexpr (i == 4) dma1(sq + 7, lane16, 1);
                    });
                    // region 2: k-step tb, row tiles 0, 1 (fX) | reads tb, row tiles 2, 3 -> fY | group 0 of k-step tb + 1
                    region_v(acc2[0], acc2[1], fX, b2w[1], fY, A + 12 * XH_FRAG, [&](auto I) XW_INL {
                        constexpr int i = decltype(I)::value;
                        if constexpr (kc < 15) l2_step(I, std::integral_constant<int, tn>{}, std::integral_constant<int, 0>{}, FC, b2w[0], 0);
                        if constexpr (first && kc < 15 && i == 3) l2_tab(1, tn, 1);
                        if constexpr (i == 4) dma1(sq + 7, lane16, 2);
                    });
                    // region 3: the last kilobyte of piece sq + 7 | barrier of the next piece | k-step tb, row tiles 2, 3 (fY) | reads
                    // the next piece's first fragments -> fX | group 1 of k-step tb + 1
                    region_v_last(acc2[2], acc2[3], fY, b2w[1], fX, An, [&](auto I) XW_INL {
                        constexpr int i = decltype(I)::value;
                        if constexpr (kc < 15) l2_step(I, std::integral_constant<int, tn>{}, std::integral_constant<int, 1>{}, FC, b2w[0], 1);
                        if constexpr (first && kc < 15 && i == 3) l2_tab(0, tn + 1, 0);
                        if constexpr (i == 1) dma1(sq + 7, lane16, 3);
                    });
                });
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
            };
            int q0 = 0;
            asm volatile("" : "+s"(q0));     // opaque: the piece addresses of pass 0 are computed like those of passes 1-3 (SALU)
            pass(q0, std::true_type{});
#pragma unroll 1
            for (int q = 1; q < 4; ++q) pass(q, std::false_type{});

            // ---- output ConcatSquash (no softplus: odefunc.py:103): the two halves of a column hold disjoint rows.  f of the point's
            // state, negated when the solve runs in reverse
            const int kidx = Lc < 2 ? 1 : stage + 1;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                float v = part[d];
                v += __shfl_xor(v, 32);
                const float od = fmaf(v, s_g3[d], s_g3[4 + d]);
                const float kv = a.reverse ? -od : od;
#pragma unroll
                for (int i = 1; i < 7; ++i)
                    if (i == kidx) k[i][d] = kv;
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the pieces left in flight by the last stage

    // ---- this workgroup's partial sums and the carry-over of its points.  Range guard: the two halves of a column split disjoint units
    // of the same point
    xmax = fmaxf(xmax, __shfl_xor(xmax, 32));
    const bool bad = !(xmax < XH_F16_LIMIT);
    double v[3] = {0.0, 0.0, 0.0};
    if (own) {
        if (bad) {
            atomicOr(a.status, DPH_GUARD);
            v[1] = 1.0;
        }
        if (Lc == 0) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const float sc = a.atol + fabsf(s[d]) * a.rtol;
                const float q0 = s[d] / sc, q1 = k[1][d] / sc;
                v[0] += (double)q0 * (double)q0;
                v[2] += (double)q1 * (double)q1;
                pp[DPH_Y * qs + (long)d * a.n] = s[d];
                pp[DPH_F0 * qs + (long)d * a.n] = k[1][d];
            }
        } else if (Lc == 1) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const float sc = a.atol + fabsf(s[d]) * a.rtol;
                const float q0 = (k[1][d] - k[0][d]) / sc;
                v[0] += (double)q0 * (double)q0;
            }
        } else {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                float eacc = 0.f, macc = 0.f;
#pragma unroll
                for (int i = 0; i < 7; ++i) {
                    eacc += DPH_CERR[i] * k[i][d];
                    macc += DPH_CMID[i] * k[i][d];
                }
                const float err = dt * eacc, ym = s[d] + dt * macc;
                const float tol = a.atol + a.rtol * fmaxf(fabsf(s[d]), fabsf(ys[d]));
                const float q0 = err / tol;
                v[0] += (double)q0 * (double)q0;
                pp[DPH_YN * qs + (long)d * a.n] = ys[d];
                pp[DPH_K7 * qs + (long)d * a.n] = k[6][d];
                pp[DPH_YM * qs + (long)d * a.n] = ym;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int o_ = 32; o_ > 0; o_ >>= 1) v[q] += __shfl_xor(v[q], o_);
    }
    if (lane0 == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) s_red[4 * wave + q] = v[q];
    }
    __syncthreads();
    if (tid == 0) {
        double *slot = a.part + (((long)par * BT + bt) * nwg + blockIdx.x) * 4;
#pragma unroll
        for (int q = 0; q < 3; ++q) slot[q] = ((s_red[q] + s_red[4 + q]) + s_red[8 + q]) + s_red[12 + q];
        slot[3] = 0.0;
    }
}

static inline long dph_align(long b) { return (b + 255) & ~255L; }
struct Dp5H3Layout { long frames, part, running, pts, total; };
static Dp5H3Layout dph_layout(int BT, int n, int max_attempts)
{
    Dp5H3Layout l;
    const long nwg = ceil_div(n, XH_PTS);
    l.frames = 0;
    l.part = dph_align(2L * BT * (long)sizeof(Dp5H3Frame));
    l.running = l.part + dph_align(2L * BT * nwg * 4 * (long)sizeof(double));
    l.pts = l.running + dph_align(((long)max_attempts + 3) * (long)sizeof(int));
    l.total = l.pts + dph_align((long)BT * 15 * n * (long)sizeof(float));
    return l;
}

extern "C" long caspr_cnf_dopri5_h3_ws_bytes(int BT, int n, int max_attempts)
{
    if (BT <= 0 || n <= 0 || max_attempts <= 0) return 0;
    return dph_layout(BT, n, max_attempts).total;
}

extern "C" int caspr_cnf_dopri5_h3_f32(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0,
                                       const float *b0, const void *w1h, const float *b1, const void *w2h, const float *b2,
                                       const float *w3, const float *b3, int H, float t_end, float rtol, float atol, int max_attempts,
                                       int reverse, const float *mbn_in, const float *mbn_out, unsigned *status, float *y_out, int BT,
                                       int n, void *ws, long ws_bytes, float *trace, int32_t *counters, void *stream)
{
    CASPR_REQUIRE(y_in && hyper && tcol && w0 && b0 && w1h && b1 && w2h && b2 && w3 && b3 && y_out && ws && trace && counters && status, "cnf_dopri5_h3: null pointer");
    CASPR_REQUIRE(H == XC_H, "cnf_dopri5_h3: hidden width %d unsupported (kernel is built for 512-512-512, flow.py:89)", H);
    CASPR_REQUIRE(BT > 0 && BT <= 65535 && n > 0 && max_attempts > 0 && ldh >= 2 * (3 * H + 3), "cnf_dopri5_h3: bad sizes");
    CASPR_REQUIRE(rtol > 0.f && atol > 0.f && t_end > 0.f && rtol < INFINITY && atol < INFINITY && t_end < INFINITY, "cnf_dopri5_h3: rtol, atol and t_end must be positive and finite");
    CASPR_REQUIRE(((uintptr_t)w1h % 16) == 0 && ((uintptr_t)w2h % 16) == 0 && ((uintptr_t)w0 % 16) == 0 && ((uintptr_t)w3 % 16) == 0,
                  "cnf_dopri5_h3: weights must be 16-byte aligned");
    const Dp5H3Layout l = dph_layout(BT, n, max_attempts);
    CASPR_REQUIRE(ws_bytes >= l.total && ((uintptr_t)ws % 256) == 0, "cnf_dopri5_h3: workspace of %ld bytes, 256-byte aligned, needed", l.total);
    hipStream_t st = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        caspr_set_error("cnf_dopri5_h3: the host loop reads the device after every attempt and cannot run under stream capture");
        return CASPR_EUNSUP;
    }
    CnfDp5H3Args a;
    a.y_in = y_in; a.hyper = hyper; a.tcol = tcol; a.w0 = w0; a.b0 = b0; a.b1 = b1; a.b2 = b2; a.w3 = w3; a.b3 = b3;
    a.mbn_in = mbn_in; a.mbn_out = mbn_out; a.w1x = (const unsigned char *)w1h; a.w2x = (const unsigned char *)w2h;
    a.y_out = y_out; a.ldh = ldh; a.n = n; a.reverse = reverse & 1; a.t_end = t_end; a.rtol = rtol; a.atol = atol;
    a.max_attempts = max_attempts;
    unsigned char *wsb = (unsigned char *)ws;
    a.frames = (Dp5H3Frame *)(wsb + l.frames);
    a.part = (double *)(wsb + l.part);
    a.running = (int *)(wsb + l.running);
    a.pts = (float *)(wsb + l.pts);
    a.trace = trace;
    a.counters = counters;
    a.status = status;
    static CasprLdsOptIn optin;
    const hipError_t err = caspr_lds_opt_in(optin, (const void *)cnf_dp5_h3w_kernel, DPH_LDS);
    if (err != hipSuccess) {
        caspr_set_error("cnf_dopri5_h3: hipFuncSetAttribute failed: %s", hipGetErrorString(err));
        return CASPR_ELAUNCH;
    }
    int *h_running = nullptr;
    if (hipHostMalloc((void **)&h_running, sizeof(int), hipHostMallocDefault) != hipSuccess) {
        caspr_set_error("cnf_dopri5_h3: hipHostMalloc failed");
        return CASPR_ELAUNCH;
    }
    hipError_t he = hipMemsetAsync(a.running, 0, ((long)max_attempts + 3) * sizeof(int), st);
    if (he == hipSuccess) he = hipMemsetAsync(trace, 0, (long)BT * (DPH_TRACE_HEAD + DPH_TRACE_ROW * (long)max_attempts) * sizeof(float), st);
    if (he == hipSuccess) he = hipMemsetAsync(status, 0, sizeof(unsigned), st);
    int running = 1, rc = CASPR_OK;
    // launch L = 0, 1: initial-step selection; L >= 2: decide attempt L - 3, run attempt L - 2; L = max_attempts + 2 decides only
    for (int L = 0; he == hipSuccess && L <= max_attempts + 2; ++L) {
        a.launch = L;
        a.last = L == max_attempts + 2;
        cnf_dp5_h3w_kernel<<<dim3(ceil_div(n, XH_PTS), BT), dim3(256), DPH_LDS, st>>>(a);
        he = hipGetLastError();
        if (he != hipSuccess || L < 3) continue;       // no frame's attempt is decided before launch 3
        // one small pinned read per attempt: the frames that launch L left running
        he = hipMemcpyAsync(h_running, a.running + L, sizeof(int), hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he != hipSuccess) break;
        running = *h_running;
        if (running == 0) break;
    }
    (void)hipHostFree(h_running);
    if (he != hipSuccess) {
        caspr_set_error("cnf_dopri5_h3: %s", hipGetErrorString(he));
        return CASPR_ELAUNCH;
    }
    if (running != 0) {
        caspr_set_error("cnf_dopri5_h3: %d of %d frames did not reach t_end within max_attempts = %d (rtol %g, atol %g)", running, BT, max_attempts,
                        (double)rtol, (double)atol);
        rc = CASPR_ENOCONV;
    }
    return rc;
}
