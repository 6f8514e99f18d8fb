// ode_dp5.hip -- the point-CNF solve (cnf.py:96-118) integrated to a TOLERANCE: adaptive Dormand-Prince 5(4) as torchdiffeq
// 0.0.1 runs it (oracle.model.dopri5_solve restates it), with the error norms taken PER FRAME: a frame's result is what the
// reference computes when it is called on that frame alone, whatever batch surrounds it.
//
// The ODE function evaluation is the one of ode_bf16x6.hip, shared with it as text (ode_x6_setup.inc, ode_x6_eval.inc; 64-point
// geometry: a wave owns 16 points and all 512 hidden units, both hidden layers on the bf16 matrix pipe in the exact three-way
// split, weight pieces by LDS-DMA; DIV: 32 points with their Hutchinson tangent columns).  This file adds the loop around it:
//  * ONE LAUNCH PER ATTEMPT.  A frame spans several workgroups and its norms need all of them, but no workgroup ever
//    waits on another: a workgroup writes its partial sums of squares (f64) to ITS slot of the workspace (slots double-
//    buffered by launch parity), and the NEXT launch's prologue adds the frame's slots in slot order.  Every workgroup of
//    the frame therefore takes the identical accept / reject decision and the identical next dt, without float atomics;
//    it commits or discards y_new, and either writes the interpolated output and retires (retired frames return at once in
//    later launches) or runs the six stage evaluations of the next attempt;
//  * launch 0 evaluates f(t0, y0), launch 1 f(t0 + h0, y0 + h0 f0) (initial-step selection: d0, d1, then d2), launch L >= 2
//    decides attempt L - 3 and runs attempt L - 2;
//  * the state is 3 + 1 floats per point: lane (g, j) of a wave holds component g of point j (g = 3: the log-density, which
//    has zero derivative without e / logp, as oracle.cnf_block), k1..k7 in registers, the tableau rows in constant memory;
//  * per-point carry-over between launches (y, f0, y_new, k7, y_mid: 20 floats) lives in the workspace;
//  * the host loop (caspr_cnf_dopri5_f32) launches until the device word "frames still running" of that launch reads zero and
//    stops with CASPR_ENOCONV after max_attempts attempts: never an unbounded loop.
// Results are bitwise run to run and independent of the other frames of the batch.
#include "ode_x6.h"

// ---- Dormand-Prince 5(4), Shampine's variant as torchdiffeq 0.0.1 dopri5.py.  Rows 0 and 1 are the two evaluations of the
// initial-step selection (y0 itself; y0 + h0 f0), rows 2..7 the six new stages of an attempt (the last one is y_new: FSAL).
__constant__ float DP_BETA[8][6] = {
    {0.f, 0.f, 0.f, 0.f, 0.f, 0.f},
    {1.f, 0.f, 0.f, 0.f, 0.f, 0.f},
    {(float)(1.0 / 5), 0.f, 0.f, 0.f, 0.f, 0.f},
    {(float)(3.0 / 40), (float)(9.0 / 40), 0.f, 0.f, 0.f, 0.f},
    {(float)(44.0 / 45), (float)(-56.0 / 15), (float)(32.0 / 9), 0.f, 0.f, 0.f},
    {(float)(19372.0 / 6561), (float)(-25360.0 / 2187), (float)(64448.0 / 6561), (float)(-212.0 / 729), 0.f, 0.f},
    {(float)(9017.0 / 3168), (float)(-355.0 / 33), (float)(46732.0 / 5247), (float)(49.0 / 176), (float)(-5103.0 / 18656), 0.f},
    {(float)(35.0 / 384), 0.f, (float)(500.0 / 1113), (float)(125.0 / 192), (float)(-2187.0 / 6784), (float)(11.0 / 84)},
};
__constant__ double DP_ALPHA[8] = {0.0, 1.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
__constant__ float DP_CERR[7] = {(float)(35.0 / 384 - 1951.0 / 21600), 0.f, (float)(500.0 / 1113 - 22642.0 / 50085), (float)(125.0 / 192 - 451.0 / 720),
                                 (float)(-2187.0 / 6784 - -12231.0 / 42400), (float)(11.0 / 84 - 649.0 / 6300), (float)(-1.0 / 60.0)};
__constant__ float DP_CMID[7] = {(float)(6025192743.0 / 30085553152.0 / 2), 0.f, (float)(51252292925.0 / 65400821598.0 / 2),
                                 (float)(-2691868925.0 / 45128329728.0 / 2), (float)(187940372067.0 / 1594534317056.0 / 2),
                                 (float)(-1776094331.0 / 19743644256.0 / 2), (float)(11237099.0 / 235043384.0 / 2)};
#define DP_SAFETY 0.9f
#define DP_IFACTOR 10.0f
#define DP_DFACTOR 0.2f

#define DP_TRACE_HEAD 8      // floats per frame before the attempt rows: d0, d1, d2, h0, first dt, 0, 0, 0
#define DP_TRACE_ROW 5       // per attempt: t, dt, ratio of x, ratio of logp, accepted (1 / 0)
#define DP_LDS (XC_LDS + 16 * 8)
// carry-over quantities of a point, each [4 components][n]
#define DP_Y 0
#define DP_F0 1
#define DP_YN 2
#define DP_K7 3
#define DP_YM 4

struct Dp5Frame {            // a frame's controller state, written by its first workgroup, double-buffered by launch parity
    double t;                // solver time (negated when the solve runs in reverse, as upstream)
    float dt, h0, d0, d1, d2, dt0;
    int done, nacc, nrej, nfe;
    int pad[2];
};

struct CnfDp5Args {
    const float *y_in, *hyper, *tcol, *w0, *b0, *b1, *b2, *w3, *b3, *mbn_in, *mbn_out;
    const float *e, *logp_in;     // DIV only: Hutchinson noise (BT,n,3), initial log-density (BT,n) or NULL
    float *logp_out;              // DIV only
    const unsigned char *w1x, *w2x;
    float *y_out;
    int ldh, n, reverse;
    float t_end, rtol, atol;
    int launch;                   // 0: f(t0, y0); 1: f(t0 + h0, y0 + h0 f0); L >= 2: decide attempt L - 3, run attempt L - 2
    int last;                     // the attempt budget is used up: decide only
    int max_attempts;
    Dp5Frame *frames;             // [2][BT]
    double *part;                 // [2][BT][workgroups of a frame][4]
    float *pts;                   // [BT][5][4][n]
    int *running;                 // [launch]: frames that did not retire in that launch
    float *trace;                 // [BT][DP_TRACE_HEAD + DP_TRACE_ROW * max_attempts]
    int *counters;                // [BT][4]: accepted, rejected, evaluations, finished
};

template <bool DIV>
__global__ __launch_bounds__(256, 1) void cnf_dp5_kernel(CnfDp5Args a)
{
    const int tid = threadIdx.x, lane0 = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g0 = lane0 >> 4;
    const int bt = blockIdx.y, BT = gridDim.y, nwg = gridDim.x;
    // DIV: a wave's 16 columns are 8 points (j < 8) and their 8 tangent columns (j >= 8); the workgroup owns 32 points
    const int col = DIV ? blockIdx.x * (XC_COLS / 2) + 8 * wave + (lane0 & 7) : blockIdx.x * XC_COLS + 16 * wave + (lane0 & 15);
    const bool tg0 = DIV && (lane0 & 8);
    const bool cvalid = col < a.n;
    const int ccol = cvalid ? col : a.n - 1;
    const float *hy = a.hyper + (long)bt * a.ldh;
    constexpr int GOFF = 0, BOFF = 3 * XC_H + 3;
    const int sd = g0 < 3 ? g0 : 0;
    // this lane's state float: component g0 of its point (g0 == 3: the log-density; without e / logp it is 0 with derivative 0
    // and is neither stored nor counted); tangent lanes carry e_d, constant over the solve
    const bool own = cvalid && !tg0 && (g0 < 3 || DIV);
    const int ti = g0 == 3 ? 1 : 0;                             // which tensor of the state (x | logp) the lane's float belongs to
    float *pp = a.pts + ((long)bt * 20 + g0) * a.n + ccol;      // quantity q at pp[q * 4 * n]
    const long qs = 4L * a.n;

    const int Lc = a.launch, par = Lc & 1;
    const Dp5Frame *fprev = a.frames + (long)(par ^ 1) * BT + bt;
    Dp5Frame *fnext = a.frames + (long)par * BT + bt;
    const bool lead = blockIdx.x == 0 && tid == 0;
    const double sgn = a.reverse ? -1.0 : 1.0;
    const double tq1 = a.reverse ? 0.0 : (double)a.t_end;       // where the solve ends, in solver time
    Dp5Frame st;
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

    float s = 0.f, f0 = 0.f;
    if (Lc == 0) {
        float v = a.y_in[((long)bt * a.n + ccol) * 3 + sd];
        if (a.mbn_in) {
            const float w = a.mbn_in[sd], bb = a.mbn_in[3 + sd], mean = a.mbn_in[6 + sd], var = a.mbn_in[9 + sd];
            if (a.reverse) v = (v - bb) * expf(-w) * expf(0.5f * logf(var + 1e-4f)) + mean;   // normalization.py:92-94
            else v = (v - mean) * expf(-0.5f * logf(var + 1e-4f)) * expf(w) + bb;             // normalization.py:70-74
        }
        if (g0 == 3) v = 0.f;
        if (DIV) {
            if (tg0) v = a.e[((long)bt * a.n + ccol) * 3 + sd];
            else if (g0 == 3) {
                float lp = a.logp_in ? a.logp_in[(long)bt * a.n + ccol] : 0.f;
                if (a.mbn_in) {
                    float ld = 0.f;
#pragma unroll
                    for (int d = 0; d < 3; ++d) ld += -0.5f * logf(a.mbn_in[9 + d] + 1e-4f) + a.mbn_in[d];   // normalization.py:103-108
                    lp = a.reverse ? lp + ld : lp - ld;
                }
                v = lp;
            }
        }
        s = v;
    } else {
        if (own) {
            s = pp[DP_Y * qs];
            f0 = pp[DP_F0 * qs];
        }
        if (DIV && tg0) s = a.e[((long)bt * a.n + ccol) * 3 + sd];
    }

    // ---- the frame's sums of squares of the previous launch: its workgroups' slots added in slot order, the same in every
    // workgroup of the frame
    double S[4] = {0.0, 0.0, 0.0, 0.0};
    if (Lc > 0) {
        const double *p = a.part + ((long)(par ^ 1) * BT + bt) * nwg * 4;
        for (int w = 0; w < nwg; ++w)
#pragma unroll
            for (int q = 0; q < 4; ++q) S[q] += p[4 * w + q];
    }
    const double nx = 3.0 * (double)a.n, nl = (double)a.n;
    float *trow = a.trace + (long)bt * (DP_TRACE_HEAD + DP_TRACE_ROW * a.max_attempts);
    float dt = st.dt, hstep = 0.f;
    if (Lc == 1) {
        // _select_initial_step: d0 = max over tensors of rms(y / scale), d1 of rms(f0 / scale)
        const double d0x = sqrt(S[0] / nx), d0l = sqrt(S[1] / nl), d1x = sqrt(S[2] / nx), d1l = sqrt(S[3] / nl);
        const double d0 = fmax(d0x, d0l), d1 = fmax(d1x, d1l);
        const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * fmax(d0x / fmax(d1x, 1e-300), d0l / fmax(d1l, 1e-300));
        st.d0 = (float)d0;
        st.d1 = (float)d1;
        st.h0 = (float)h0;
        hstep = st.h0;
    } else if (Lc == 2) {
        const float d2 = (float)(fmax(sqrt(S[0] / nx), sqrt(S[1] / nl)) / (double)st.h0);
        const float h1 = (st.d1 <= 1e-15f && d2 <= 1e-15f) ? fmaxf(1e-6f, st.h0 * 1e-3f) : powf(0.01f / fmaxf(st.d1, d2), 0.2f);
        st.d2 = d2;
        dt = fminf(100.f * st.h0, h1);
        st.dt0 = dt;
        if (lead) {
            trow[0] = st.d0; trow[1] = st.d1; trow[2] = d2; trow[3] = st.h0; trow[4] = dt; trow[5] = trow[6] = trow[7] = 0.f;
        }
        hstep = dt;
    } else if (Lc >= 3) {
        // ---- decide attempt Lc - 3: ratio = mean((err / tol)^2) per tensor, accept iff both <= 1
        const float r0 = (float)(S[0] / nx), r1 = (float)(S[1] / nl);
        const bool accept = r0 <= 1.f && r1 <= 1.f;
        const float r = fmaxf(r0, r1);
        float dt_next;
        if (r == 0.f) dt_next = dt * DP_IFACTOR;
        else {
            const float inv_d = r < 1.f ? 1.f : 1.f / DP_DFACTOR;
            const float factor = fmaxf(1.f / DP_IFACTOR, fminf(powf(sqrtf(r), 0.2f) / DP_SAFETY, inv_d));
            dt_next = dt / factor;
        }
        if (lead) {
            float *tr = trow + DP_TRACE_HEAD + DP_TRACE_ROW * (Lc - 3);
            tr[0] = (float)(sgn * st.t); tr[1] = dt; tr[2] = r0; tr[3] = r1; tr[4] = accept ? 1.f : 0.f;
        }
        if (accept) {
            ++st.nacc;
            const double t1s = st.t + (double)dt;
            float yn = 0.f, k7 = 0.f, ym = 0.f;
            if (own) {
                yn = pp[DP_YN * qs];
                k7 = pp[DP_K7 * qs];
                ym = pp[DP_YM * qs];
            }
            if (t1s >= tq1) {
                // ---- the step went past the end: the 4th-order interpolant at the end time (y_new itself when it lands on it)
                double v = (double)yn;
                if (t1s != tq1) {
                    const double y0d = s, y1d = yn, ymd = ym, fa = f0, fb = k7, h = dt;
                    const double A = 2.0 * h * (fb - fa) - 8.0 * (y1d + y0d) + 16.0 * ymd;
                    const double B = h * (5.0 * fa - 3.0 * fb) + 18.0 * y0d + 14.0 * y1d - 32.0 * ymd;
                    const double C = h * (fb - 4.0 * fa) - 11.0 * y0d - 5.0 * y1d + 16.0 * ymd;
                    const double D = h * fa;
                    const double xx = (tq1 - st.t) / (t1s - st.t);
                    v = (((A * xx + B) * xx + C) * xx + D) * xx + y0d;
                }
                float o = (float)v;
                if (own && g0 == 3) {
                    if (a.mbn_out) {
                        float ld = 0.f;
#pragma unroll
                        for (int d = 0; d < 3; ++d) ld += -0.5f * logf(a.mbn_out[9 + d] + 1e-4f) + a.mbn_out[d];
                        o = a.reverse ? o + ld : o - ld;
                    }
                    a.logp_out[(long)bt * a.n + col] = o;
                }
                if (own && g0 < 3) {
                    if (a.mbn_out) {
                        const float w = a.mbn_out[sd], bb = a.mbn_out[3 + sd], mean = a.mbn_out[6 + sd], var = a.mbn_out[9 + sd];
                        if (a.reverse) o = (o - bb) * expf(-w) * expf(0.5f * logf(var + 1e-4f)) + mean;
                        else o = (o - mean) * expf(-0.5f * logf(var + 1e-4f)) * expf(w) + bb;
                    }
                    a.y_out[((long)bt * a.n + col) * 3 + sd] = o;
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
            if (own) {                                          // (tangent lanes keep e)
                s = yn;
                f0 = k7;
                pp[DP_Y * qs] = s;
                pp[DP_F0 * qs] = f0;
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

#include "ode_x6_setup.inc"
    double *s_red = (double *)(s_g3 + 8);                       // [4 waves][4] partial sums of squares: the 16 * 8 bytes of DP_LDS past XC_LDS

    // the first piece of layer 1; every layer pass leaves the NEXT pass's first piece in flight
    dma(a.w1x, 0, lane0 * 16);

    float k[7] = {f0, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // k1..k7 of this lane's state float (k1 = f0: FSAL)
    float ylast = s;                                   // the last stage's input: y_new of an attempt
    {
#pragma unroll 1
        for (int stage = 0; stage < nst; ++stage) {
            const int row = Lc < 2 ? Lc : 2 + stage;
            // stage input y + h * sum_i beta[row][i] k_i (tangent lanes: their k stay 0) and its time, negated back for the
            // gates when the solve runs in reverse
            float bacc = 0.f;
#pragma unroll
            for (int i = 0; i < 6; ++i) bacc += DP_BETA[row][i] * k[i];
            const float ystage_in = row == 0 ? s : s + hstep * bacc;
            ylast = ystage_in;
            const float t = (float)(sgn * (tq + DP_ALPHA[row] * (double)hstep));
#define XC_STAGE_INPUT ystage_in
#define XC_LAYERS_ON true
#include "ode_x6_eval.inc"
            float nd = 0.f;
            if (DIV) {
                // -divergence estimate = -(e . J e) (odefunc.py:26,136): tangent lanes (g < 3) hold e_g and all of J e
                float dv = (tg && g < 3) ? ystage * od : 0.f;
                dv += __shfl_xor(dv, 16);
                dv += __shfl_xor(dv, 32);
                nd = -xc_partner(dv);                        // lands in the point's value column (every g)
            }
            // f of this lane's state float (negated when the solve runs in reverse)
            float kv = (DIV && tg) ? 0.f : (g < 3 ? od : nd);
            if (a.reverse) kv = -kv;
            const int kidx = Lc < 2 ? 1 : stage + 1;
#pragma unroll
            for (int i = 1; i < 7; ++i)
                if (i == kidx) k[i] = kv;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the prefetch left in flight by the last layer pass

    // ---- this workgroup's partial sums of squares and the carry-over of its points
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (Lc == 0) {
        if (own) {
            const float sc = a.atol + fabsf(s) * a.rtol;
            const float q0 = s / sc, q1 = k[1] / sc;
            v[ti] = (double)q0 * (double)q0;
            v[2 + ti] = (double)q1 * (double)q1;
            pp[DP_Y * qs] = s;
            pp[DP_F0 * qs] = k[1];
        }
    } else if (Lc == 1) {
        if (own) {
            const float sc = a.atol + fabsf(s) * a.rtol;
            const float q0 = (k[1] - k[0]) / sc;
            v[ti] = (double)q0 * (double)q0;
        }
    } else {
        float eacc = 0.f, macc = 0.f;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            eacc += DP_CERR[i] * k[i];
            macc += DP_CMID[i] * k[i];
        }
        if (own) {
            const float err = dt * eacc, ym = s + dt * macc;
            const float tol = a.atol + a.rtol * fmaxf(fabsf(s), fabsf(ylast));
            const float q0 = err / tol;
            v[ti] = (double)q0 * (double)q0;
            pp[DP_YN * qs] = ylast;
            pp[DP_K7 * qs] = k[6];
            pp[DP_YM * qs] = ym;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int o_ = 32; o_ > 0; o_ >>= 1) v[q] += __shfl_xor(v[q], o_);
    }
    if (lane0 == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) s_red[4 * wave + q] = v[q];
    }
    __syncthreads();
    if (tid == 0) {
        double *slot = a.part + (((long)par * BT + bt) * nwg + blockIdx.x) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) slot[q] = ((s_red[q] + s_red[4 + q]) + s_red[8 + q]) + s_red[12 + q];
    }
    if (lead) {
        st.dt = dt;
        st.nfe += nst;
        *fnext = st;
        int *c = a.counters + 4 * bt;
        c[0] = st.nacc; c[1] = st.nrej; c[2] = st.nfe; c[3] = 0;
        atomicAdd(a.running + Lc, 1);
    }
}

static inline long dp5_align(long b) { return (b + 255) & ~255L; }
struct Dp5Layout { long frames, part, running, pts, total; };
static Dp5Layout dp5_layout(int BT, int n, int max_attempts)
{
    Dp5Layout l;
    const long nwg = ceil_div(n, XC_COLS / 2);           // the divergence variant's count: the larger one
    l.frames = 0;
    l.part = dp5_align(2L * BT * (long)sizeof(Dp5Frame));
    l.running = l.part + dp5_align(2L * BT * nwg * 4 * (long)sizeof(double));
    l.pts = l.running + dp5_align(((long)max_attempts + 3) * (long)sizeof(int));
    l.total = l.pts + dp5_align((long)BT * 20 * n * (long)sizeof(float));
    return l;
}

extern "C" long caspr_cnf_dopri5_ws_bytes(int BT, int n, int max_attempts)
{
    if (BT <= 0 || n <= 0 || max_attempts <= 0) return 0;
    return dp5_layout(BT, n, max_attempts).total;
}

extern "C" int caspr_cnf_dopri5_f32(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0,
                                    const float *b0, const void *w1x, const float *b1, const void *w2x, const float *b2,
                                    const float *w3, const float *b3, int H, float t_end, float rtol, float atol, int max_attempts,
                                    int reverse, const float *mbn_in, const float *mbn_out, const float *e, const float *logp_in,
                                    float *logp_out, float *y_out, int BT, int n, void *ws, long ws_bytes, float *trace,
                                    int32_t *counters, void *stream)
{
    CASPR_REQUIRE(y_in && hyper && tcol && w0 && b0 && w1x && b1 && w2x && b2 && w3 && b3 && y_out && ws && trace && counters, "cnf_dopri5: null pointer");
    CASPR_REQUIRE(H == XC_H, "cnf_dopri5: hidden width %d unsupported (kernel is built for 512-512-512, flow.py:89)", H);
    CASPR_REQUIRE(BT > 0 && BT <= 65535 && n > 0 && max_attempts > 0 && ldh >= 2 * (3 * H + 3), "cnf_dopri5: bad sizes");
    CASPR_REQUIRE(rtol > 0.f && atol > 0.f && t_end > 0.f && rtol < INFINITY && atol < INFINITY && t_end < INFINITY, "cnf_dopri5: rtol, atol and t_end must be positive and finite");
    CASPR_REQUIRE((e == nullptr) == (logp_out == nullptr), "cnf_dopri5: e and logp_out must be given together");
    CASPR_REQUIRE(((uintptr_t)w1x % 16) == 0 && ((uintptr_t)w2x % 16) == 0 && ((uintptr_t)w0 % 16) == 0 && ((uintptr_t)w3 % 16) == 0,
                  "cnf_dopri5: weights must be 16-byte aligned");
    const Dp5Layout l = dp5_layout(BT, n, max_attempts);
    CASPR_REQUIRE(ws_bytes >= l.total && ((uintptr_t)ws % 256) == 0, "cnf_dopri5: workspace of %ld bytes, 256-byte aligned, needed", l.total);
    hipStream_t st = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        caspr_set_error("cnf_dopri5: the host loop reads the device after every attempt and cannot run under stream capture");
        return CASPR_EUNSUP;
    }
    CnfDp5Args a;
    a.y_in = y_in; a.hyper = hyper; a.tcol = tcol; a.w0 = w0; a.b0 = b0; a.b1 = b1; a.b2 = b2; a.w3 = w3; a.b3 = b3;
    a.mbn_in = mbn_in; a.mbn_out = mbn_out; a.w1x = (const unsigned char *)w1x; a.w2x = (const unsigned char *)w2x;
    a.e = e; a.logp_in = logp_in; a.logp_out = logp_out;
    a.y_out = y_out; a.ldh = ldh; a.n = n; a.reverse = reverse & 1; a.t_end = t_end; a.rtol = rtol; a.atol = atol;
    a.max_attempts = max_attempts;
    unsigned char *wsb = (unsigned char *)ws;
    a.frames = (Dp5Frame *)(wsb + l.frames);
    a.part = (double *)(wsb + l.part);
    a.running = (int *)(wsb + l.running);
    a.pts = (float *)(wsb + l.pts);
    a.trace = trace;
    a.counters = counters;
    static CasprLdsOptIn optin_s, optin_d;
    const hipError_t err = e ? caspr_lds_opt_in(optin_d, (const void *)cnf_dp5_kernel<true>, DP_LDS)
                             : caspr_lds_opt_in(optin_s, (const void *)cnf_dp5_kernel<false>, DP_LDS);
    if (err != hipSuccess) {
        caspr_set_error("cnf_dopri5: hipFuncSetAttribute failed: %s", hipGetErrorString(err));
        return CASPR_ELAUNCH;
    }
    int *h_running = nullptr;
    if (hipHostMalloc((void **)&h_running, sizeof(int), hipHostMallocDefault) != hipSuccess) {
        caspr_set_error("cnf_dopri5: hipHostMalloc failed");
        return CASPR_ELAUNCH;
    }
    hipError_t he = hipMemsetAsync(a.running, 0, ((long)max_attempts + 3) * sizeof(int), st);
    if (he == hipSuccess) he = hipMemsetAsync(trace, 0, (long)BT * (DP_TRACE_HEAD + DP_TRACE_ROW * (long)max_attempts) * sizeof(float), st);
    int running = 1, rc = CASPR_OK;
    // launch L = 0, 1: initial-step selection; L >= 2: decide attempt L - 3, run attempt L - 2; L = max_attempts + 2 decides only
    for (int L = 0; he == hipSuccess && L <= max_attempts + 2; ++L) {
        a.launch = L;
        a.last = L == max_attempts + 2;
        if (e) cnf_dp5_kernel<true><<<dim3(ceil_div(n, XC_COLS / 2), BT), dim3(256), DP_LDS, st>>>(a);
        else cnf_dp5_kernel<false><<<dim3(ceil_div(n, XC_COLS), BT), dim3(256), DP_LDS, st>>>(a);
        he = hipGetLastError();
        if (he != hipSuccess || L < 3) continue;       // no frame retires before the first decision
        // one small pinned read per attempt: the frames that launch L left running
        he = hipMemcpyAsync(h_running, a.running + L, sizeof(int), hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he != hipSuccess) break;
        running = *h_running;
        if (running == 0) break;
    }
    (void)hipHostFree(h_running);
    if (he != hipSuccess) {
        caspr_set_error("cnf_dopri5: %s", hipGetErrorString(he));
        return CASPR_ELAUNCH;
    }
    if (running != 0) {
        caspr_set_error("cnf_dopri5: %d of %d frames did not reach t_end within max_attempts = %d (rtol %g, atol %g)", running, BT, max_attempts,
                        (double)rtol, (double)atol);
        rc = CASPR_ENOCONV;
    }
    return rc;
}
