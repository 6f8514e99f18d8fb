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
// What this loop shares with cnf_dp5_h3w_kernel (ode_dp5_f16x3w.hip) is in dp5.h (frame state, slot sum, publication, block
// reduction, workspace layout, host driver), the controller's rules in dp5_rules.h, the tableau in dp5_tables.inc; the two-tensor
// norms are this file's own.
#include "ode_x6.h"
#include "dp5.h"

// the tableau (dp5_tables.inc), in this file's constant memory as DP_BETA, DP_ALPHA, DP_CERR, DP_CMID
#define DP5_TAB(x) DP_##x
#include "dp5_tables.inc"

#define DP_LDS (XC_LDS + 16 * 8)
// workspace (dp5.h): slots for the divergence variant's workgroup count, the larger one (32 points each); 5 x 4 carry-over floats a point
#define DP_WG_PTS (XC_COLS / 2)
#define DP_PT_FLOATS 20

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
    float *trace;                 // [BT][DP5_TRACE_HEAD + DP5_TRACE_ROW * max_attempts]
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
    float *pp = a.pts + ((long)bt * DP_PT_FLOATS + g0) * a.n + ccol;      // quantity q at pp[q * 4 * n]
    const long qs = 4L * a.n;

    const int Lc = a.launch, par = Lc & 1;
    const Dp5Frame *fprev = a.frames + (long)(par ^ 1) * BT + bt;
    Dp5Frame *fnext = a.frames + (long)par * BT + bt;
    const bool lead = blockIdx.x == 0 && tid == 0;
    const double sgn = a.reverse ? -1.0 : 1.0;
    const double tq1 = a.reverse ? 0.0 : (double)a.t_end;       // where the solve ends, in solver time
    Dp5Frame st;
    DP5_FRAME_LOAD_OR_RETURN(st, fprev, fnext, Lc, lead, a.reverse, a.t_end);

    float s = 0.f, f0 = 0.f;
    if (Lc == 0) {
        float v = a.y_in[((long)bt * a.n + ccol) * 3 + sd];
        if (a.mbn_in) v = mbn_apply(a.mbn_in, sd, a.reverse, v);
        if (g0 == 3) v = 0.f;
        if (DIV) {
            if (tg0) v = a.e[((long)bt * a.n + ccol) * 3 + sd];
            else if (g0 == 3) {
                float lp = a.logp_in ? a.logp_in[(long)bt * a.n + ccol] : 0.f;
                if (a.mbn_in) lp = mbn_shift_logp(a.mbn_in, a.reverse, lp);
                v = lp;
            }
        }
        s = v;
    } else {
        if (own) {
            s = pp[DP5_Y * qs];
            f0 = pp[DP5_F0 * qs];
        }
        if (DIV && tg0) s = a.e[((long)bt * a.n + ccol) * 3 + sd];
    }

    // ---- the frame's sums of squares of the previous launch: its workgroups' slots added in slot order, the same in every
    // workgroup of the frame
    DP5_SLOT_SUM(S, a.part, Lc, BT, bt, nwg)
    const double nx = 3.0 * (double)a.n, nl = (double)a.n;
    float *trow = a.trace + (long)bt * (DP5_TRACE_HEAD + DP5_TRACE_ROW * a.max_attempts);
    float dt = st.dt, hstep = 0.f;
    if (Lc == 1) {
        // _select_initial_step: d0 = max over tensors of rms(y / scale), d1 of rms(f0 / scale)
        const double d0x = sqrt(S[0] / nx), d0l = sqrt(S[1] / nl), d1x = sqrt(S[2] / nx), d1l = sqrt(S[3] / nl);
        const double d0 = fmax(d0x, d0l), d1 = fmax(d1x, d1l);
        const double h0 = dp5_h0(d0, d1, [=] { return fmax(dp5_quot(d0x, d1x), dp5_quot(d0l, d1l)); });
        st.d0 = (float)d0;
        st.d1 = (float)d1;
        st.h0 = (float)h0;
        hstep = st.h0;
    } else if (Lc == 2) {
        const float d2 = (float)(fmax(sqrt(S[0] / nx), sqrt(S[1] / nl)) / (double)st.h0);
        st.d2 = d2;
        dt = DP5_FIRST_DT(st.d1, d2, st.h0);
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
        const float dt_next = dp5_next_dt(r, dt);
        if (lead) {
            float *tr = trow + DP5_TRACE_HEAD + DP5_TRACE_ROW * (Lc - 3);
            tr[0] = (float)(sgn * st.t); tr[1] = dt; tr[2] = r0; tr[3] = r1; tr[4] = accept ? 1.f : 0.f;
        }
        if (accept) {
            ++st.nacc;
            const double t1s = st.t + (double)dt;
            float yn = 0.f, k7 = 0.f, ym = 0.f;
            if (own) {
                yn = pp[DP5_YN * qs];
                k7 = pp[DP5_K7 * qs];
                ym = pp[DP5_YM * qs];
            }
            if (t1s >= tq1) {
                // ---- the step went past the end: the 4th-order interpolant at the end time (y_new itself when it lands on it)
                double v = (double)yn;
                if (t1s != tq1) v = dp5_interp_at(dp5_interp(s, yn, ym, f0, k7, dt), (tq1 - st.t) / (t1s - st.t));
                float o = (float)v;
                if (own && g0 == 3) {
                    if (a.mbn_out) o = mbn_shift_logp(a.mbn_out, a.reverse, o);
                    a.logp_out[(long)bt * a.n + col] = o;
                }
                if (own && g0 < 3) {
                    if (a.mbn_out) o = mbn_apply(a.mbn_out, sd, a.reverse, o);
                    a.y_out[((long)bt * a.n + col) * 3 + sd] = o;
                }
                if (lead) {
                    st.t = t1s;
                    st.dt = dt_next;
                    st.done = 1;
                    DP5_PUBLISH(fnext, st, a.counters, bt, 1, false, a.running + Lc);
                }
                return;
            }
            // commit: (t, y, f0) <- (t + dt, y_new, k7)
            st.t = t1s;
            if (own) {                                          // (tangent lanes keep e)
                s = yn;
                f0 = k7;
                pp[DP5_Y * qs] = s;
                pp[DP5_F0 * qs] = f0;
            }
        } else {
            ++st.nrej;
        }
        dt = dt_next;
        hstep = dt;
        if (a.last) {
            if (lead) {
                st.dt = dt;
                DP5_PUBLISH(fnext, st, a.counters, bt, 0, true, a.running + Lc);
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
            pp[DP5_Y * qs] = s;
            pp[DP5_F0 * qs] = k[1];
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
            pp[DP5_YN * qs] = ylast;
            pp[DP5_K7 * qs] = k[6];
            pp[DP5_YM * qs] = ym;
        }
    }
    DP5_BLOCK_REDUCE(v, 4, s_red, a.part + (((long)par * BT + bt) * nwg + blockIdx.x) * 4, tid, lane0, wave);
    if (lead) {
        st.dt = dt;
        st.nfe += nst;
        DP5_PUBLISH(fnext, st, a.counters, bt, 0, true, a.running + Lc);
    }
}

extern "C" long caspr_cnf_dopri5_ws_bytes(int BT, int n, int max_attempts) { return dp5_ws_bytes(BT, n, max_attempts, DP_WG_PTS, DP_PT_FLOATS); }

extern "C" int caspr_cnf_dopri5_f32(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0,
                                    const float *b0, const void *w1x, const float *b1, const void *w2x, const float *b2,
                                    const float *w3, const float *b3, int H, float t_end, float rtol, float atol, int max_attempts,
                                    int reverse, const float *mbn_in, const float *mbn_out, const float *e, const float *logp_in,
                                    float *logp_out, float *y_out, int BT, int n, void *ws, long ws_bytes, float *trace,
                                    int32_t *counters, void *stream)
{
    const int bad = dp5_check("cnf_dopri5", y_in && hyper && tcol && w0 && b0 && w1x && b1 && w2x && b2 && w3 && b3 && y_out && ws && trace && counters,
                              (e == nullptr) == (logp_out == nullptr), H, XC_H, BT, n, max_attempts, ldh, rtol, atol, t_end, w0, w1x, w2x, w3, ws, ws_bytes,
                              dp5_ws_bytes(BT, n, max_attempts, DP_WG_PTS, DP_PT_FLOATS));
    if (bad) return bad;
    const Dp5Layout l = dp5_layout(BT, n, max_attempts, DP_WG_PTS, DP_PT_FLOATS);
    hipStream_t st = (hipStream_t)stream;
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
    return dp5_run("cnf_dopri5", e ? optin_d : optin_s, e ? (const void *)cnf_dp5_kernel<true> : (const void *)cnf_dp5_kernel<false>, DP_LDS, BT,
                   max_attempts, rtol, atol, a.running, trace, nullptr, st, [&](int L, bool last) {
                       a.launch = L;
                       a.last = last;
                       if (e) cnf_dp5_kernel<true><<<dim3(ceil_div(n, XC_COLS / 2), BT), dim3(256), DP_LDS, st>>>(a);
                       else cnf_dp5_kernel<false><<<dim3(ceil_div(n, XC_COLS), BT), dim3(256), DP_LDS, st>>>(a);
                   });
}
