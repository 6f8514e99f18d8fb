// ode_dp5_f16x3w.hip -- the point-CNF SAMPLING solve integrated to a TOLERANCE (adaptive Dormand-Prince 5(4), error control per frame)
// on THREE f16 products per f32 product (config.cnf_dp5_split = "f16x3"): the launch protocol of ode_dp5.hip around the evaluation of
// ode_f16x3w.hip.  The loop's shared pieces are ONE text with ode_dp5.hip (dp5.h: frame state, slot sum, publication, block
// reduction, workspace and host driver; dp5_rules.h: the controller's rules; dp5_tables.inc: the tableau); the evaluation is shared
// with ode_f16x3w.hip as text (ode_h3w.h, ode_h3w_setup.inc, ode_h3w_ring.inc, ode_h3w_eval.inc); read their headers first, this one
// lists what is particular to the combination.
//
//  * evaluation: cnf_rk4_h3w_kernel's stage body -- 128 points per workgroup, a wave owns 32 points and all 512 units, layer
//    1's 256 accumulators in the hand-managed accumulator file (the f16 planes kept there during layer 2), the 8-deep LDS-DMA weight
//    ring with vmcnt(24) piece barriers, the 2^4 activation scale and the weight shifts behind the pack_cnf_h3 packs, the explicit
//    subnormal flush, v_max3_f32 range tracking.  The stage loop is `#pragma unroll 1` with ONE copy of the body: the accumulator-move
//    and MFMA counts are those of the RK4 kernel (audit.audit_cnf_dp5_h3w).  The piece sequence keeps running across the stages of a
//    launch (128 pieces a stage, a multiple of the ring: the last pieces of a stage prefetch the first of the next).  There is ONE
//    text; of its two instruction streams (same values, same bits) this kernel selects the older with two switches: the f32
//    compare-and-select flush and one M0 write per LDS-DMA instruction (audit_cnf_dp5_h3w asks for that), where the RK4 kernel flushes
//    on the f16 word (xh_flush_word) and writes M0 and the source address once per piece.  Clearing the switches needs this kernel's
//    register budget rechecked (.vgpr_count 488 of 512; the word flush holds one more VGPR), the audit's rule changed, and a timing;
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
// This kernel compiles the older of the two instruction streams the shared text carries (ode_h3w.h), in every build flavour, and has
// no phase stamps
#define XH_OLD_FLUSH 1
#define XH_OLD_DMA 1
#define XH_NO_FLUSH1 0
#define XH_NO_FLUSH2 0
#define XH_STAMP(i)
#include "ode_h3w.h"
#include "dp5.h"

// the tableau (dp5_tables.inc), in this file's constant memory as DPH_BETA, DPH_ALPHA, DPH_CERR, DPH_CMID
#define DP5_TAB(x) DPH_##x
#include "dp5_tables.inc"

#define DPH_LDS (XH_LDS + 16 * 8)
#define DPH_PT_FLOATS 15     // carry-over floats of a point in the workspace (dp5.h: a slot per 128-point workgroup): 5 quantities x 3
#define DPH_GUARD 2u         // the status word's bit of this kernel (cnf_rk4_h3w_kernel sets bit 0)

struct CnfDp5H3Args {
    const float *y_in, *hyper, *tcol, *w0, *b0, *b1, *b2, *w3, *b3, *mbn_in, *mbn_out;
    const unsigned char *w1x, *w2x;   // the pack_cnf_h3 packs
    float *y_out;
    int ldh, n, reverse;
    float t_end, rtol, atol;
    int launch;                   // 0: f(t0, y0); 1: f(t0 + h0, y0 + h0 f0); L >= 2: decide attempt L - 3, run attempt L - 2
    int last;                     // the attempt budget is used up: decide only
    int max_attempts;
    Dp5Frame *frames;             // [2][BT]
    double *part;                 // [2][BT][workgroups of a frame][4]: sum of squares, points the range guard caught, second sum (launch 0), 0
    float *pts;                   // [BT][5][3][n]
    int *running;                 // [launch]: frames that did not retire in that launch
    float *trace;                 // [BT][DP5_TRACE_HEAD + DP5_TRACE_ROW * max_attempts]
    int *counters;                // [BT][4]: accepted, rejected, evaluations, finished (1; 3: retired by the range guard)
    unsigned *status;             // one word per solve, zeroed in front of launch 0: DPH_GUARD set <-> the range guard tripped
};

__global__ __launch_bounds__(256, 1) void cnf_dp5_h3w_kernel(CnfDp5H3Args a)
{
    const int tid = threadIdx.x, lane0 = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bt = blockIdx.y, BT = gridDim.y, nwg = gridDim.x;
    const int col = blockIdx.x * XH_PTS + 32 * wave + (lane0 & 31);
    const bool cvalid = col < a.n;
    const int ccol = cvalid ? col : a.n - 1;
    // lanes l and l + 32 hold the same point: the lower one owns it (counts it in the norms, stores its carry-over and its output)
    const bool own = cvalid && lane0 < 32;
    float *pp = a.pts + (long)bt * DPH_PT_FLOATS * a.n + ccol;             // quantity q, component d at pp[q * qs + d * n]
    const long qs = 3L * a.n;

    const int Lc = a.launch, par = Lc & 1;
    const Dp5Frame *fprev = a.frames + (long)(par ^ 1) * BT + bt;
    Dp5Frame *fnext = a.frames + (long)par * BT + bt;
    const bool lead = blockIdx.x == 0 && tid == 0;
    const double sgn = a.reverse ? -1.0 : 1.0;
    const double tq1 = a.reverse ? 0.0 : (double)a.t_end;       // where the solve ends, in solver time
    Dp5Frame st;
    DP5_FRAME_LOAD_OR_RETURN(st, fprev, fnext, Lc, lead, a.reverse, a.t_end);

    float s[3], f0[3] = {0.f, 0.f, 0.f};
    if (Lc == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            float v = a.y_in[((long)bt * a.n + ccol) * 3 + d];
            if (a.mbn_in) v = mbn_apply(a.mbn_in, d, a.reverse, v);
            s[d] = v;
        }
    } else {
        // (A lane that does not own its point -- the upper half of a wave, a column past n clamped to point n - 1 -- may read these two
        // AFTER the point's owner, possibly in another wave, has committed the accepted step to them further down.  Harmless, and only
        // because of what follows: y and f0 matter after a REJECTED attempt, when nobody writes them, or at the interpolant, which the
        // owner alone computes; on accept every lane replaces them by y_new and k7, which this launch only reads.)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            s[d] = pp[DP5_Y * qs + (long)d * a.n];
            f0[d] = pp[DP5_F0 * qs + (long)d * a.n];
        }
    }

    // ---- the frame's sums of the previous launch: its workgroups' slots added in slot order, the same in every workgroup of the frame
    DP5_SLOT_SUM(S, a.part, Lc, BT, bt, nwg)
    const double nx = 3.0 * (double)a.n;
    float *trow = a.trace + (long)bt * (DP5_TRACE_HEAD + DP5_TRACE_ROW * a.max_attempts);
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
                float *tr = trow + DP5_TRACE_HEAD + DP5_TRACE_ROW * (Lc - 3);
                tr[0] = (float)(sgn * st.t); tr[1] = dt; tr[2] = __uint_as_float(0x7fc00000u); tr[3] = 0.f; tr[4] = 0.f;
                ++st.nrej;
            }
            st.done = 1;
            DP5_PUBLISH(fnext, st, a.counters, bt, 3, false, a.running + Lc);
        }
        return;
    }
    if (Lc == 1) {
        // _select_initial_step: d0 = rms(y / scale), d1 = rms(f0 / scale)
        const double d0 = sqrt(S[0] / nx), d1 = sqrt(S[2] / nx);
        const double h0 = dp5_h0(d0, d1);
        st.d0 = (float)d0;
        st.d1 = (float)d1;
        st.h0 = (float)h0;
        hstep = st.h0;
    } else if (Lc == 2) {
        const float d2 = (float)(sqrt(S[0] / nx) / (double)st.h0);
        st.d2 = d2;
        dt = DP5_FIRST_DT(st.d1, d2, st.h0);
        st.dt0 = dt;
        if (lead) {
            trow[0] = st.d0; trow[1] = st.d1; trow[2] = d2; trow[3] = st.h0; trow[4] = dt; trow[5] = trow[6] = trow[7] = 0.f;
        }
        hstep = dt;
    } else if (Lc >= 3) {
        // ---- decide attempt Lc - 3: ratio = mean((err / tol)^2), accept iff <= 1
        const float r = (float)(S[0] / nx);
        const bool accept = r <= 1.f;
        const float dt_next = dp5_next_dt(r, dt);
        if (lead) {
            float *tr = trow + DP5_TRACE_HEAD + DP5_TRACE_ROW * (Lc - 3);
            tr[0] = (float)(sgn * st.t); tr[1] = dt; tr[2] = r; tr[3] = 0.f; tr[4] = accept ? 1.f : 0.f;
        }
        if (accept) {
            ++st.nacc;
            const double t1s = st.t + (double)dt;
            float yn[3], k7[3], ym[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                yn[d] = pp[DP5_YN * qs + (long)d * a.n];
                k7[d] = pp[DP5_K7 * qs + (long)d * a.n];
                ym[d] = pp[DP5_YM * qs + (long)d * a.n];
            }
            if (t1s >= tq1) {
                // ---- the step went past the end: the 4th-order interpolant at the end time (y_new itself when it lands on it)
                if (own) {
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        double v = (double)yn[d];
                        if (t1s != tq1) {
                            // (the text of dp5_interp / dp5_interp_at, dp5_rules.h: through the functions this kernel's register
                            // allocation changes -- 488 of 512 VGPRs)
                            DP5_INTERP_COEFS(s[d], yn[d], ym[d], f0[d], k7[d], dt)
                            const double xx = (tq1 - st.t) / (t1s - st.t);
                            v = DP5_INTERP_HORNER(xx);
                        }
                        float o = (float)v;
                        if (a.mbn_out) o = mbn_apply(a.mbn_out, d, a.reverse, o);
                        a.y_out[((long)bt * a.n + col) * 3 + d] = o;
                    }
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
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                s[d] = yn[d];
                f0[d] = k7[d];
                if (own) {
                    pp[DP5_Y * qs + (long)d * a.n] = s[d];
                    pp[DP5_F0 * qs + (long)d * a.n] = f0[d];
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
                DP5_PUBLISH(fnext, st, a.counters, bt, 0, true, a.running + Lc);
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
        DP5_PUBLISH(fnext, st, a.counters, bt, 0, true, a.running + Lc);
    }

    // ================= the evaluation of cnf_rk4_h3w_kernel (ode_f16x3w.hip), shared with it as text =================
#include "ode_h3w_setup.inc"
    // (the table registers: the same text in cnf_rk4_h3w_kernel, see ode_h3w_setup.inc)
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
#include "ode_h3w_ring.inc"
    double *s_red = (double *)(s_g3 + 8);           // [4 waves][4] partial sums: the 16 * 8 bytes of DPH_LDS past XH_LDS

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
            // stage input y + dt * sum_i beta[row][i] k_i
#define XH_STAGE_INPUT                                                                                        \
    _Pragma("unroll") for (int d = 0; d < 3; ++d) {                                                           \
        float bacc = 0.f;                                                                                     \
        _Pragma("unroll") for (int i = 0; i < 6; ++i) bacc += DPH_BETA[row][i] * k[i][d];                     \
        ys[d] = row == 0 ? s[d] : s[d] + hstep * bacc;                                                        \
    }
#include "ode_h3w_eval.inc"

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
                pp[DP5_Y * qs + (long)d * a.n] = s[d];
                pp[DP5_F0 * qs + (long)d * a.n] = k[1][d];
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
                pp[DP5_YN * qs + (long)d * a.n] = ys[d];
                pp[DP5_K7 * qs + (long)d * a.n] = k[6][d];
                pp[DP5_YM * qs + (long)d * a.n] = ym;
            }
        }
    }
    DP5_BLOCK_REDUCE(v, 3, s_red, a.part + (((long)par * BT + bt) * nwg + blockIdx.x) * 4, tid, lane0, wave);
}

extern "C" long caspr_cnf_dopri5_h3_ws_bytes(int BT, int n, int max_attempts) { return dp5_ws_bytes(BT, n, max_attempts, XH_PTS, DPH_PT_FLOATS); }

extern "C" int caspr_cnf_dopri5_h3_f32(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0,
                                       const float *b0, const void *w1h, const float *b1, const void *w2h, const float *b2,
                                       const float *w3, const float *b3, int H, float t_end, float rtol, float atol, int max_attempts,
                                       int reverse, const float *mbn_in, const float *mbn_out, unsigned *status, float *y_out, int BT,
                                       int n, void *ws, long ws_bytes, float *trace, int32_t *counters, void *stream)
{
    const int bad = dp5_check("cnf_dopri5_h3", y_in && hyper && tcol && w0 && b0 && w1h && b1 && w2h && b2 && w3 && b3 && y_out && ws && trace && counters && status,
                              true, H, XC_H, BT, n, max_attempts, ldh, rtol, atol, t_end, w0, w1h, w2h, w3, ws, ws_bytes,
                              dp5_ws_bytes(BT, n, max_attempts, XH_PTS, DPH_PT_FLOATS));
    if (bad) return bad;
    const Dp5Layout l = dp5_layout(BT, n, max_attempts, XH_PTS, DPH_PT_FLOATS);
    hipStream_t st = (hipStream_t)stream;
    CnfDp5H3Args a;
    a.y_in = y_in; a.hyper = hyper; a.tcol = tcol; a.w0 = w0; a.b0 = b0; a.b1 = b1; a.b2 = b2; a.w3 = w3; a.b3 = b3;
    a.mbn_in = mbn_in; a.mbn_out = mbn_out; a.w1x = (const unsigned char *)w1h; a.w2x = (const unsigned char *)w2h;
    a.y_out = y_out; a.ldh = ldh; a.n = n; a.reverse = reverse & 1; a.t_end = t_end; a.rtol = rtol; a.atol = atol;
    a.max_attempts = max_attempts;
    unsigned char *wsb = (unsigned char *)ws;
    a.frames = (Dp5Frame *)(wsb + l.frames);
    a.part = (double *)(wsb + l.part);
    a.running = (int *)(wsb + l.running);
    a.pts = (float *)(wsb + l.pts);
    a.trace = trace;
    a.counters = counters;
    a.status = status;
    static CasprLdsOptIn optin;
    return dp5_run("cnf_dopri5_h3", optin, (const void *)cnf_dp5_h3w_kernel, DPH_LDS, BT, max_attempts, rtol, atol, a.running, trace, status, st,
                   [&](int L, bool last) {
                       a.launch = L;
                       a.last = last;
                       cnf_dp5_h3w_kernel<<<dim3(ceil_div(n, XH_PTS), BT), dim3(256), DPH_LDS, st>>>(a);
                   });
}
