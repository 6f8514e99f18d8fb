// ode_latent_dp5.hip -- the latent ODE (latent_ode_model.py:45-70) integrated to a TOLERANCE: adaptive Dormand-Prince 5(4) as
// torchdiffeq 0.0.1 runs it (oracle.model.dopri5_solve restates it), the whole solve in ONE launch with the step control on the
// device.  ONE difference from the reference, the one the point-CNF solve of ode_dp5.hip makes: norms and decisions are taken PER
// SEQUENCE (row of B), not over the whole (B, D) tensor -- a sequence's codes are what the reference computes when it is called
// on that sequence alone, whatever batch surrounds it.
//
// The evaluation is the one of latent_rk4_kernel (ode.hip), copied: one 512-thread workgroup advects up to 16 sequences as the 16
// columns of the f32 MFMA tile, each wave owns 64 of the 512 hidden units and streams its packed weights from L2 once per
// evaluation for all columns, the hidden state is an LDS B-tile.  What differs is the loop around it:
//  * the dynamics do not read t, so every column carries ITS OWN t, dt, next-stamp cursor and finished flag.  Attempts run in
//    lockstep (six evaluations each, the seventh stage is the next attempt's first: FSAL), every column with its own dt; a column
//    that has emitted its last stamp, and a padding column, runs with dt = 0 and is neither read nor written by the control phase.
//    MFMA columns are independent, so a column never sees its neighbours;
//  * the control phase is wave-local: wave w owns columns 2w and 2w + 1, lane d holds component d.  The sum of squares of a norm
//    is an f64 xor-butterfly over the 64 lanes -- one fixed order, every lane ends with the same bits -- so all lanes take the
//    identical accept / reject decision and the identical next dt (f32, as ode_dp5.hip), without atomics or a designated thread;
//  * steps are not clipped at the output stamps: after an accepted step the wave emits every stamp up to the step's end from the
//    4th-order interpolant (y_new itself at the step's end, z0 at stamps equal to times[0]); repeated stamps evaluate the same
//    polynomial at the same abscissa and give the same bits;
//  * the loop ends when all 16 columns have finished or max_attempts rounds have run.  The exit test reads the 16 finished flags
//    from LDS behind a barrier: workgroup-uniform, every thread passes the same barriers.  A sequence that has not finished gets
//    finished = 0 and NaN in the rows it did not reach.
// No inter-workgroup communication, no co-residency requirement, no host read: the launch can be captured.
// A sequence's output, trace and counters are bit-identical whichever column, workgroup or batch it sits in.
// The controller's rules (next step, initial step, interpolant) are dp5_rules.h's and the tableau dp5_tables.inc's: one text with
// the two point-CNF solves.
#include "ode_latent_dp5.h"
#include "dp5_rules.h"

// the tableau (dp5_tables.inc), in this file's constant memory as LDP_BETA, LDP_CERR, LDP_CMID (the dynamics do not read t: no stage times)
#define DP5_TAB(x) LDP_##x
#define DP5_TAB_NO_ALPHA
#include "dp5_tables.inc"

// the hooks of ode_latent_dp5_eval.inc: the solve keeps y_new (row 7 of the stage inputs) and no layer rows
#define LDP_EVAL_IN(row, i, d, c, v) if (row == 7) s_yn[i] = v;
#define LDP_EVAL_ROW(l, r, v)

// TAPE: the solve under autograd (caspr_latent_dopri5_tape_f32).  The same text and the same bits in out / trace / counters; every
// accepted step n of a sequence also leaves its start state z_n in tape_z (B, max_steps, D) and its size in tape_dt (B, max_steps),
// which is all the reverse sweep (ode_latent_dp5_adjoint.inc) needs to rebuild the step.  A sequence whose next accepted step would
// not fit stops like one that used up max_attempts: finished = 0, NaN in the rows it did not reach; that attempt is not counted.
template <bool TAPE>
__global__ __launch_bounds__(512) void latent_dp5_kernel(const float *__restrict__ z0, int ldz, const float *__restrict__ times,
                                                         int B, int Tu, int D, int H, float rtol, float atol, int max_attempts,
                                                         const float *__restrict__ w0p, const float *__restrict__ b0,
                                                         const float *__restrict__ w1p, const float *__restrict__ b1,
                                                         const float *__restrict__ w2p, const float *__restrict__ b2,
                                                         const float *__restrict__ w3p, const float *__restrict__ b3,
                                                         float *__restrict__ out, float *__restrict__ trace, int *__restrict__ counters,
                                                         float *__restrict__ tape_z, float *__restrict__ tape_dt, int max_steps)
{
    // B-tiles: stage input (64 x 16, padded to 32 k-rows of 4), two hidden buffers (512 x 16)
    __shared__ __attribute__((aligned(16))) float s_in[16 * LDP_NCOL * 4];
    __shared__ __attribute__((aligned(16))) float s_h1[128 * LDP_NCOL * 4], s_h2[128 * LDP_NCOL * 4];
    __shared__ float s_z[LDP_EL], s_yn[LDP_EL], s_k[7][LDP_EL];      // state, y_new, k1..k7; element (d, c) at d * 16 + c
    __shared__ float s_dt[LDP_NCOL];                                  // the step of the next evaluations, per column (0: masked)
    __shared__ int s_done[LDP_NCOL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, j = lane & 15;
    const int b0i = blockIdx.x * LDP_NCOL;
    const int KC0 = 2 * ((D + 31) / 32), KCH = 2 * ((H + 31) / 32);
    const int RTH = (H + 15) / 16, RTD = (D + 15) / 16;

    for (int i = tid; i < LDP_EL; i += 512) {
        const int d = i / LDP_NCOL, c = i % LDP_NCOL;
        s_z[i] = (d < D && b0i + c < B) ? z0[(long)(b0i + c) * ldz + d] : 0.f;
        s_yn[i] = 0.f;
#pragma unroll
        for (int q = 0; q < 7; ++q) s_k[q][i] = 0.f;
    }
    for (int i = tid; i < 16 * LDP_NCOL * 4; i += 512) s_in[i] = 0.f;   // K padding rows stay zero
    for (int i = tid; i < 128 * LDP_NCOL * 4; i += 512) { s_h1[i] = 0.f; s_h2[i] = 0.f; }
    if (tid < LDP_NCOL) { s_dt[tid] = 0.f; s_done[tid] = b0i + tid < B ? 0 : 1; }
    __syncthreads();

#include "ode_latent_dp5_eval.inc"

    // ---- the control state of this wave's two columns (wave-uniform), lane = component d
    const bool dv = lane < D;
    const int ei[2] = {lane * LDP_NCOL + 2 * wave, lane * LDP_NCOL + 2 * wave + 1};   // this lane's element of either column
    const float t_first = times[0];
    const double dD = (double)D;
    double tc[2] = {0.0, 0.0};                       // solver time, relative to times[0]
    float dtc[2] = {0.f, 0.f}, h0c[2] = {0.f, 0.f}, d0c[2] = {0.f, 0.f}, d1c[2] = {0.f, 0.f};
    int cur[2] = {0, 0}, nacc[2] = {0, 0}, nrej[2] = {0, 0};
    bool fin[2], valid[2], over[2] = {false, false};         // over: the tape is full (TAPE only)
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) { valid[cc] = b0i + 2 * wave + cc < B; fin[cc] = !valid[cc]; }

    // the stamps of column cc up to time t1 (inclusive) from the interpolant p (dp5_rules.h) of the step [t0, t1] (lin == false:
    // every stamp takes y1 -- the rows at times[0])
    auto emit = [&](int cc, double t0, double t1, bool lin, const Dp5Interp &p, float y1) {
        float *orow = out + (long)(b0i + 2 * wave + cc) * Tu * D;
        int c1 = cur[cc];
        while (c1 < Tu) {                            // the stamps are ascending: the ones <= t1 are a prefix of the rest
            const int i = c1 + lane;
            const bool le = i < Tu && (double)(times[i] - t_first) <= t1;
            const unsigned long long m = __ballot(le);
            const int n = m == ~0ull ? 64 : __builtin_ctzll(~m);
            c1 += n;
            if (n < 64) break;
        }
        for (int i = cur[cc]; i < c1; ++i) {
            const double tn = (double)(times[i] - t_first);     // latent_ode_model.py:58
            double v = (double)y1;
            if (lin && tn != t1) v = dp5_interp_at(p, (tn - t0) / (t1 - t0));
            if (dv) orow[(long)i * D + lane] = (float)v;
        }
        cur[cc] = c1;
    };

    // ---- _select_initial_step(order = 4): f0 = f(z0); d0, d1; h0; f1 = f(z0 + h0 f0); d2; first dt
    write_in(0);
    dyn(s_k[0]);
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
        if (!valid[cc]) continue;
        const float z = s_z[ei[cc]], f0 = s_k[0][ei[cc]];
        const float sc = atol + fabsf(z) * rtol;
        const float a = z / sc, b = f0 / sc;
        const double S0 = ldp_wave_sum(dv ? (double)a * (double)a : 0.0), S1 = ldp_wave_sum(dv ? (double)b * (double)b : 0.0);
        const double d0 = sqrt(S0 / dD), d1 = sqrt(S1 / dD);
        const double h0 = dp5_h0(d0, d1);
        d0c[cc] = (float)d0;
        d1c[cc] = (float)d1;
        h0c[cc] = (float)h0;
        if (lane == 0) s_dt[2 * wave + cc] = h0c[cc];
    }
    __syncthreads();
    write_in(1);
    dyn(s_k[1]);
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
        if (!valid[cc]) continue;
        const int c = 2 * wave + cc;
        const float z = s_z[ei[cc]], f0 = s_k[0][ei[cc]], f1 = s_k[1][ei[cc]];
        const float sc = atol + fabsf(z) * rtol;
        const float a = (f1 - f0) / sc;
        const double S = ldp_wave_sum(dv ? (double)a * (double)a : 0.0);
        const float d2 = (float)(sqrt(S / dD) / (double)h0c[cc]);
        dtc[cc] = dp5_first_dt(d1c[cc], d2, h0c[cc]);
        if (trace && lane < LDP_TRACE_HEAD) {
            const float hd[LDP_TRACE_HEAD] = {d0c[cc], d1c[cc], d2, h0c[cc], dtc[cc], 0.f, 0.f, 0.f};
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < LDP_TRACE_HEAD; ++q) v = lane == q ? hd[q] : v;
            trace[(long)(b0i + c) * (LDP_TRACE_HEAD + LDP_TRACE_ROW * max_attempts) + lane] = v;
        }
        emit(cc, 0.0, 0.0, false, Dp5Interp{0.0, 0.0, 0.0, 0.0, (double)z}, z);   // the stamps equal to times[0]: z0
        fin[cc] = cur[cc] >= Tu;
        if (lane == 0) { s_dt[c] = fin[cc] ? 0.f : dtc[cc]; s_done[c] = fin[cc] ? 1 : 0; }
    }
    // masked columns (padding) keep s_dt = 0 from here on
    if (lane == 0)
#pragma unroll
        for (int cc = 0; cc < 2; ++cc)
            if (!valid[cc]) s_dt[2 * wave + cc] = 0.f;

    // ---- the attempts
    for (int att = 0;; ++att) {
        __syncthreads();
        int all = 1;
#pragma unroll
        for (int c = 0; c < LDP_NCOL; ++c) all &= s_done[c];
        if (all || att >= max_attempts) break;                           // workgroup-uniform: s_done is read behind the barrier
#pragma unroll 1
        for (int row = 2; row < 8; ++row) {
            write_in(row);
            dyn(s_k[row - 1]);
        }
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            if (fin[cc]) continue;
            const int c = 2 * wave + cc, e = ei[cc];
            const float dt = dtc[cc];
            const float z = s_z[e], yn = s_yn[e];
            float kk[7];
#pragma unroll
            for (int q = 0; q < 7; ++q) kk[q] = s_k[q][e];
            float es = 0.f, ms = 0.f;
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                if (LDP_CERR[q] != 0.f) es += LDP_CERR[q] * kk[q];
                if (LDP_CMID[q] != 0.f) ms += LDP_CMID[q] * kk[q];
            }
            const float err = dt * es;
            const float tol = atol + rtol * fmaxf(fabsf(z), fabsf(yn));
            const float qe = err / tol;
            const float r = (float)(ldp_wave_sum(dv ? (double)qe * (double)qe : 0.0) / dD);     // mean((err / tol)^2)
            const bool accept = r <= 1.f;
            const float dt_next = dp5_next_dt(r, dt);
            if constexpr (TAPE)
                if (accept && nacc[cc] >= max_steps) {
                    over[cc] = fin[cc] = true;
                    if (lane == 0) { s_dt[c] = 0.f; s_done[c] = 1; }
                    continue;
                }
            if (trace && lane < LDP_TRACE_ROW) {
                const float v = lane == 0 ? (float)tc[cc] : lane == 1 ? dt : lane == 2 ? r : (accept ? 1.f : 0.f);
                trace[(long)(b0i + c) * (LDP_TRACE_HEAD + LDP_TRACE_ROW * max_attempts) + LDP_TRACE_HEAD + LDP_TRACE_ROW * att + lane] = v;
            }
            if (accept) {
                if constexpr (TAPE) {
                    float *tz = tape_z + ((long)(b0i + c) * max_steps + nacc[cc]) * D;
                    if (dv) tz[lane] = z;
                    if (lane == 0) tape_dt[(long)(b0i + c) * max_steps + nacc[cc]] = dt;
                }
                ++nacc[cc];
                const double t0 = tc[cc], t1 = tc[cc] + (double)dt;
                const float ymid = z + dt * ms;
                emit(cc, t0, t1, true, dp5_interp(z, yn, ymid, kk[0], kk[6], dt), yn);
                tc[cc] = t1;
                if (dv) { s_z[e] = yn; s_k[0][e] = kk[6]; }              // commit; FSAL
                fin[cc] = cur[cc] >= Tu;
            } else
                ++nrej[cc];
            dtc[cc] = dt_next;
            if (lane == 0) { s_dt[c] = fin[cc] ? 0.f : dt_next; s_done[c] = fin[cc] ? 1 : 0; }
        }
    }

    // ---- counters; NaN in the rows a sequence did not reach; zero in the trace rows it did not use
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
        if (!valid[cc]) continue;
        const long b = b0i + 2 * wave + cc;
        const int na = nacc[cc] + nrej[cc];
        if (lane < 4) counters[b * 4 + lane] = lane == 0 ? nacc[cc] : lane == 1 ? nrej[cc] : lane == 2 ? 2 + 6 * na : (fin[cc] && !(TAPE && over[cc]) ? 1 : 0);
        if (dv)
            for (int i = cur[cc]; i < Tu; ++i) out[(b * Tu + i) * D + lane] = __builtin_nanf("");
        if (trace) {
            float *tr = trace + b * (LDP_TRACE_HEAD + LDP_TRACE_ROW * max_attempts) + LDP_TRACE_HEAD;
            for (long i = (long)LDP_TRACE_ROW * na + lane; i < (long)LDP_TRACE_ROW * max_attempts; i += 64) tr[i] = 0.f;
        }
    }
}

extern "C" int caspr_latent_dopri5_f32(const float *z0, int ldz, const float *times, int B, int Tu, int D, int H,
                                       float rtol, float atol, int max_attempts, const float *w0p, const float *b0,
                                       const float *w1p, const float *b1, const float *w2p, const float *b2,
                                       const float *w3p, const float *b3, float *out, float *trace, int32_t *counters,
                                       void *stream)
{
    CASPR_REQUIRE(z0 && times && out && counters && w0p && w1p && w2p && w3p && b0 && b1 && b2 && b3, "latent_dopri5: null pointer");
    CASPR_REQUIRE(B > 0 && Tu > 0 && max_attempts > 0 && D > 0 && H > 0 && ldz >= D, "latent_dopri5: bad sizes B=%d Tu=%d D=%d H=%d ldz=%d max_attempts=%d",
                  B, Tu, D, H, ldz, max_attempts);
    CASPR_REQUIRE(rtol > 0.f && atol > 0.f && isfinite(rtol) && isfinite(atol), "latent_dopri5: rtol and atol must be positive and finite");
    if (!(D <= 64 && H <= 512 && H % 64 == 0)) {
        caspr_set_error("latent_dopri5: unsupported sizes D=%d H=%d (need D<=64, H<=512, H %% 64 == 0)", D, H);
        return CASPR_EUNSUP;
    }
    latent_dp5_kernel<false><<<dim3(ceil_div(B, LDP_NCOL)), dim3(512), 0, (hipStream_t)stream>>>(z0, ldz, times, B, Tu, D, H, rtol, atol, max_attempts,
                                                                                                w0p, b0, w1p, b1, w2p, b2, w3p, b3, out, trace,
                                                                                                (int *)counters, nullptr, nullptr, 0);
    CASPR_CHECK_LAUNCH("latent_dopri5");
    return CASPR_OK;
}

extern "C" int caspr_latent_dopri5_tape_f32(const float *z0, int ldz, const float *times, int B, int Tu, int D, int H,
                                            float rtol, float atol, int max_attempts, int max_steps, const float *w0p, const float *b0,
                                            const float *w1p, const float *b1, const float *w2p, const float *b2,
                                            const float *w3p, const float *b3, float *out, float *trace, int32_t *counters,
                                            float *tape_z, float *tape_dt, void *stream)
{
    CASPR_REQUIRE(z0 && times && out && counters && tape_z && tape_dt && w0p && w1p && w2p && w3p && b0 && b1 && b2 && b3,
                  "latent_dopri5_tape: null pointer");
    CASPR_REQUIRE(B > 0 && Tu > 0 && max_attempts > 0 && max_steps > 0 && D > 0 && H > 0 && ldz >= D,
                  "latent_dopri5_tape: bad sizes B=%d Tu=%d D=%d H=%d ldz=%d max_attempts=%d max_steps=%d", B, Tu, D, H, ldz, max_attempts, max_steps);
    CASPR_REQUIRE(rtol > 0.f && atol > 0.f && isfinite(rtol) && isfinite(atol), "latent_dopri5_tape: rtol and atol must be positive and finite");
    if (!(D <= 64 && H <= 512 && H % 64 == 0)) {
        caspr_set_error("latent_dopri5_tape: unsupported sizes D=%d H=%d (need D<=64, H<=512, H %% 64 == 0)", D, H);
        return CASPR_EUNSUP;
    }
    latent_dp5_kernel<true><<<dim3(ceil_div(B, LDP_NCOL)), dim3(512), 0, (hipStream_t)stream>>>(z0, ldz, times, B, Tu, D, H, rtol, atol, max_attempts,
                                                                                               w0p, b0, w1p, b1, w2p, b2, w3p, b3, out, trace,
                                                                                               (int *)counters, tape_z, tape_dt, max_steps);
    CASPR_CHECK_LAUNCH("latent_dopri5_tape");
    return CASPR_OK;
}

// the reverse sweep of the taped solve: latent_dp5_adjoint_kernel, caspr_latent_dopri5_adjoint_f32
#include "ode_latent_dp5_adjoint.inc"
