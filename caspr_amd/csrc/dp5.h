// dp5.h -- what the two adaptive point-CNF solves, cnf_dp5_kernel<DIV> (ode_dp5.hip) and cnf_dp5_h3w_kernel (ode_dp5_f16x3w.hip),
// share besides the pure rules (dp5_rules.h) and the tableau (dp5_tables.inc): the ONE text of their launch protocol.
//  * device: the frame's controller state and its load at the head of a launch, the slot-order sum of a frame's partial sums, the
//    publication of the frame's state and counters, the workgroup's reduction into its slot;
//  * host: the workspace layout, the argument checks and the launch loop of caspr_cnf_dopri5_f32 and caspr_cnf_dopri5_h3_f32.
// The protocol itself is described in ode_dp5.hip's header.  The norms (two tensors there, one here), the range guard of the f16x3
// route and the evaluations are the kernels' own.
#pragma once
#include "common.h"
#include "dp5_rules.h"

#define DP5_TRACE_HEAD 8     // floats per frame before the attempt rows: d0, d1, d2, h0, first dt, 0, 0, 0
#define DP5_TRACE_ROW 5      // per attempt: t, dt, ratio of x, ratio of logp (0 on the f16x3 route), accepted (1 / 0)
// carry-over quantities of a point, each [components][n]
#define DP5_Y 0
#define DP5_F0 1
#define DP5_YN 2
#define DP5_K7 3
#define DP5_YM 4

struct Dp5Frame {            // a frame's controller state, written by its first workgroup, double-buffered by launch parity
    double t;                // solver time (negated when the solve runs in reverse, as upstream)
    float dt, h0, d0, d1, d2, dt0;
    int done, nacc, nrej, nfe;
    int pad[2];
};

// The four device pieces below are statement macros over the kernels' own variables, not functions: as __forceinline__ functions
// every one of them changed the register allocation of a kernel (tools/code_object_diff.py), as text they compile to the same code.
// Each is one statement and takes its semicolon, except DP5_SLOT_SUM, which declares S in the caller's scope.

// the frame's state st at the head of launch Lc: the previous launch's, or the initial one.  A retired frame's state is carried
// over and the workgroup RETURNS FROM THE KERNEL
#define DP5_FRAME_LOAD_OR_RETURN(st, fprev, fnext, Lc, lead, reverse, t_end)    \
    do {                                                                         \
        if (Lc > 0) {                                                            \
            st = *(fprev);                                                       \
            if (st.done) {                                                       \
                if (lead) *(fnext) = st;                                         \
                return;                                                          \
            }                                                                    \
        } else {                                                                 \
            st.t = (reverse) ? -(double)(t_end) : 0.0;                           \
            st.dt = st.h0 = st.d0 = st.d1 = st.d2 = st.dt0 = 0.f;                \
            st.done = st.nacc = st.nrej = st.nfe = 0;                            \
            st.pad[0] = st.pad[1] = 0;                                           \
        }                                                                        \
    } while (0)

// double S[4]: the frame's sums of the previous launch, its workgroups' slots added in slot order -- the same in every workgroup of
// the frame.  A declaration and a statement: not for the body of an unbraced if
#define DP5_SLOT_SUM(S, part, Lc, BT, bt, nwg)                                             \
    double S[4] = {0.0, 0.0, 0.0, 0.0};                                                    \
    if (Lc > 0) {                                                                          \
        const double *p = (part) + ((long)(((Lc) & 1) ^ 1) * (BT) + (bt)) * (nwg) * 4;     \
        for (int w = 0; w < (nwg); ++w)                                                    \
            _Pragma("unroll") for (int q = 0; q < 4; ++q) S[q] += p[4 * w + q];            \
    }

// the frame's lead thread publishes the state after this launch and the counters (finished: counters[3]); bump (true / false): the
// frame is still running, counted in this launch's word
#define DP5_PUBLISH(fnext, st, counters, bt, finished, bump, running)                      \
    do {                                                                                   \
        *(fnext) = st;                                                                     \
        int *c = (counters) + 4 * (bt);                                                    \
        c[0] = st.nacc; c[1] = st.nrej; c[2] = st.nfe; c[3] = finished;                    \
        if (bump) atomicAdd(running, 1);                                                   \
    } while (0)

// the workgroup's NQ partial sums v (f64, one set per lane) -> its slot: a butterfly over the wave, the four waves' sums through
// s_red ([4 waves][4] doubles of LDS) added in wave order by thread 0; the slot's remaining entries are zeroed.  Holds a
// __syncthreads(): every thread of the workgroup passes it
#define DP5_BLOCK_REDUCE(v, NQ, s_red, slot_, tid, lane0, wave)                                                            \
    do {                                                                                                                   \
        _Pragma("unroll") for (int q = 0; q < NQ; ++q) {                                                                   \
            _Pragma("unroll") for (int o_ = 32; o_ > 0; o_ >>= 1) v[q] += __shfl_xor(v[q], o_);                            \
        }                                                                                                                  \
        if (lane0 == 0) {                                                                                                  \
            _Pragma("unroll") for (int q = 0; q < NQ; ++q) s_red[4 * wave + q] = v[q];                                     \
        }                                                                                                                  \
        __syncthreads();                                                                                                   \
        if (tid == 0) {                                                                                                    \
            double *slot = slot_;                                                                                          \
            _Pragma("unroll") for (int q = 0; q < NQ; ++q) slot[q] = ((s_red[q] + s_red[4 + q]) + s_red[8 + q]) + s_red[12 + q];   \
            _Pragma("unroll") for (int q = NQ; q < 4; ++q) slot[q] = 0.0;                                                  \
        }                                                                                                                  \
    } while (0)

// ---- host: the workspace [frames 2 x BT | slots 2 x BT x workgroups of a frame x 4 f64 | running, one word per launch | carry-over
// of the points], each part 256-byte aligned.  wg_pts: points of a workgroup, pt_floats: carry-over floats of a point
static inline long dp5_align(long b) { return (b + 255) & ~255L; }
struct Dp5Layout { long frames, part, running, pts, total; };
static Dp5Layout dp5_layout(int BT, int n, int max_attempts, int wg_pts, int pt_floats)
{
    Dp5Layout l;
    const long nwg = ceil_div(n, wg_pts);
    l.frames = 0;
    l.part = dp5_align(2L * BT * (long)sizeof(Dp5Frame));
    l.running = l.part + dp5_align(2L * BT * nwg * 4 * (long)sizeof(double));
    l.pts = l.running + dp5_align(((long)max_attempts + 3) * (long)sizeof(int));
    l.total = l.pts + dp5_align((long)BT * pt_floats * n * (long)sizeof(float));
    return l;
}
static long dp5_ws_bytes(int BT, int n, int max_attempts, int wg_pts, int pt_floats)
{
    if (BT <= 0 || n <= 0 || max_attempts <= 0) return 0;
    return dp5_layout(BT, n, max_attempts, wg_pts, pt_floats).total;
}

// the argument checks of an entry, in their order; name: the route's, for the messages.  ptrs / pair: the entry's own two conditions
// (no null pointer; e and logp_out given together)
static int dp5_check(const char *name, bool ptrs, bool pair, int H, int H_built, int BT, int n, int max_attempts, int ldh, float rtol, float atol,
                     float t_end, const void *w0, const void *w1, const void *w2, const void *w3, const void *ws, long ws_bytes, long ws_need)
{
    CASPR_REQUIRE(ptrs, "%s: null pointer", name);
    CASPR_REQUIRE(H == H_built, "%s: hidden width %d unsupported (kernel is built for 512-512-512, flow.py:89)", name, H);
    CASPR_REQUIRE(BT > 0 && BT <= 65535 && n > 0 && max_attempts > 0 && ldh >= 2 * (3 * H + 3), "%s: bad sizes", name);
    CASPR_REQUIRE(rtol > 0.f && atol > 0.f && t_end > 0.f && rtol < INFINITY && atol < INFINITY && t_end < INFINITY, "%s: rtol, atol and t_end must be positive and finite", name);
    CASPR_REQUIRE(pair, "%s: e and logp_out must be given together", name);
    CASPR_REQUIRE(((uintptr_t)w1 % 16) == 0 && ((uintptr_t)w2 % 16) == 0 && ((uintptr_t)w0 % 16) == 0 && ((uintptr_t)w3 % 16) == 0,
                  "%s: weights must be 16-byte aligned", name);
    CASPR_REQUIRE(ws_bytes >= ws_need && ((uintptr_t)ws % 256) == 0, "%s: workspace of %ld bytes, 256-byte aligned, needed", name, ws_need);
    return CASPR_OK;
}

// the host loop: launch(L, last) until the device word "frames still running" of launch L reads zero; CASPR_ENOCONV after max_attempts
// attempts -- never an unbounded loop.  d_running: the layout's words; status: the route's status word, zeroed with them, or NULL
template <typename Launch>
static int dp5_run(const char *name, CasprLdsOptIn &optin, const void *kernel, size_t lds, int BT, int max_attempts, float rtol, float atol,
                   int *d_running, float *trace, unsigned *status, hipStream_t st, Launch launch)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        caspr_set_error("%s: the host loop reads the device after every attempt and cannot run under stream capture", name);
        return CASPR_EUNSUP;
    }
    const hipError_t err = caspr_lds_opt_in(optin, kernel, lds);
    if (err != hipSuccess) {
        caspr_set_error("%s: hipFuncSetAttribute failed: %s", name, hipGetErrorString(err));
        return CASPR_ELAUNCH;
    }
    int *h_running = nullptr;
    if (hipHostMalloc((void **)&h_running, sizeof(int), hipHostMallocDefault) != hipSuccess) {
        caspr_set_error("%s: hipHostMalloc failed", name);
        return CASPR_ELAUNCH;
    }
    hipError_t he = hipMemsetAsync(d_running, 0, ((long)max_attempts + 3) * sizeof(int), st);
    if (he == hipSuccess) he = hipMemsetAsync(trace, 0, (long)BT * (DP5_TRACE_HEAD + DP5_TRACE_ROW * (long)max_attempts) * sizeof(float), st);
    if (he == hipSuccess && status) he = hipMemsetAsync(status, 0, sizeof(unsigned), st);
    int running = 1;
    // launch L = 0, 1: initial-step selection; L >= 2: decide attempt L - 3, run attempt L - 2; L = max_attempts + 2 decides only
    for (int L = 0; he == hipSuccess && L <= max_attempts + 2; ++L) {
        launch(L, L == max_attempts + 2);
        he = hipGetLastError();
        if (he != hipSuccess || L < 3) continue;       // no frame's attempt is decided before launch 3: none retires
        // one small pinned read per attempt: the frames that launch L left running
        he = hipMemcpyAsync(h_running, d_running + L, sizeof(int), hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        if (he != hipSuccess) break;
        running = *h_running;
        if (running == 0) break;
    }
    (void)hipHostFree(h_running);
    if (he != hipSuccess) {
        caspr_set_error("%s: %s", name, hipGetErrorString(he));
        return CASPR_ELAUNCH;
    }
    if (running != 0) {
        caspr_set_error("%s: %d of %d frames did not reach t_end within max_attempts = %d (rtol %g, atol %g)", name, running, BT, max_attempts,
                        (double)rtol, (double)atol);
        return CASPR_ENOCONV;
    }
    return CASPR_OK;
}
