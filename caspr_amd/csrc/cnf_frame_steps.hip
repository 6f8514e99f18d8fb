// cnf_frame_steps.hip -- the controller of the per-frame RK4 step counts of the point-CNF sampling solve (cnf.py:70-128 with
// logpx = None; flow.py:96-99: the reference controls its error at every call, a fixed step count does not).
//
// The pilot (ops.cnf_frame_steps) solves the first g points of every frame on the ladder of step counts 1, 2, 4, .., S_max with the
// narrow sampling kernel and a step table that holds the rung for the frames still undecided and 0 (skip) for the others.  After
// rung P >= 2 the UPDATE kernel below looks at every undecided frame: its Richardson estimate e = max |x_P - x_{P/2}| / 15 of the
// P-step error against bound = tol (1 + max |x_P|) -- the accuracy guard's criterion (models/caspr.py), frame by frame.  A frame
// that passes takes the smallest count the fourth-order law predicts to pass with a safety factor, never below P/2 + 1 (P/2 was not
// shown to pass) and never above P (which was); a frame that fails goes on to rung 2 P, or is capped at S_max.  The ORDER kernel
// sorts the frames by descending count (longest first) for the main launch.
//
// Nothing here is read by the host: all launches are enqueued unconditionally, the path is capturable.  Every decision is a function
// of the frame's own pilot points alone.  The maxima are order-independent (no atomics); everything after them is f64 with two
// correctly rounded square roots, no contraction (build.py: -ffp-contract=off), so tests/frame_steps_ref.py reproduces each decision
// and each statistic bit for bit.  Table and order are written with ordinary vector stores.
#include "common.h"

// one wave per frame
__global__ __launch_bounds__(64) void cnf_steps_update_kernel(const float *__restrict__ x_prev, const float *__restrict__ x_cur, int BT, int g,
                                                              int P, double tol, double safety, int S_max, int *__restrict__ steps,
                                                              int *__restrict__ next_tab, int *__restrict__ capped, double *__restrict__ stats)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= BT) return;
    if (steps[f] != 0) {        // decided at an earlier rung: skipped from now on, statistics kept
        if (lane == 0) next_tab[f] = 0;
        return;
    }
    const float *xp = x_prev + (long)f * g * 3, *xc = x_cur + (long)f * g * 3;
    float d = 0.0f, xm = 0.0f;
    int bad = 0;
    for (int i = lane; i < 3 * g; i += 64) {
        const float c = xc[i], df = c - xp[i];
        bad |= !(fabsf(c) < INFINITY) || !(fabsf(df) < INFINITY);     // NaN or infinity in either solution
        d = fmaxf(d, fabsf(df));
        xm = fmaxf(xm, fabsf(c));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        d = fmaxf(d, __shfl_xor(d, o));
        xm = fmaxf(xm, __shfl_xor(xm, o));
        bad |= __shfl_xor(bad, o);
    }
    if (lane != 0) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double dd = nan, bound = nan, pred = nan;
    bool pass = false;
    if (!bad) {
        dd = (double)d;
        bound = tol * (1.0 + (double)xm);
        const double e = dd / 15.0;
        pred = ((double)P * sqrt(sqrt(e / bound))) * safety;
        pass = e <= bound;
    }
    int S = 0, cap = 0;
    if (pass) {
        // (pred is NaN only for tol = 0 with e = 0: the largest count of the bracket then)
        S = (P == 2) ? 2 : (pred >= (double)P || !(pred == pred)) ? P : max((int)ceil(pred), P / 2 + 1);
    } else if (P >= S_max) {
        S = S_max;
        cap = 1;
    }
    steps[f] = S;
    next_tab[f] = S ? 0 : 2 * P;
    capped[f] = cap;
    stats[4 * f] = dd;
    stats[4 * f + 1] = bound;
    stats[4 * f + 2] = pred;
    stats[4 * f + 3] = S ? (double)P : 0.0;
}

// order[rank(f)] = f, rank(f) = #{j : S_j > S_f} + #{j < f : S_j == S_f}: the stable descending sort, by counting (BT^2 comparisons,
// one launch, nothing shared between workgroups; BT <= 65535).  Every rank is hit exactly once, so every row of `order` is written.
__global__ __launch_bounds__(256) void cnf_steps_order_kernel(const int *__restrict__ steps, int BT, int *__restrict__ order)
{
    __shared__ int tile[256];
    const int f = blockIdx.x * 256 + threadIdx.x;
    const int Sf = f < BT ? steps[f] : 0;
    int rank = 0;
    for (int j0 = 0; j0 < BT; j0 += 256) {
        __syncthreads();
        tile[threadIdx.x] = (j0 + threadIdx.x < BT) ? steps[j0 + threadIdx.x] : 0;
        __syncthreads();
        const int m = min(256, BT - j0);
        for (int k = 0; k < m; ++k) {
            const int Sj = tile[k];
            rank += (Sj > Sf) || (Sj == Sf && j0 + k < f);
        }
    }
    if (f < BT) order[rank] = f;
}

extern "C" int caspr_cnf_steps_update_f32(const float *x_prev, const float *x_cur, int BT, int g, int P, double tol, double safety, int S_max,
                                          int *steps, int *next_tab, int *capped, double *stats, void *stream)
{
    CASPR_REQUIRE(x_prev && x_cur && steps && next_tab && capped && stats, "cnf_steps_update: null pointer");
    CASPR_REQUIRE(BT > 0 && BT <= 65535 && g > 0 && g <= (1 << 24), "cnf_steps_update: bad sizes");
    CASPR_REQUIRE(S_max >= 2 && S_max <= 256 && (S_max & (S_max - 1)) == 0, "cnf_steps_update: S_max %d is not a power of two in 2..256", S_max);
    CASPR_REQUIRE(P >= 2 && P <= S_max && (P & (P - 1)) == 0, "cnf_steps_update: rung %d is not a power of two in 2..S_max", P);
    CASPR_REQUIRE(tol >= 0.0 && tol < INFINITY && safety >= 1.0 && safety < INFINITY, "cnf_steps_update: tol must be finite and >= 0, safety finite and >= 1");
    cnf_steps_update_kernel<<<BT, 64, 0, (hipStream_t)stream>>>(x_prev, x_cur, BT, g, P, tol, safety, S_max, steps, next_tab, capped, stats);
    CASPR_CHECK_LAUNCH("cnf_steps_update");
    return CASPR_OK;
}

extern "C" int caspr_cnf_steps_order(const int *steps, int BT, int *order, void *stream)
{
    CASPR_REQUIRE(steps && order, "cnf_steps_order: null pointer");
    CASPR_REQUIRE(BT > 0 && BT <= 65535, "cnf_steps_order: BT %d outside 1..65535", BT);
    cnf_steps_order_kernel<<<ceil_div(BT, 256), 256, 0, (hipStream_t)stream>>>(steps, BT, order);
    CASPR_CHECK_LAUNCH("cnf_steps_order");
    return CASPR_OK;
}
