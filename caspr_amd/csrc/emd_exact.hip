// emd_exact.hip -- the EXACT earth mover's distance between two clouds of equal size: the cost of the optimal one-to-one assignment, by a
// forward Jacobi auction with epsilon scaling (Bertsekas), and the gradient of that cost with the matching held fixed.  The reference has
// only the approximation (utils/emd.py:11-12, evaluations.py:45-46: approxmatch + matchcost, restated in emd.hip); this is the yardstick
// the approximation is measured against, with semantics that are derivable rather than measured (include/caspr_hip.h states them,
// tests/emd_exact_ref.py restates them in numpy f64, and the two agree bit for bit in assign and prices).
//
// One workgroup of 1024 threads (16 waves) per frame, everything in LDS (72 n bytes, 144 KiB at n = 2048):
//   price f64[n] | best u64[n] | winkey u64[n] | bidv f64[n] | q x,y,z f32[n] | p x,y,z f32[n] | owner i32[n] | list0, list1 i32[n] | bidj i32[n]
// A round:
//   A  a wave serves one unassigned bidder at a time (wave w: list[w], list[w + 16], ...): lanes stride over the objects j, four at a time
//      with their LDS reads issued together, v = -c[i,j] - price[j] with c recomputed from the coordinates; (best value, lowest index,
//      second value) meet across the wave (DPP inside a 16-lane row, readlane across the four rows); lane 0 posts
//      bid = price[j1] + (v1 - v2) + eps as bidj / bidv and as a 64-bit LDS max of the bid's bit pattern on best[j1] (bids are positive
//      doubles: their bits order as unsigned integers).  A round with nb <= 8 bidders gives each of them W = 2, 4, 8 or 16 waves (the
//      largest power of two <= 16 / nb): the waves split the objects, their partial results meet through LDS behind one more barrier and
//      a thread per bidder posts.  Measured on an MI355X at n = 2048: with one wave per bidder and a rolled scan a round took 8.6 us on
//      uniform clouds (5 bids per round on average, most rounds with one or two), which is what this split is for.  price is only READ
//      here: every bid of a round is computed from the prices at the start of the round.
//   B  a thread per bidder: if its bid holds the maximum, a 64-bit LDS max of (round << 32 | 0x7fffffff - i) on winkey[j1]: the lowest
//      bidder index among the holders wins.  The round number in the key makes every earlier round's key smaller: nothing is reset.
//   C  a thread per bidder: the winner takes the object (owner, price = bid), the previous owner and every loser go to the next list.
// best[j] never needs a reset either: a bid is >= the price it was computed from, and after the round price[j] is the winning bid, so
// best[j] == bits(price[j]) before every round.  The integer maxima are order-independent and the order of the next list does not enter
// any value (bids come from start-of-round prices, ties from indices), so a frame's assign, prices, cost and counts are functions of the
// frame alone: not of the wave schedule, of B or of the frame's place in the batch.  No float atomics.
// Every loop is bounded: a round posts >= 1 bid, a frame stops when its bid count would pass max_bids, phases <= 64; three or four workgroup
// barriers per round under conditions every thread reads from LDS after a barrier (uniform), no spin, no cross-workgroup wait.
// Measured shape of the work (f64 prototype, n = 2048): 3-8 n rounds with 5-20 bidders each on ordinary clouds -- most waves idle in
// most rounds, which is the nature of the algorithm and why frames run side by side on the chip.
#include "common.h"

#include <limits.h>
#include <math.h>

#define EMDX_THREADS 1024
#define EMDX_WAVES (EMDX_THREADS / 64)
#define EMDX_MAX_N 2048
#define EMDX_MAX_PHASES 64
#define EMDX_LDS_PER_POINT 72

// (best value, its lowest index, second-best value) of two disjoint sets of candidates
__device__ __forceinline__ void emdx_merge(double &v1, int &j1, double &v2, double ov1, int oj1, double ov2)
{
    const bool take = ov1 > v1 || (ov1 == v1 && oj1 < j1);
    const double lost = take ? v1 : ov1, second = take ? ov2 : v2;
    v2 = lost > second ? lost : second;
    if (take) { v1 = ov1; j1 = oj1; }
}

template <int CTRL>
__device__ __forceinline__ void emdx_merge_dpp(double &v1, int &j1, double &v2)
{
    const double ov1 = dpp_mov<CTRL>(v1), ov2 = dpp_mov<CTRL>(v2);
    const int oj1 = dpp_mov_i32<CTRL>(j1);
    emdx_merge(v1, j1, v2, ov1, oj1, ov2);
}

__device__ __forceinline__ double emdx_readlane(double v, int lane)
{
    const long long b = __builtin_bit_cast(long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __builtin_bit_cast(double, (long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ float emdx_dist(float x1, float y1, float z1, float x2, float y2, float z2)
{
    const float dx = x1 - x2, dy = y1 - y2, dz = z1 - z2;
    return sqrtf(dx * dx + dy * dy + dz * dz);
}

// one lane's share of a bidder's scan: objects jstart, jstart + jstep, ... ascending (so a strict > keeps the lowest index), four at a time
// with their LDS reads issued together; an index past the end reads object n - 1 and is given the value -inf, which changes nothing
__device__ __forceinline__ void emdx_scan(float x, float y, float z, const float *qx, const float *qy, const float *qz, const double *price, int n,
                                          int jstart, int jstep, double &v1, int &j1, double &v2)
{
    for (int j0 = jstart; j0 < n; j0 += 4 * jstep) {
        float c[4];
        double pr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u * jstep, jj = j < n ? j : n - 1;
            c[u] = emdx_dist(x, y, z, qx[jj], qy[jj], qz[jj]);
            pr[u] = price[jj];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + u * jstep;
            double v = -(double)c[u] - pr[u];
            if (j >= n) v = -INFINITY;
            const bool g1 = v > v1, g2 = v > v2;
            v2 = g1 ? v1 : (g2 ? v : v2);
            v1 = g1 ? v : v1;
            j1 = g1 ? j : j1;
        }
    }
}

// the bid of the bidder at list position pos, from its best value v1 at object j1 and its second-best value v2
__device__ __forceinline__ void emdx_post(double v1, int j1, double v2, int n, double e, int pos, const double *price, unsigned long long *best,
                                          int *bidj, double *bidv, int *fail)
{
    if (j1 >= n) {
        *fail = 1;                                    // no object compares above -inf (NaN or infinite input): the frame stops, nothing is indexed
        return;
    }
    if (n == 1) v2 = v1;
    const double bid = price[j1] + (v1 - v2) + e;
    bidj[pos] = j1;
    bidv[pos] = bid;
    atomicMax(&best[j1], (unsigned long long)__builtin_bit_cast(long long, bid));
}

__global__ __launch_bounds__(EMDX_THREADS) void emd_exact_kernel(const float *__restrict__ xyz1, const float *__restrict__ xyz2, int n, double eps,
                                                                 long max_bids, float *__restrict__ cost, int *__restrict__ assign,
                                                                 double *__restrict__ prices, int *__restrict__ info)
{
    extern __shared__ double emdx_lds[];
    __shared__ int cnt[2];
    __shared__ int fail;
    __shared__ float red[6 * EMDX_WAVES];
    __shared__ double part_v1[EMDX_WAVES], part_v2[EMDX_WAVES];
    __shared__ int part_j1[EMDX_WAVES];
    double *price = emdx_lds;
    unsigned long long *best = (unsigned long long *)(price + n), *winkey = best + n;
    double *bidv = (double *)(winkey + n);
    float *qx = (float *)(bidv + n), *qy = qx + n, *qz = qy + n, *px = qz + n, *py = px + n, *pz = py + n;
    int *owner = (int *)(pz + n), *list0 = owner + n, *list1 = list0 + n, *bidj = list1 + n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long b = blockIdx.x;
    const float *p1 = xyz1 + b * n * 3, *p2 = xyz2 + b * n * 3;

    // both clouds into LDS, their bounding box on the way (min and max are exact: their order does not matter)
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int j = tid; j < n; j += EMDX_THREADS) {
        const float a[3] = {p1[j * 3], p1[j * 3 + 1], p1[j * 3 + 2]}, c[3] = {p2[j * 3], p2[j * 3 + 1], p2[j * 3 + 2]};
        px[j] = a[0]; py[j] = a[1]; pz[j] = a[2];
        qx[j] = c[0]; qy[j] = c[1]; qz[j] = c[2];
        price[j] = 0.0; best[j] = 0ull; winkey[j] = 0ull;
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], fminf(a[k], c[k])); hi[k] = fmaxf(hi[k], fmaxf(a[k], c[k])); }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
        for (int w = 32; w >= 1; w >>= 1) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], w)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], w)); }
    if (lane == 0)
        for (int k = 0; k < 3; ++k) { red[k * EMDX_WAVES + wave] = lo[k]; red[(3 + k) * EMDX_WAVES + wave] = hi[k]; }
    if (tid == 0) fail = 0;
    __syncthreads();
    float ext[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float l = red[k * EMDX_WAVES], h = red[(3 + k) * EMDX_WAVES];
        for (int w = 1; w < EMDX_WAVES; ++w) { l = fminf(l, red[k * EMDX_WAVES + w]); h = fmaxf(h, red[(3 + k) * EMDX_WAVES + w]); }
        ext[k] = h - l;
    }
    const float diag = sqrtf(ext[0] * ext[0] + ext[1] * ext[1] + ext[2] * ext[2]);
    double e = (double)diag / 4.0;
    if (!(e > eps)) e = eps;

    long bids = 0;
    int rounds = 0, phases = 0;
    bool converged = false;
    while (phases < EMDX_MAX_PHASES) {
        ++phases;
        __syncthreads();     // a thread that has yet to read the count that ended the last phase (cnt[0] when its rounds were even) reads it first
        for (int j = tid; j < n; j += EMDX_THREADS) { owner[j] = -1; list0[j] = j; }
        if (tid == 0) cnt[0] = n;
        __syncthreads();
        int cur = 0;
        bool stopped = false;
        for (;;) {
            const int nb = cnt[cur];
            if (nb == 0) break;
            if (bids + nb > max_bids) { stopped = true; break; }
            bids += nb;
            ++rounds;
            const int *list = cur ? list1 : list0;
            int *next = cur ? list0 : list1;
            if (tid == 0) cnt[cur ^ 1] = 0;
            // A: the bids, from the prices at the start of the round.  W waves share a bidder when the round has few of them (W = the largest
            // power of two <= 16 / nb): each scans every W-th group of 64 objects and the W partial results meet through LDS behind one more
            // barrier.  The merge is a maximum with index tie-breaks, so the split changes no bit.
            int W = 1;
            while (W * 2 * nb <= EMDX_WAVES) W *= 2;
            for (int pos0 = 0; pos0 < nb; pos0 += EMDX_WAVES / W) {          // one pass when W > 1
                const int pos = pos0 + wave / W, part = wave % W;
                if (pos >= nb) continue;
                const int i = list[pos];
                double w1 = -INFINITY, w2 = -INFINITY;
                int k1 = INT_MAX;
                emdx_scan(px[i], py[i], pz[i], qx, qy, qz, price, n, part * 64 + lane, 64 * W, w1, k1, w2);
                emdx_merge_dpp<0xB1>(w1, k1, w2);     // xor 1, xor 2, the other quad, the other half of the row: disjoint sets at every step
                emdx_merge_dpp<0x4E>(w1, k1, w2);
                emdx_merge_dpp<0x141>(w1, k1, w2);
                emdx_merge_dpp<0x140>(w1, k1, w2);
                double v1 = emdx_readlane(w1, 0), v2 = emdx_readlane(w2, 0);
                int j1 = __builtin_amdgcn_readlane(k1, 0);
#pragma unroll
                for (int row = 1; row < 4; ++row)
                    emdx_merge(v1, j1, v2, emdx_readlane(w1, row * 16), __builtin_amdgcn_readlane(k1, row * 16), emdx_readlane(w2, row * 16));
                if (lane == 0) {
                    if (W == 1) emdx_post(v1, j1, v2, n, e, pos, price, best, bidj, bidv, &fail);
                    else { part_v1[wave] = v1; part_v2[wave] = v2; part_j1[wave] = j1; }
                }
            }
            if (W > 1) {
                __syncthreads();
                if (tid < nb) {
                    double v1 = part_v1[tid * W], v2 = part_v2[tid * W];
                    int j1 = part_j1[tid * W];
                    for (int k = 1; k < W; ++k) emdx_merge(v1, j1, v2, part_v1[tid * W + k], part_j1[tid * W + k], part_v2[tid * W + k]);
                    emdx_post(v1, j1, v2, n, e, tid, price, best, bidj, bidv, &fail);
                }
            }
            __syncthreads();
            if (fail) { stopped = true; break; }
            // B: among the bidders that hold an object's maximum, the lowest index
            for (int pos = tid; pos < nb; pos += EMDX_THREADS) {
                const int j = bidj[pos];
                if ((unsigned long long)__builtin_bit_cast(long long, bidv[pos]) == best[j])
                    atomicMax(&winkey[j], ((unsigned long long)(unsigned)rounds << 32) | (unsigned)(INT_MAX - list[pos]));
            }
            __syncthreads();
            // C: the winner takes the object; its previous owner and the losers bid again
            for (int pos = tid; pos < nb; pos += EMDX_THREADS) {
                const int i = list[pos], j = bidj[pos];
                if (winkey[j] == (((unsigned long long)(unsigned)rounds << 32) | (unsigned)(INT_MAX - i))) {
                    const int prev = owner[j];
                    owner[j] = i;
                    price[j] = bidv[pos];
                    if (prev >= 0) next[atomicAdd(&cnt[cur ^ 1], 1)] = prev;
                } else {
                    next[atomicAdd(&cnt[cur ^ 1], 1)] = i;
                }
            }
            __syncthreads();
            cur ^= 1;
        }
        if (stopped) break;
        if (e <= eps) { converged = true; break; }
        e = e / 5.0;
        if (!(e > eps)) e = eps;
    }

    // every thread holds the same converged / counts; owner and price are complete behind the last barrier
    float my = 0.f;
    for (int j = tid; j < n; j += EMDX_THREADS) {
        prices[b * n + j] = price[j];
        if (converged) {
            const int i = owner[j];
            assign[b * n + i] = j;
            my += emdx_dist(px[i], py[i], pz[i], qx[j], qy[j], qz[j]);
        } else {
            assign[b * n + j] = -1;
        }
    }
    for (int w = 32; w >= 1; w >>= 1) my += __shfl_xor(my, w);     // a fixed tree: the same bits on every run
    __syncthreads();                                              // red was read by everyone long ago; the barrier orders its reuse
    if (lane == 0) red[wave] = my;
    __syncthreads();
    if (tid == 0) {
        float s = red[0];
        for (int w = 1; w < EMDX_WAVES; ++w) s += red[w];
        cost[b] = converged ? s : NAN;
        info[b * 4 + 0] = converged ? 1 : 0;
        info[b * 4 + 1] = phases;
        info[b * 4 + 2] = rounds;
        info[b * 4 + 3] = (int)bids;
    }
}

extern "C" long caspr_emd_exact_ws_bytes(int B, int n) { (void)B; (void)n; return 0; }

extern "C" int caspr_emd_exact_f32(const float *xyz1, const float *xyz2, int B, int n, double eps, long max_bids, float *cost, int32_t *assign,
                                   double *prices, int32_t *info, void *ws, long ws_bytes, void *stream)
{
    (void)ws;
    CASPR_REQUIRE(xyz1 && xyz2 && cost && assign && prices && info && B > 0 && n > 0, "emd_exact: bad arguments");
    CASPR_REQUIRE(n <= EMDX_MAX_N, "emd_exact: n=%d: a frame lives in the LDS of one workgroup, n <= %d", n, EMDX_MAX_N);
    CASPR_REQUIRE(B <= 65535, "emd_exact: B=%d: B <= 65535", B);
    CASPR_REQUIRE(eps > 0.0 && eps < (double)INFINITY, "emd_exact: eps=%g must be positive and finite", eps);
    CASPR_REQUIRE(max_bids >= 1 && max_bids <= 2147483647L, "emd_exact: max_bids=%ld must lie in 1 .. 2^31 - 1", max_bids);
    CASPR_REQUIRE(ws_bytes >= caspr_emd_exact_ws_bytes(B, n), "emd_exact: workspace too small");
    static CasprLdsOptIn optin;
    const hipError_t err = caspr_lds_opt_in(optin, (const void *)emd_exact_kernel, (size_t)EMDX_LDS_PER_POINT * EMDX_MAX_N);
    if (err != hipSuccess) {
        caspr_set_error("emd_exact: hipFuncSetAttribute failed: %s", hipGetErrorString(err));
        return CASPR_ELAUNCH;
    }
    emd_exact_kernel<<<dim3(B), dim3(EMDX_THREADS), (size_t)EMDX_LDS_PER_POINT * n, (hipStream_t)stream>>>(xyz1, xyz2, n, eps, max_bids, cost, assign,
                                                                                                          prices, info);
    CASPR_CHECK_LAUNCH("emd_exact");
    return CASPR_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The gradient of the cost with the matching held fixed (the true gradient wherever the optimum is unique):
//   d cost / d x_i = g (x_i - y_assign[i]) / |x_i - y_assign[i]|,   d cost / d y_j = -(the term of the one i with assign[i] = j)
// One workgroup per frame builds the inverse permutation in LDS; then a thread owns one output point: no atomics, bit-reproducible.
// The term is formed in f64 from the f32 coordinates and rounded once.  A coincident pair contributes exactly 0 (caspr_emd_bwd_f32's
// convention); a frame whose assign holds an index outside 0 .. n-1 (the -1 of a frame that did not converge) gets NaN in every
// component, and so does an object no point is assigned to.
__device__ __forceinline__ void emdx_term(const float *__restrict__ p, const float *__restrict__ q, double g, double t[3])
{
    const double dx = (double)p[0] - (double)q[0], dy = (double)p[1] - (double)q[1], dz = (double)p[2] - (double)q[2];
    const double c = sqrt(dx * dx + dy * dy + dz * dz);
    t[0] = c > 0.0 ? g * dx / c : 0.0;
    t[1] = c > 0.0 ? g * dy / c : 0.0;
    t[2] = c > 0.0 ? g * dz / c : 0.0;
}

__global__ __launch_bounds__(256) void emd_exact_bwd_kernel(const float *__restrict__ xyz1, const float *__restrict__ xyz2,
                                                            const int *__restrict__ assign, const float *__restrict__ gcost, int n,
                                                            float *__restrict__ gxyz1, float *__restrict__ gxyz2)
{
    __shared__ int inv[EMDX_MAX_N];
    __shared__ int bad;
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    const float *p = xyz1 + b * n * 3, *q = xyz2 + b * n * 3;
    const int *a = assign + b * n;
    if (tid == 0) bad = 0;
    for (int j = tid; j < n; j += 256) inv[j] = -1;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int j = a[i];
        if ((unsigned)j >= (unsigned)n) bad = 1;
        else inv[j] = i;
    }
    __syncthreads();
    const bool frame_bad = bad != 0;
    const double g = (double)gcost[b];
    double t[3];
    if (gxyz1) {
        float *d = gxyz1 + b * n * 3;
        for (int i = tid; i < n; i += 256) {
            if (frame_bad) { t[0] = t[1] = t[2] = (double)NAN; }
            else emdx_term(p + i * 3, q + a[i] * 3, g, t);
            d[i * 3] = (float)t[0]; d[i * 3 + 1] = (float)t[1]; d[i * 3 + 2] = (float)t[2];
        }
    }
    if (gxyz2) {
        float *d = gxyz2 + b * n * 3;
        for (int j = tid; j < n; j += 256) {
            const int i = inv[j];
            if (frame_bad || i < 0) { t[0] = t[1] = t[2] = (double)NAN; }
            else emdx_term(p + i * 3, q + j * 3, g, t);
            d[j * 3] = (float)-t[0]; d[j * 3 + 1] = (float)-t[1]; d[j * 3 + 2] = (float)-t[2];
        }
    }
}

extern "C" int caspr_emd_exact_bwd_f32(const float *xyz1, const float *xyz2, const int32_t *assign, const float *gcost, int B, int n,
                                       float *gxyz1, float *gxyz2, void *stream)
{
    CASPR_REQUIRE(xyz1 && xyz2 && assign && gcost && B > 0 && n > 0, "emd_exact_bwd: bad arguments");
    CASPR_REQUIRE(n <= EMDX_MAX_N, "emd_exact_bwd: n=%d: the inverse permutation lives in LDS, n <= %d", n, EMDX_MAX_N);
    CASPR_REQUIRE(B <= 65535, "emd_exact_bwd: B=%d: B <= 65535", B);
    CASPR_REQUIRE(gxyz1 || gxyz2, "emd_exact_bwd: gxyz1 and gxyz2 are both NULL: nothing to compute");
    emd_exact_bwd_kernel<<<dim3(B), dim3(256), 0, (hipStream_t)stream>>>(xyz1, xyz2, assign, gcost, n, gxyz1, gxyz2);
    CASPR_CHECK_LAUNCH("emd_exact_bwd");
    return CASPR_OK;
}
