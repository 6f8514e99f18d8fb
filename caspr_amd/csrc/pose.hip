// pose.hip -- rigid registration of index-corresponding point clouds by RANSAC (utils/evaluations.py:297-437,
// test_observed_camera_pose_ransac: Open3D registration_ransac_based_on_correspondence with ransac_n = 4, threshold 0.015,
// RANSACConvergenceCriteria(50000, 5000), TransformationEstimationPointToPoint(False); call site evaluations.py:370-375).
//
// For F frames of N correspondences src_i <-> dst_i (f32 rows of row_stride 3 or 4; only x, y, z are read), K hypotheses of
// n indices each (3 <= n <= 8), all arithmetic in f64 (an f32 input widens exactly):
//
//   Sampling   hypothesis h of frame f draws, with replacement (as Open3D's std::rand() % N), the indices
//                idx_j = mix(key ^ j) % N,  j = 0 .. n-1,  key = mix(mix(mix(mix(lo ^ 0x9e3779b9) ^ hi) ^ f) ^ h)
//              with lo / hi the low / high 32 bits of the 64-bit seed and, in uint32 arithmetic (every product mod 2^32),
//                mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
//              The reference seeds Open3D from the clock; here the seed is an argument and one seed gives bitwise-equal outputs.
//   Estimate   Horn's closed form without scale: centroids ca, cb of the n pairs (summed j = 0 .. n-1, divided by n), the
//              cross-covariance S = sum_j (a_j - ca)(b_j - cb)^T, its 4x4 symmetric matrix, the eigenvector of the largest
//              eigenvalue by POSE_SWEEPS cyclic Jacobi sweeps (no data-dependent branch; a rotation whose off-diagonal entry is
//              0 is the identity), the unit quaternion -> R (det R = +1 without a reflection fix), t = cb - R ca.  A degenerate
//              sample (repeated or collinear indices, identical points) gives a finite R, t: S = 0 gives R = I.
//   Score      i is an inlier when d2 = |R src_i + t - dst_i|^2 < threshold^2; fitness = inliers / N,
//              inlier_rmse = sqrt(sum_inliers d2 / inliers) (0 without inliers); d2 summed in index order.
//   Select     per frame the best hypothesis: most inliers, then lowest rmse, then lowest h (Open3D's order plus an index
//              tie-break); a total order, so the reduction's shape cannot change the winner.  No float atomics anywhere.
//   Refine     (refine = 1, optional) refit R, t on the winner's inlier set (at least 3 inliers) -- centroids, then the
//              cross-covariance, each a fixed-order workgroup reduction in f64 -- and score the refit: inliers / rmse then
//              describe the returned transform.  refine = 0 returns the winning hypothesis's transform and score.
//
// PARITY IS UNPINNED: our reading of the Open3D release the reference calls (the o3d.registration namespace, <= 0.9) is a loop
// of min(max_iteration, max_validation) = 5000 hypotheses without a final refit, which refine = 0 restates; that release's
// source was not available to check against, and its sampler (std::rand) is not reproducible across C libraries anyway.
//
// Two kernels: pose_score_kernel (one lane per hypothesis, 256 per workgroup; the frame's clouds staged through LDS in tiles
// of POSE_TILE points, read back as broadcasts) writes (inliers, rmse) per hypothesis to the workspace; pose_select_kernel (one
// workgroup per frame) picks the winner, re-derives its transform from the hash, optionally refines, and writes T.
// Built with -ffp-contract=off (build.py): every f64 expression below rounds as written, left to right, which is what the
// numpy restatement in tests/test_pose_ransac.py evaluates.
#include "common.h"

#define POSE_BLOCK 256
#define POSE_TILE 1024
#define POSE_SWEEPS 8
#define POSE_MAX_N 8

struct PoseArgs {
    const float *src, *dst;
    int N, rs, K, n;
    double thr2;
    unsigned long long seed;
};

struct PoseRT {
    double r[9], t[3];
};

__host__ __device__ __forceinline__ uint32_t pose_mix(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ uint32_t pose_key(unsigned long long seed, int f, int h)
{
    uint32_t x = pose_mix((uint32_t)seed ^ 0x9e3779b9u);
    x = pose_mix(x ^ (uint32_t)(seed >> 32));
    x = pose_mix(x ^ (uint32_t)f);
    return pose_mix(x ^ (uint32_t)h);
}

// Horn: S (row-major, S[3*i+k] = sum a_i b_k of the centred pairs), centroids ca (source) / cb (target) -> R, t with b ~ R a + t
__device__ __forceinline__ void pose_horn(const double S[9], const double ca[3], const double cb[3], PoseRT &o)
{
    const double sxx = S[0], sxy = S[1], sxz = S[2], syx = S[3], syy = S[4], syz = S[5], szx = S[6], szy = S[7], szz = S[8];
    double A[4][4], V[4][4];
    A[0][0] = (sxx + syy) + szz; A[0][1] = syz - szy;         A[0][2] = szx - sxz;         A[0][3] = sxy - syx;
    A[1][1] = (sxx - syy) - szz; A[1][2] = sxy + syx;         A[1][3] = szx + sxz;
    A[2][2] = (syy - sxx) - szz; A[2][3] = syz + szy;
    A[3][3] = (szz - sxx) - syy;
    A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[3][0] = A[0][3]; A[2][1] = A[1][2]; A[3][1] = A[1][3]; A[3][2] = A[2][3];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll
    for (int sw = 0; sw < POSE_SWEEPS; ++sw) {
#pragma unroll
        for (int pq = 0; pq < 6; ++pq) {
            const int p = pq < 3 ? 0 : (pq < 5 ? 1 : 2), q = pq < 3 ? pq + 1 : (pq < 5 ? pq - 1 : 3);
            const double apq = A[p][q];
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
            t = theta < 0.0 ? -t : t;
            t = apq != 0.0 ? t : 0.0;           // also masks the NaN of 0 / 0; theta -> inf gives t = 0
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double akp = A[k][p], akq = A[k][q];
                A[k][p] = c * akp - s * akq;
                A[k][q] = s * akp + c * akq;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double apk = A[p][k], aqk = A[q][k];
                A[p][k] = c * apk - s * aqk;
                A[q][k] = s * apk + c * aqk;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double vkp = V[k][p], vkq = V[k][q];
                V[k][p] = c * vkp - s * vkq;
                V[k][q] = s * vkp + c * vkq;
            }
        }
    }
    // the column of the largest diagonal entry (first on ties), normalised
    double best = A[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const bool b = A[k][k] > best;
        best = b ? A[k][k] : best;
        w = b ? V[0][k] : w; x = b ? V[1][k] : x; y = b ? V[2][k] : y; z = b ? V[3][k] : z;
    }
    const double nrm = sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / nrm; x = x / nrm; y = y / nrm; z = z / nrm;
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    double *R = o.r;
    R[0] = ((ww + xx) - yy) - zz;  R[1] = 2.0 * (x * y - w * z);    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);  R[4] = ((ww - xx) + yy) - zz;    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);  R[7] = 2.0 * (y * z + w * x);    R[8] = ((ww - xx) - yy) + zz;
#pragma unroll
    for (int i = 0; i < 3; ++i) o.t[i] = cb[i] - ((R[3 * i] * ca[0] + R[3 * i + 1] * ca[1]) + R[3 * i + 2] * ca[2]);
}

// the transform of hypothesis h of frame f (the sampled rows are read from global memory twice: centroids, then S)
__device__ __forceinline__ void pose_hypothesis(const PoseArgs &a, int f, int h, PoseRT &o)
{
    const uint32_t key = pose_key(a.seed, f, h);
    const float *src = a.src + (long)f * a.N * a.rs, *dst = a.dst + (long)f * a.N * a.rs;
    double ca[3] = {0.0, 0.0, 0.0}, cb[3] = {0.0, 0.0, 0.0}, S[9];
    for (int j = 0; j < a.n; ++j) {
        const long i = (long)(pose_mix(key ^ (uint32_t)j) % (uint32_t)a.N) * a.rs;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            ca[c] = ca[c] + (double)src[i + c];
            cb[c] = cb[c] + (double)dst[i + c];
        }
    }
    const double dn = (double)a.n;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ca[c] = ca[c] / dn;
        cb[c] = cb[c] / dn;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) S[k] = 0.0;
    for (int j = 0; j < a.n; ++j) {
        const long i = (long)(pose_mix(key ^ (uint32_t)j) % (uint32_t)a.N) * a.rs;
        const double ax = (double)src[i] - ca[0], ay = (double)src[i + 1] - ca[1], az = (double)src[i + 2] - ca[2];
        const double bx = (double)dst[i] - cb[0], by = (double)dst[i + 1] - cb[1], bz = (double)dst[i + 2] - cb[2];
        S[0] = S[0] + ax * bx; S[1] = S[1] + ax * by; S[2] = S[2] + ax * bz;
        S[3] = S[3] + ay * bx; S[4] = S[4] + ay * by; S[5] = S[5] + ay * bz;
        S[6] = S[6] + az * bx; S[7] = S[7] + az * by; S[8] = S[8] + az * bz;
    }
    pose_horn(S, ca, cb, o);
}

// squared residual of one correspondence, in the order the restatement evaluates it
__device__ __forceinline__ double pose_d2(const PoseRT &m, double sx, double sy, double sz, double dx, double dy, double dz)
{
    const double rx = (((m.r[0] * sx + m.r[1] * sy) + m.r[2] * sz) + m.t[0]) - dx;
    const double ry = (((m.r[3] * sx + m.r[4] * sy) + m.r[5] * sz) + m.t[1]) - dy;
    const double rz = (((m.r[6] * sx + m.r[7] * sy) + m.r[8] * sz) + m.t[2]) - dz;
    return (rx * rx + ry * ry) + rz * rz;
}

__device__ __forceinline__ double pose_rmse(int cnt, double sum) { return cnt > 0 ? sqrt(sum / (double)cnt) : 0.0; }

// grid (ceil(K / 256), F): lane = hypothesis; ws_cnt / ws_rmse (F, K)
__global__ __launch_bounds__(POSE_BLOCK) void pose_score_kernel(PoseArgs a, int *__restrict__ ws_cnt, double *__restrict__ ws_rmse)
{
    __shared__ f32x4 pts[POSE_TILE * 2];   // point i: {sx, sy, sz, 0}, {dx, dy, dz, 0}
    const int f = blockIdx.y, tid = threadIdx.x, h = blockIdx.x * POSE_BLOCK + tid;
    PoseRT m;
    pose_hypothesis(a, f, h < a.K ? h : a.K - 1, m);   // lanes past K compute a real hypothesis and write nothing
    const float *src = a.src + (long)f * a.N * a.rs, *dst = a.dst + (long)f * a.N * a.rs;
    int cnt = 0;
    double sum = 0.0;
    for (int base = 0; base < a.N; base += POSE_TILE) {
        const int tile = min(POSE_TILE, a.N - base);
        __syncthreads();
        for (int i = tid; i < tile; i += POSE_BLOCK) {
            const long g = (long)(base + i) * a.rs;
            f32x4 s, d;
            s.x = src[g]; s.y = src[g + 1]; s.z = src[g + 2]; s.w = 0.f;
            d.x = dst[g]; d.y = dst[g + 1]; d.z = dst[g + 2]; d.w = 0.f;
            pts[2 * i] = s;
            pts[2 * i + 1] = d;
        }
        __syncthreads();
        for (int i = 0; i < tile; ++i) {
            const f32x4 s = pts[2 * i], d = pts[2 * i + 1];
            const double d2 = pose_d2(m, (double)s.x, (double)s.y, (double)s.z, (double)d.x, (double)d.y, (double)d.z);
            const bool in = d2 < a.thr2;
            cnt += in ? 1 : 0;
            sum = sum + (in ? d2 : 0.0);
        }
    }
    if (h < a.K) {
        ws_cnt[(long)f * a.K + h] = cnt;
        ws_rmse[(long)f * a.K + h] = pose_rmse(cnt, sum);
    }
}

__device__ __forceinline__ bool pose_better(int c1, double r1, int h1, int c2, double r2, int h2)
{
    return c1 != c2 ? c1 > c2 : (r1 != r2 ? r1 < r2 : h1 < h2);
}

// fixed-shape tree sum over the workgroup (the same pairing on every run); every thread returns the total
__device__ double pose_block_sum(double v, double *red)
{
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int w = POSE_BLOCK / 2; w >= 1; w >>= 1) {
        if (tid < w) red[tid] = red[tid] + red[tid + w];
        __syncthreads();
    }
    return red[0];
}

// the inliers of transform m over the whole frame: count and sum of d2 (each thread a strided subset in order, then the tree)
__device__ void pose_score_frame(const PoseArgs &a, const float *src, const float *dst, const PoseRT &m, double *red, int &cnt, double &sum)
{
    double c = 0.0, s = 0.0;
    for (int i = threadIdx.x; i < a.N; i += POSE_BLOCK) {
        const long g = (long)i * a.rs;
        const double d2 = pose_d2(m, (double)src[g], (double)src[g + 1], (double)src[g + 2], (double)dst[g], (double)dst[g + 1], (double)dst[g + 2]);
        const bool in = d2 < a.thr2;
        c = c + (in ? 1.0 : 0.0);
        s = s + (in ? d2 : 0.0);
    }
    cnt = (int)pose_block_sum(c, red);
    sum = pose_block_sum(s, red);
}

// grid F, one workgroup per frame
__global__ __launch_bounds__(POSE_BLOCK) void pose_select_kernel(PoseArgs a, int refine, const int *__restrict__ ws_cnt, const double *__restrict__ ws_rmse,
                                                                double *__restrict__ T, int *__restrict__ inliers, double *__restrict__ rmse, int *__restrict__ best)
{
    __shared__ double red[POSE_BLOCK];
    __shared__ int redc[POSE_BLOCK], redh[POSE_BLOCK];
    __shared__ PoseRT win;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int *cnt = ws_cnt + (long)f * a.K;
    const double *rm = ws_rmse + (long)f * a.K;
    int bc = -1, bh = a.K;
    double br = 0.0;
    for (int h = tid; h < a.K; h += POSE_BLOCK) {
        if (pose_better(cnt[h], rm[h], h, bc, br, bh)) { bc = cnt[h]; br = rm[h]; bh = h; }
    }
    redc[tid] = bc; red[tid] = br; redh[tid] = bh;
    __syncthreads();
    for (int w = POSE_BLOCK / 2; w >= 1; w >>= 1) {
        if (tid < w && pose_better(redc[tid + w], red[tid + w], redh[tid + w], redc[tid], red[tid], redh[tid])) {
            redc[tid] = redc[tid + w]; red[tid] = red[tid + w]; redh[tid] = redh[tid + w];
        }
        __syncthreads();
    }
    const int hbest = redh[0];
    int c_out = redc[0];
    double r_out = red[0];
    if (tid == 0) {
        PoseRT m;
        pose_hypothesis(a, f, hbest, m);
        win = m;
    }
    __syncthreads();
    if (refine && c_out >= 3) {
        const float *src = a.src + (long)f * a.N * a.rs, *dst = a.dst + (long)f * a.N * a.rs;
        const PoseRT m = win;
        double ls[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = tid; i < a.N; i += POSE_BLOCK) {
            const long g = (long)i * a.rs;
            const double sx = src[g], sy = src[g + 1], sz = src[g + 2], dx = dst[g], dy = dst[g + 1], dz = dst[g + 2];
            const bool in = pose_d2(m, sx, sy, sz, dx, dy, dz) < a.thr2;
            ls[0] = ls[0] + (in ? sx : 0.0); ls[1] = ls[1] + (in ? sy : 0.0); ls[2] = ls[2] + (in ? sz : 0.0);
            ls[3] = ls[3] + (in ? dx : 0.0); ls[4] = ls[4] + (in ? dy : 0.0); ls[5] = ls[5] + (in ? dz : 0.0);
        }
        double ca[3], cb[3], S[9];
        const double dn = (double)c_out;
        for (int c = 0; c < 3; ++c) {
            ca[c] = pose_block_sum(ls[c], red) / dn;
            cb[c] = pose_block_sum(ls[3 + c], red) / dn;
        }
        double lS[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = tid; i < a.N; i += POSE_BLOCK) {
            const long g = (long)i * a.rs;
            const double sx = src[g], sy = src[g + 1], sz = src[g + 2], dx = dst[g], dy = dst[g + 1], dz = dst[g + 2];
            const bool in = pose_d2(m, sx, sy, sz, dx, dy, dz) < a.thr2;
            const double ax = in ? sx - ca[0] : 0.0, ay = in ? sy - ca[1] : 0.0, az = in ? sz - ca[2] : 0.0;
            const double bx = in ? dx - cb[0] : 0.0, by = in ? dy - cb[1] : 0.0, bz = in ? dz - cb[2] : 0.0;
            lS[0] = lS[0] + ax * bx; lS[1] = lS[1] + ax * by; lS[2] = lS[2] + ax * bz;
            lS[3] = lS[3] + ay * bx; lS[4] = lS[4] + ay * by; lS[5] = lS[5] + ay * bz;
            lS[6] = lS[6] + az * bx; lS[7] = lS[7] + az * by; lS[8] = lS[8] + az * bz;
        }
        for (int k = 0; k < 9; ++k) S[k] = pose_block_sum(lS[k], red);
        __syncthreads();
        if (tid == 0) {
            PoseRT r;
            pose_horn(S, ca, cb, r);
            win = r;
        }
        __syncthreads();
        const PoseRT r = win;
        double sum;
        pose_score_frame(a, src, dst, r, red, c_out, sum);
        r_out = pose_rmse(c_out, sum);
    }
    if (tid == 0) {
        double *o = T + (long)f * 16;
        for (int i = 0; i < 3; ++i) {
            o[4 * i] = win.r[3 * i]; o[4 * i + 1] = win.r[3 * i + 1]; o[4 * i + 2] = win.r[3 * i + 2]; o[4 * i + 3] = win.t[i];
        }
        o[12] = 0.0; o[13] = 0.0; o[14] = 0.0; o[15] = 1.0;
        inliers[f] = c_out;
        rmse[f] = r_out;
        best[f] = hbest;
    }
}

static long pose_align(long b) { return (b + 255) & ~255L; }

extern "C" long caspr_pose_ransac_ws_bytes(int F, int N, int K)
{
    (void)N;
    if (F <= 0 || K <= 0) return 256;
    return pose_align((long)F * K * 8) + pose_align((long)F * K * 4);
}

extern "C" int caspr_pose_ransac_f32(const float *src, const float *dst, int F, int N, int row_stride, int K, int n, double threshold,
                                     unsigned long long seed, int refine, double *T, int *inliers, double *rmse, int *best, void *ws,
                                     long ws_bytes, void *stream)
{
    CASPR_REQUIRE(src && dst && T && inliers && rmse && best && ws, "pose_ransac: null pointer");
    CASPR_REQUIRE(F > 0 && K > 0, "pose_ransac: F = %d, K = %d (both must be positive)", F, K);
    CASPR_REQUIRE(n >= 3 && n <= POSE_MAX_N, "pose_ransac: sample size %d outside 3..%d", n, POSE_MAX_N);
    CASPR_REQUIRE(N >= n, "pose_ransac: N = %d correspondences, fewer than the sample size %d", N, n);
    CASPR_REQUIRE(row_stride == 3 || row_stride == 4, "pose_ransac: row_stride %d (3 or 4)", row_stride);
    CASPR_REQUIRE(threshold > 0.0 && threshold < 1e150, "pose_ransac: threshold %g must be positive and finite", threshold);
    CASPR_REQUIRE(refine == 0 || refine == 1, "pose_ransac: refine %d (0 or 1)", refine);
    CASPR_REQUIRE(ws_bytes >= caspr_pose_ransac_ws_bytes(F, N, K), "pose_ransac: workspace too small");
    PoseArgs a{src, dst, N, row_stride, K, n, threshold * threshold, seed};
    double *ws_rmse = (double *)ws;
    int *ws_cnt = (int *)((char *)ws + pose_align((long)F * K * 8));
    pose_score_kernel<<<dim3(ceil_div(K, POSE_BLOCK), F), dim3(POSE_BLOCK), 0, (hipStream_t)stream>>>(a, ws_cnt, ws_rmse);
    CASPR_CHECK_LAUNCH("pose_score");
    pose_select_kernel<<<dim3(F), dim3(POSE_BLOCK), 0, (hipStream_t)stream>>>(a, refine, ws_cnt, ws_rmse, T, inliers, rmse, best);
    CASPR_CHECK_LAUNCH("pose_select");
    return CASPR_OK;
}
