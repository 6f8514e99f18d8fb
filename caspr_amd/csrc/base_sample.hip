// base_sample.hip -- the decoder's base-distribution draw on the device (models/caspr.py: decode with base_sampler="device";
// reference: caspr.py:228-258 with models/utils.py:10-29 and transform_utils.py:80-85, which draw on the host generators).
//
// One launch writes y (F, n, 3) f32 and logp_y (F, n) = sum_c (-0.5 log(2 pi) - 0.5 y_c^2), the value
// standard_normal_logprob(y).sum(2) gives on the rounded f32 y: per component (-C) - ((0.5 * y) * y) with C = (float)(0.5 log(2 pi)),
// the three components added as (l0 + l2) + l1 -- the order in which ATen's reduction kernel adds a contiguous dimension of three on
// ROCm (two lanes per output, lane 0 holds l0 + l2, lane 1 holds l1; tests/test_base_sample.py::test_logp_bit_exact).  Built with
// -ffp-contract=off (build.py): every expression rounds as written.
//
// Generator   Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), one block of four
//             32-bit words per call:
//               key     = (seed & 0xffffffff, seed >> 32)
//               counter = (point index i,  frame_ids[f] & 0xffffffff,  frame_ids[f] >> 32 (as unsigned),  (draw << 4) | block)
//             with 0 <= draw < 2^28 and block < 16.  frame_ids is read from device memory: a sample is a function of
//             (seed, draw, frame id, point, block, word) and of nothing else -- not of F, of the launch geometry, or of which
//             rows share a launch -- so a batch split over several launches or ranks draws the same samples.
// Uniform     word x -> k = x >> 8 (24 bits) -> u = (k + 0.5) 2^-24, in (0, 1).  k + 0.5 needs 25 significant bits for
//             k >= 2^23, so the kernel never forms u in f32 where that would round; it uses the two exact values
//               w = (min(k, 2^24 - 1 - k) + 0.5) 2^-24   (u itself below one half, 1 - u above)
//               v = ((k - 2^23) + 0.5) 2^-23 = 2 u - 1   (|k - 2^23| <= 2^23: exact, and never 0)
// Normal      Box-Muller on a pair of words (x0, x1): r = sqrt(-2 ln u(x0)), ln u = logf(w) below one half and log1pf(-w) above;
//             (r cos(2 pi u(x1)), r sin(2 pi u(x1))) = (-r cospi(v(x1)), -r sinpi(v(x1))).  A block gives four normals:
//             words (0, 1) -> c0, c1; words (2, 3) -> c2, c3.
// Modes       Gaussian:  y = (c0, c1, c2) of block 0.
//             Truncated (trunc_std > 0, models/utils.py:truncated_normal): component c takes block c; its value is the first of
//               the block's four candidates with |candidate| < trunc_std, candidate 0 if none qualifies.
//             Contours (radii != null, caspr.py:232-250): point i belongs to contour min(i / (n / R), R - 1) (integer division;
//               n < R: all to the last) -- the first R - 1 contours get n / R points each, the last the rest --, and is
//               radius * cube / |cube| with cube = (v(x0), v(x1), v(x2)) of block 0 (sphere_surface_points).  No component of
//               cube can be 0 (v is an odd multiple of 2^-24), so |cube| > 0: no branch for a zero-length draw.
// raw         (optional, (F, n, 4) int32) receives the four words of block 0 of every point, in every mode.
//
// Geometry: one lane per point, BS_BLOCK lanes per workgroup, ceil(n / BS_BLOCK) workgroups per frame; the lanes past n of a
// frame's last workgroup return before any store.
#include "common.h"

#include <cmath>

#define BS_BLOCK 64

struct BaseSampleArgs {
    const long long *frame_ids;
    const float *radii;
    float *y, *logp;
    int *raw;
    int n, R, groups_per_frame;
    unsigned int k0, k1, draw;
    float trunc_std;
};

struct BsWords {
    uint32_t w[4];
};

__device__ __forceinline__ BsWords bs_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        if (r < 9) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
    }
    return BsWords{{c0, c1, c2, c3}};
}

// 2 u - 1 of a word, exact
__device__ __forceinline__ float bs_signed(uint32_t x)
{
    return ((float)((int)(x >> 8) - (1 << 23)) + 0.5f) * 0x1p-23f;
}

// the two normals of a pair of words
__device__ __forceinline__ void bs_normal_pair(uint32_t x0, uint32_t x1, float &a, float &b)
{
    const uint32_t k = x0 >> 8;
    const bool low = k < (1u << 23);
    const float w = ((float)(low ? k : 0xFFFFFFu - k) + 0.5f) * 0x1p-24f;
    const float ln_u = low ? logf(w) : log1pf(-w);
    const float r = sqrtf(-2.0f * ln_u);
    float s, c;
    sincospif(bs_signed(x1), &s, &c);
    a = -(r * c);
    b = -(r * s);
}

__device__ __forceinline__ float bs_logp(float y)
{
    return (float)-0.91893853320467274178 - (0.5f * y) * y;   // the double 0.5 log(2 pi) narrowed, as ATen narrows the Python scalar
}

__global__ __launch_bounds__(BS_BLOCK) void base_sample_kernel(BaseSampleArgs a)
{
    const int f = blockIdx.x / a.groups_per_frame;
    const int i = (blockIdx.x - f * a.groups_per_frame) * BS_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const unsigned long long fid = (unsigned long long)a.frame_ids[f];
    const uint32_t c1 = (uint32_t)fid, c2 = (uint32_t)(fid >> 32), c3 = a.draw << 4;
    const size_t p = (size_t)f * a.n + i;
    const BsWords b0 = bs_philox((uint32_t)i, c1, c2, c3, a.k0, a.k1);
    if (a.raw) {
#pragma unroll
        for (int q = 0; q < 4; ++q) a.raw[p * 4 + q] = (int)b0.w[q];
    }
    float y[3];
    if (a.radii) {
        const int per = a.n / a.R;
        const int ci = per > 0 ? min(i / per, a.R - 1) : a.R - 1;
        const float radius = a.radii[ci];
        const float v0 = bs_signed(b0.w[0]), v1 = bs_signed(b0.w[1]), v2 = bs_signed(b0.w[2]);
        const float norm = sqrtf((v0 * v0 + v1 * v1) + v2 * v2);
        y[0] = (radius * v0) / norm;
        y[1] = (radius * v1) / norm;
        y[2] = (radius * v2) / norm;
    } else if (a.trunc_std > 0.0f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const BsWords b = c == 0 ? b0 : bs_philox((uint32_t)i, c1, c2, c3 | (uint32_t)c, a.k0, a.k1);
            float cand[4];
            bs_normal_pair(b.w[0], b.w[1], cand[0], cand[1]);
            bs_normal_pair(b.w[2], b.w[3], cand[2], cand[3]);
            float pick = cand[0];
#pragma unroll
            for (int q = 3; q >= 0; --q) pick = fabsf(cand[q]) < a.trunc_std ? cand[q] : pick;   // the lowest qualifying q wins
            y[c] = pick;
        }
    } else {
        float unused;
        bs_normal_pair(b0.w[0], b0.w[1], y[0], y[1]);
        bs_normal_pair(b0.w[2], b0.w[3], y[2], unused);
    }
    a.y[p * 3 + 0] = y[0];
    a.y[p * 3 + 1] = y[1];
    a.y[p * 3 + 2] = y[2];
    a.logp[p] = (bs_logp(y[0]) + bs_logp(y[2])) + bs_logp(y[1]);   // the order of ATen's sum over a contiguous dimension of three (header)
}

extern "C" int caspr_base_sample_f32(int F, int n, unsigned long long seed, unsigned int draw, const long long *frame_ids,
                                     float trunc_std, const float *radii, int R, float *y, float *logp, int *raw, void *stream)
{
    CASPR_REQUIRE(frame_ids && y && logp, "base_sample: null pointer");
    CASPR_REQUIRE(F > 0 && n > 0, "base_sample: F = %d, n = %d (both must be positive)", F, n);
    CASPR_REQUIRE(draw < (1u << 28), "base_sample: draw number %u does not fit 28 bits", draw);
    CASPR_REQUIRE(std::isfinite(trunc_std), "base_sample: trunc_std must be finite");
    CASPR_REQUIRE(trunc_std >= 0.0f, "base_sample: trunc_std %g is negative (0 = no truncation)", (double)trunc_std);
    CASPR_REQUIRE(radii ? R >= 1 : R == 0, "base_sample: R = %d (>= 1 with radii, 0 without)", R);
    CASPR_REQUIRE(!(radii && trunc_std > 0.0f), "base_sample: contours and truncation exclude each other");
    const long groups = (long)ceil_div(n, BS_BLOCK);
    CASPR_REQUIRE(groups * F < (1l << 31), "base_sample: F = %d frames of n = %d points exceed the grid", F, n);
    BaseSampleArgs a{frame_ids, radii, y, logp, raw, n, R, (int)groups, (unsigned int)seed, (unsigned int)(seed >> 32), draw, trunc_std};
    base_sample_kernel<<<dim3((unsigned)(groups * F)), dim3(BS_BLOCK), 0, (hipStream_t)stream>>>(a);
    CASPR_CHECK_LAUNCH("base_sample");
    return CASPR_OK;
}
