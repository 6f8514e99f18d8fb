// ode_latent_dp5.h -- what the adaptive latent solve (ode_latent_dp5.hip: latent_dp5_kernel<TAPE>) and its reverse sweep
// (ode_latent_dp5_adjoint.inc: latent_dp5_adjoint_kernel) share: the column / trace layout and the streamed matrix product of one
// layer.  The evaluation itself (four layers around these products) is the text of ode_latent_dp5_eval.inc.
#pragma once
#include <math.h>
#include <stdlib.h>

#include "common.h"

#define LDP_NCOL 16
#define LDP_EL (64 * LDP_NCOL)    // one state array: [d][c]
#define LDP_TRACE_HEAD 8          // floats per sequence before the attempt rows: d0, d1, d2, h0, first dt, 0, 0, 0
#define LDP_TRACE_ROW 4           // per attempt: t, dt, ratio, accepted (1 / 0)

// out rows [16*rt0, 16*(rt0+nrt)) of W (packed, KC chunks) times the B-tile `in`; epilogue(rt, acc)   (lat_layer of ode.hip)
template <int NRT, typename Epi>
__device__ __forceinline__ void ldp_layer(const float *__restrict__ wp, int KC, int rt0, const float *in, int lane, Epi epi)
{
    // One CU streams the whole weight set from L2 every evaluation: keep 4 chunks (4 x NRT KiB per wave,
    // 128 KiB per workgroup) of A fragments in flight in a register ring to cover the L2 latency.
    const int g = lane >> 4, j = lane & 15;
    f32x4 acc[NRT];
#pragma unroll
    for (int i = 0; i < NRT; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float *wb = wp + ((long)rt0 * KC) * 256 + lane * 4;
    f32x4 ring[4][NRT];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < NRT; ++i) ring[s][i] = ld4(wb + ((long)i * KC + (s < KC ? s : 0)) * 256);
    for (int kc0 = 0; kc0 < KC; kc0 += 4) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int kc = kc0 + s;
            if (kc < KC) {
                const f32x4 bf = ld4(in + btile_off(kc * 4 + g, j, LDP_NCOL));
#pragma unroll
                for (int i = 0; i < NRT; ++i) {
                    const f32x4 af = ring[s][i];
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[i] = mfma16(af[q], bf[q], acc[i]);
                }
                const int kn = (kc + 4 < KC) ? kc + 4 : kc;
#pragma unroll
                for (int i = 0; i < NRT; ++i) ring[s][i] = ld4(wb + ((long)i * KC + kn) * 256);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NRT; ++i) epi(rt0 + i, acc[i]);
}

// sum over the 64 lanes in one fixed order; every lane returns the same bits (a + b == b + a)
__device__ __forceinline__ double ldp_wave_sum(double v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}
