// backward_flow_value.hip -- training tier, part 4: the gated softplus layers of the CNF's ODE function (ConcatSquashLinear +
// Softplus, diffeq_layers.py:83-90 / odefunc.py:98-105) on VALUE rows only, forward and backward, for the gradient of the
// SAMPLING solve (cnf.py:70-128 with reverse = True and logpx = None, as caspr.py:262 runs it in decode(); train/flow_grad.py:
// CnfSampleSolve).  That direction carries no Hutchinson tangent and no log-density, so the (2R, C) value | tangent tensors of
// backward_flow.hip would be half zeros; these kernels work on R = frames x n rows, point p in row p, frame f = p / n:
//
//   a = (Z[p] + b) g[f] + beta[f]     H[p] = softplus(a)
//   backward, given dH:   da = dH s (s = sigmoid(a))    dZ = da g    dg[f] = sum_{p in f} da (Z[p] + b)    dbeta[f] = sum_{p in f} da
//
// Only Z is kept between the two passes; a and s are recomputed.  Memory-bound element-wise work with per-frame reductions: a
// thread owns FOUR consecutive channels (16-byte loads and stores), a wave 256 channels of one point at a time (whatever is per
// point -- y, dZo -- is a wave-uniform address), a workgroup = (256-channel chunk, frame, point split).  Every per-frame sum is taken
// in a fixed order -- points of a split by the four waves in turn, the waves' partials in LDS, the splits by the caller -- with no
// atomics: two runs give the same bits.  There are no padding rows: any n >= 1, and a row past R is never read or written.
#include "common.h"

#define CV_CHUNK 256              // channels per workgroup: 64 lanes x 4

static __device__ __forceinline__ float cv_readlane(float v, int l)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
static __device__ __forceinline__ float cv_wave_sum(float v)   // uniform result: DPP row sums, then the four rows
{
    v = row_allreduce_add<16>(v);
    return (cv_readlane(v, 0) + cv_readlane(v, 16)) + (cv_readlane(v, 32) + cv_readlane(v, 48));
}
// softplus and sigmoid of a from one 2^(-|a| log2 e) on the hardware transcendentals (as cnf_in_fwd_rows_kernel of backward_flow.hip)
static __device__ __forceinline__ float cv_sigmoid(float a)
{
    const float u = __builtin_amdgcn_exp2f(fabsf(a) * -1.44269504088896341f);
    const float rc = __builtin_amdgcn_rcpf(1.0f + u);
    return a >= 0.0f ? rc : u * rc;
}

// point splits of the backward kernels for n points per frame (the caller sizes the dgate / dbeta / dW0 partials with it)
extern "C" int caspr_cnf_value_splits(int n) { return n >= 256 ? 8 : 1; }

// ---------------------------------------------------------------------------------------------
// First layer (3 -> C): H = softplus((W0 y + b0) g[f] + beta[f]).  K = 3: three FMAs per output, a pure streaming write of H.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cnf_in_value_fwd_kernel(const float *__restrict__ Yp, const float *__restrict__ W0,
                                                               const float *__restrict__ b, const float *__restrict__ gate,
                                                               const float *__restrict__ beta, int n, int C, float *__restrict__ H, int ldh)
{
    const int lane = threadIdx.x & 63;
    const int sub = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = blockIdx.z * CV_CHUNK + lane * 4;
    const long f = blockIdx.y;
    if (c >= C) return;
    float w[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int d = 0; d < 3; ++d) w[q][d] = W0[(long)(c + q) * 3 + d];
    const f32x4 bb = ld4(b + c), g = ld4(gate + f * C + c), be = ld4(beta + f * C + c);
    const int p_end = (blockIdx.x * 32 + 32) < n ? (blockIdx.x * 32 + 32) : n;
    for (int pi = blockIdx.x * 32 + sub; pi < p_end; pi += 4) {
        const long pt = f * n + pi;
        const float *yp = Yp + pt * 3;                                   // wave-uniform address
        const float y0 = yp[0], y1 = yp[1], y2 = yp[2];
        f32x4 hv;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float zv = (w[q][0] * y0 + w[q][1] * y1) + w[q][2] * y2;
            hv[q] = softplus_fast((zv + bb[q]) * g[q] + be[q]);
        }
        st4(H + pt * ldh + c, hv);
    }
}

// Backward: recomputes W0 y from y.  Partials per point split, summed by the caller: dgate / dbeta (frames, nsplit, C),
// dW0 (frames * nsplit, C, 3), dy (chunks, R, 3) = per-chunk sums over the chunk's channels of dZ W0.
__global__ __launch_bounds__(256) void cnf_in_value_bwd_kernel(const float *__restrict__ Yp, const float *__restrict__ W0,
                                                               const float *__restrict__ b, const float *__restrict__ gate,
                                                               const float *__restrict__ beta, const float *__restrict__ dH, int ldd,
                                                               long R, int n, int C, int nsplit, float *__restrict__ dgate,
                                                               float *__restrict__ dbeta, float *__restrict__ dW0p, float *__restrict__ dYp)
{
    __shared__ float s_red[3][64][20];
    const int lane = threadIdx.x & 63;
    const int sub = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int chunk = blockIdx.x, c = chunk * CV_CHUNK + lane * 4;
    const bool ok = c < C;
    const long f = blockIdx.y;
    const int ps = blockIdx.z, per = (n + nsplit - 1) / nsplit;
    const int p_beg = ps * per, p_end = (p_beg + per) < n ? (p_beg + per) : n;
    float w[4][3];
    f32x4 bb = (f32x4){0.f, 0.f, 0.f, 0.f}, g = bb, be = bb;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int d = 0; d < 3; ++d) w[q][d] = ok ? W0[(long)(c + q) * 3 + d] : 0.f;
    if (ok) { bb = ld4(b + c); g = ld4(gate + f * C + c); be = ld4(beta + f * C + c); }
    float acc[20];                 // [q]: dgate, [4 + q]: dbeta, [8 + 3 q + d]: dW0
#pragma unroll
    for (int k = 0; k < 20; ++k) acc[k] = 0.f;
    for (int pi = p_beg + sub; pi < p_end; pi += 4) {
        const long pt = f * n + pi;
        const float *yp = Yp + pt * 3;                                   // wave-uniform
        const float y0 = yp[0], y1 = yp[1], y2 = yp[2];
        f32x4 dh = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (ok) dh = ld4(dH + pt * ldd + c);
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float zb = ((w[q][0] * y0 + w[q][1] * y1) + w[q][2] * y2) + bb[q];
            const float da = dh[q] * cv_sigmoid(zb * g[q] + be[q]);
            const float dz = da * g[q];
            acc[q] += da * zb;
            acc[4 + q] += da;
            acc[8 + 3 * q] += dz * y0;
            acc[9 + 3 * q] += dz * y1;
            acc[10 + 3 * q] += dz * y2;
            d0 += dz * w[q][0];
            d1 += dz * w[q][1];
            d2 += dz * w[q][2];
        }
        d0 = cv_wave_sum(d0); d1 = cv_wave_sum(d1); d2 = cv_wave_sum(d2);
        if (lane == 0) {
            float *o = dYp + ((long)chunk * R + pt) * 3;
            o[0] = d0; o[1] = d1; o[2] = d2;
        }
    }
    if (sub > 0) {
#pragma unroll
        for (int k = 0; k < 20; ++k) s_red[sub - 1][lane][k] = acc[k];
    }
    __syncthreads();
    if (sub == 0 && ok) {
#pragma unroll
        for (int k = 0; k < 20; ++k) acc[k] = (acc[k] + s_red[0][lane][k]) + (s_red[1][lane][k] + s_red[2][lane][k]);
        const long fs = f * nsplit + ps;
        st4(dgate + fs * C + c, (f32x4){acc[0], acc[1], acc[2], acc[3]});
        st4(dbeta + fs * C + c, (f32x4){acc[4], acc[5], acc[6], acc[7]});
        float *o = dW0p + (fs * C + c) * 3;
#pragma unroll
        for (int k = 0; k < 12; ++k) o[k] = acc[8 + k];
    }
}

// ---------------------------------------------------------------------------------------------
// Hidden activation on a given product Z (R, ldz)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cnf_act_value_fwd_kernel(const float *__restrict__ Z, int ldz, const float *__restrict__ b,
                                                                const float *__restrict__ gate, const float *__restrict__ beta,
                                                                long R, int n, int C, float *__restrict__ H, int ldh)
{
    const int C4 = C >> 2;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= R * C4) return;
    const long pt = t / C4;
    const int c = (int)(t % C4) * 4;
    const long f = pt / n;
    const f32x4 zv = ld4(Z + pt * ldz + c), bb = ld4(b + c), g = ld4(gate + f * C + c), be = ld4(beta + f * C + c);
    f32x4 hv;
#pragma unroll
    for (int q = 0; q < 4; ++q) hv[q] = softplus_fast((zv[q] + bb[q]) * g[q] + be[q]);
    st4(H + pt * ldh + c, hv);
}

// dH == NULL: the layer feeds the 3-channel output layer directly (odefunc.py:103, no activation behind it) and its dH is that layer's
// data gradient dH[p][c] = sum_j dZo[p][j] Wo[j][c], formed here (three FMAs per element) instead of being written by a K = 3 conv.
// dgate / dbeta (frames, nsplit, C): partials per point split.
__global__ __launch_bounds__(256) void cnf_act_value_bwd_kernel(const float *__restrict__ Z, int ldz, const float *__restrict__ b,
                                                                const float *__restrict__ gate, const float *__restrict__ beta,
                                                                const float *__restrict__ dH, int ldd, const float *__restrict__ dZo, int ldo,
                                                                const float *__restrict__ Wo, int ldw, int n, int C, int nsplit,
                                                                float *__restrict__ dZ, int lddz, float *__restrict__ dgate,
                                                                float *__restrict__ dbeta)
{
    __shared__ float s_red[3][64][8];
    const int lane = threadIdx.x & 63;
    const int sub = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = blockIdx.x * CV_CHUNK + lane * 4;
    const bool ok = c < C;
    const long f = blockIdx.y;
    const int ps = blockIdx.z, per = (n + nsplit - 1) / nsplit;
    const int p_beg = ps * per, p_end = (p_beg + per) < n ? (p_beg + per) : n;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // [q]: dgate, [4 + q]: dbeta
    if (ok) {
        const f32x4 bb = ld4(b + c), g = ld4(gate + f * C + c), be = ld4(beta + f * C + c);
        f32x4 w0 = (f32x4){0.f, 0.f, 0.f, 0.f}, w1 = w0, w2 = w0;
        if (!dH) { w0 = ld4(Wo + c); w1 = ld4(Wo + ldw + c); w2 = ld4(Wo + 2 * (long)ldw + c); }
        for (int pi = p_beg + sub; pi < p_end; pi += 4) {
            const long pt = f * n + pi;
            const f32x4 zv = ld4(Z + pt * ldz + c);
            f32x4 dh, dz;
            if (dH) {
                dh = ld4(dH + pt * ldd + c);
            } else {
                const float *o = dZo + pt * ldo;                         // wave-uniform row
                const float o0 = o[0], o1 = o[1], o2 = o[2];
#pragma unroll
                for (int q = 0; q < 4; ++q) dh[q] = (o0 * w0[q] + o1 * w1[q]) + o2 * w2[q];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float zb = zv[q] + bb[q];
                const float da = dh[q] * cv_sigmoid(zb * g[q] + be[q]);
                dz[q] = da * g[q];
                acc[q] += da * zb;
                acc[4 + q] += da;
            }
            st4(dZ + pt * lddz + c, dz);
        }
    }
    if (sub > 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) s_red[sub - 1][lane][k] = acc[k];
    }
    __syncthreads();
    if (sub == 0 && ok) {
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = (acc[k] + s_red[0][lane][k]) + (s_red[1][lane][k] + s_red[2][lane][k]);
        const long fs = f * nsplit + ps;
        st4(dgate + fs * C + c, (f32x4){acc[0], acc[1], acc[2], acc[3]});
        st4(dbeta + fs * C + c, (f32x4){acc[4], acc[5], acc[6], acc[7]});
    }
}

// ---------------------------------------------------------------------------------------------
// Epilogue of the 3-channel output layer (odefunc.py:103-105): a[p][j] = (Zo[p][j] + b[j]) gate[f][j] + beta[f][j] = dy/dt.
// Backward: dZo (R, 4; column 3 zero), dgate / dbeta (frames, 3) summed over each frame's points in a fixed order.
// gate / beta are rows of a (frames, ldg) tensor.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cnf_out_value_fwd_kernel(const float *__restrict__ Zo, int ldo, const float *__restrict__ b,
                                                                const float *__restrict__ gate, const float *__restrict__ beta, int ldg,
                                                                long R, int n, float *__restrict__ A)
{
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= R) return;
    const long f = p / n;
#pragma unroll
    for (int j = 0; j < 3; ++j) A[p * 3 + j] = (Zo[p * ldo + j] + b[j]) * gate[f * ldg + j] + beta[f * ldg + j];
}

__global__ __launch_bounds__(256) void cnf_out_value_bwd_kernel(const float *__restrict__ dA, const float *__restrict__ Zo, int ldo,
                                                                const float *__restrict__ b, const float *__restrict__ gate, int ldg, int n,
                                                                float *__restrict__ dZo, float *__restrict__ dgate, float *__restrict__ dbeta)
{
    __shared__ float s_red[4][6];
    const long f = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float g[3], bb[3], acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 3; ++j) { g[j] = gate[f * ldg + j]; bb[j] = b[j]; }
    for (int pi = threadIdx.x; pi < n; pi += 256) {
        const long p = f * n + pi;
        f32x4 dv = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float da = dA[p * 3 + j];
            dv[j] = da * g[j];
            acc[j] += da * (Zo[p * ldo + j] + bb[j]);
            acc[3 + j] += da;
        }
        st4(dZo + p * 4, dv);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] = cv_wave_sum(acc[k]);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 6; ++k) s_red[wave][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < 6) {
        const float t = (s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + (s_red[2][threadIdx.x] + s_red[3][threadIdx.x]);
        if (threadIdx.x < 3) dgate[f * 3 + threadIdx.x] = t;
        else dbeta[f * 3 + threadIdx.x - 3] = t;
    }
}

// ---------------------------------------------------------------------------------------------
// entries (include/caspr_hip_train.h)
// ---------------------------------------------------------------------------------------------
static bool cv_al16(const void *p) { return ((uintptr_t)p % 16) == 0; }

extern "C" int caspr_cnf_in_value_f32(const float *Y, const float *W0, const float *b, const float *gate, const float *beta, long R, int n,
                                      int C, float *H, int ldh, void *stream)
{
    CASPR_REQUIRE(Y && W0 && b && gate && beta && H && R > 0 && n > 0 && R % n == 0 && C > 0 && C % 4 == 0 && ldh >= C && ldh % 4 == 0,
                  "cnf_in_value: bad arguments (C=%d must be a multiple of 4, R a multiple of n)", C);
    CASPR_REQUIRE(cv_al16(b) && cv_al16(gate) && cv_al16(beta) && cv_al16(H), "cnf_in_value: b, gate, beta, H must be 16-byte aligned");
    const long frames = R / n;
    CASPR_REQUIRE(frames <= 65535 && ceil_div(C, CV_CHUNK) <= 65535, "cnf_in_value: %ld frames > 65535", frames);
    cnf_in_value_fwd_kernel<<<dim3(ceil_div(n, 32), (unsigned)frames, ceil_div(C, CV_CHUNK)), dim3(256), 0, (hipStream_t)stream>>>(Y, W0, b, gate, beta, n, C,
                                                                                                                            H, ldh);
    CASPR_CHECK_LAUNCH("cnf_in_value");
    return CASPR_OK;
}

extern "C" int caspr_cnf_in_value_bwd_f32(const float *Y, const float *W0, const float *b, const float *gate, const float *beta, const float *dH,
                                          int ldd, long R, int n, int C, float *dgate, float *dbeta, float *dW0_part, float *dY_part, void *stream)
{
    CASPR_REQUIRE(Y && W0 && b && gate && beta && dH && dgate && dbeta && dW0_part && dY_part && R > 0 && n > 0 && R % n == 0 && C > 0 && C % 4 == 0 &&
                      ldd >= C && ldd % 4 == 0,
                  "cnf_in_value_bwd: bad arguments (C=%d must be a multiple of 4, R a multiple of n)", C);
    CASPR_REQUIRE(cv_al16(b) && cv_al16(gate) && cv_al16(beta) && cv_al16(dH) && cv_al16(dgate) && cv_al16(dbeta),
                  "cnf_in_value_bwd: b, gate, beta, dH, dgate, dbeta must be 16-byte aligned");
    const long frames = R / n;
    CASPR_REQUIRE(frames <= 65535, "cnf_in_value_bwd: %ld frames > 65535", frames);
    const int ns = caspr_cnf_value_splits(n);
    cnf_in_value_bwd_kernel<<<dim3(ceil_div(C, CV_CHUNK), (unsigned)frames, ns), dim3(256), 0, (hipStream_t)stream>>>(Y, W0, b, gate, beta, dH, ldd, R, n, C,
                                                                                                                    ns, dgate, dbeta, dW0_part, dY_part);
    CASPR_CHECK_LAUNCH("cnf_in_value_bwd");
    return CASPR_OK;
}

extern "C" int caspr_cnf_act_value_f32(const float *Z, int ldz, const float *b, const float *gate, const float *beta, long R, int n, int C,
                                       float *H, int ldh, void *stream)
{
    CASPR_REQUIRE(Z && b && gate && beta && H && R > 0 && n > 0 && R % n == 0 && C > 0 && C % 4 == 0 && ldz % 4 == 0 && ldh % 4 == 0 && ldz >= C &&
                      ldh >= C,
                  "cnf_act_value: bad arguments (C=%d must be a multiple of 4, R a multiple of n)", C);
    CASPR_REQUIRE(cv_al16(Z) && cv_al16(b) && cv_al16(gate) && cv_al16(beta) && cv_al16(H), "cnf_act_value: 16-byte alignment required");
    const long total = R * (C / 4);
    CASPR_REQUIRE((total + 255) / 256 <= 2147483647L, "cnf_act_value: too many rows");
    cnf_act_value_fwd_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(Z, ldz, b, gate, beta, R, n, C, H, ldh);
    CASPR_CHECK_LAUNCH("cnf_act_value");
    return CASPR_OK;
}

static int cnf_act_value_bwd_launch(const char *who, const float *Z, int ldz, const float *b, const float *gate, const float *beta, const float *dH,
                                    int ldd, const float *dZo, int ldo, const float *Wo, int ldw, long R, int n, int C, float *dZ, int lddz,
                                    float *dgate, float *dbeta, void *stream)
{
    CASPR_REQUIRE(Z && b && gate && beta && (dH || (dZo && Wo)) && dZ && dgate && dbeta && R > 0 && n > 0 && R % n == 0 && C > 0 && C % 4 == 0 &&
                      ldz >= C && ldz % 4 == 0 && (!dH || (ldd >= C && ldd % 4 == 0)) && lddz >= C && lddz % 4 == 0,
                  "%s: bad arguments (C=%d must be a multiple of 4, R a multiple of n)", who, C);
    CASPR_REQUIRE(cv_al16(Z) && cv_al16(b) && cv_al16(gate) && cv_al16(beta) && cv_al16(dH) && cv_al16(dZ) && cv_al16(dgate) && cv_al16(dbeta) &&
                      (dH || (cv_al16(Wo) && ldw % 4 == 0)),
                  "%s: 16-byte alignment required", who);
    const long frames = R / n;
    CASPR_REQUIRE(frames <= 65535, "%s: %ld frames > 65535", who, frames);
    const int ns = caspr_cnf_value_splits(n);
    cnf_act_value_bwd_kernel<<<dim3(ceil_div(C, CV_CHUNK), (unsigned)frames, ns), dim3(256), 0, (hipStream_t)stream>>>(Z, ldz, b, gate, beta, dH, ldd, dZo, ldo,
                                                                                                                     Wo, ldw, n, C, ns, dZ, lddz, dgate, dbeta);
    CASPR_CHECK_LAUNCH(who);
    return CASPR_OK;
}

extern "C" int caspr_cnf_act_value_bwd_f32(const float *Z, int ldz, const float *b, const float *gate, const float *beta, const float *dH, int ldd,
                                           long R, int n, int C, float *dZ, int lddz, float *dgate, float *dbeta, void *stream)
{
    CASPR_REQUIRE(dH, "cnf_act_value_bwd: dH is NULL");
    return cnf_act_value_bwd_launch("cnf_act_value_bwd", Z, ldz, b, gate, beta, dH, ldd, nullptr, 0, nullptr, 0, R, n, C, dZ, lddz, dgate, dbeta, stream);
}

// the same for the layer in front of the 3-channel output layer: dH = dZo Wo formed on the fly (dZo (R, ldo >= 3), Wo (3, ldw >= C))
extern "C" int caspr_cnf_act_value_bwd_out_f32(const float *Z, int ldz, const float *b, const float *gate, const float *beta, const float *dZo,
                                               int ldo, const float *Wo, int ldw, long R, int n, int C, float *dZ, int lddz, float *dgate,
                                               float *dbeta, void *stream)
{
    CASPR_REQUIRE(dZo && Wo && ldo >= 3 && ldw >= C, "cnf_act_value_bwd_out: bad arguments");
    return cnf_act_value_bwd_launch("cnf_act_value_bwd_out", Z, ldz, b, gate, beta, nullptr, 0, dZo, ldo, Wo, ldw, R, n, C, dZ, lddz, dgate, dbeta, stream);
}

extern "C" int caspr_cnf_out_value_f32(const float *Zo, int ldo, const float *b, const float *gate, const float *beta, int ldg, long R, int n,
                                       float *A, void *stream)
{
    CASPR_REQUIRE(Zo && b && gate && beta && A && R > 0 && n > 0 && R % n == 0 && ldo >= 3 && ldg >= 3, "cnf_out_value: bad arguments");
    CASPR_REQUIRE((R + 255) / 256 <= 2147483647L, "cnf_out_value: too many rows");
    cnf_out_value_fwd_kernel<<<dim3((unsigned)((R + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(Zo, ldo, b, gate, beta, ldg, R, n, A);
    CASPR_CHECK_LAUNCH("cnf_out_value");
    return CASPR_OK;
}

extern "C" int caspr_cnf_out_value_bwd_f32(const float *dA, const float *Zo, int ldo, const float *b, const float *gate, int ldg, long R, int n,
                                           float *dZo, float *dgate, float *dbeta, void *stream)
{
    CASPR_REQUIRE(dA && Zo && b && gate && dZo && dgate && dbeta && R > 0 && n > 0 && R % n == 0 && ldo >= 3 && ldg >= 3 && cv_al16(dZo),
                  "cnf_out_value_bwd: bad arguments");
    const long frames = R / n;
    CASPR_REQUIRE(frames <= 2147483647L, "cnf_out_value_bwd: too many frames");
    cnf_out_value_bwd_kernel<<<dim3((unsigned)frames), dim3(256), 0, (hipStream_t)stream>>>(dA, Zo, ldo, b, gate, ldg, n, dZo, dgate, dbeta);
    CASPR_CHECK_LAUNCH("cnf_out_value_bwd");
    return CASPR_OK;
}
