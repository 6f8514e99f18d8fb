// ode_bf16x6.hip -- the point-CNF solve (cnf.py:70-128) with the two 512x512 hidden layers on the bf16 matrix pipe in the
// exact three-way split of gemm_bf16x6.hip: the DEFAULT kernel of the CNF (ops.CNF_BF16X6; cnf_rk4_kernel of ode.hip is
// the f32-MFMA alternative).  Two instantiations: DIV = false integrates the state only (sampling, cnf.py:71-74 with
// logpx = None); DIV = true also integrates the Hutchinson divergence estimate (odefunc.py:119-142) for forward() / NLL:
// forward-mode tangents J e ride as the UPPER 8 columns of every wave's 16-column tile next to their 8 points (e^T J^T e ==
// e^T J e), the value column's pre-activation reaches its tangent column through one DPP row rotate per layer.
//
// Different geometry from the f32 kernel, forced by the 2.67x faster products (weights can no longer be streamed from L2
// into every wave's fragments: 4x the bytes per MFMA cycle):
//  * a 256-thread workgroup owns 64 points of one frame; WAVE w owns ALL 512 hidden units of its 16 points
//    (32 row tiles x 1 column tile = 128 accumulator registers), one wave per SIMD, one workgroup per CU;
//  * the hidden activation never touches LDS: an accumulator (D) fragment holds rows 4g..4g+3 of a 16-row tile for
//    column j, a bf16 B fragment holds 8 k-slots for column j -- two row tiles ARE one B fragment of the next layer
//    once the weight pack lists its k in the same order (slot s of lane group g <-> unit 32kc + 4g + s for s < 4,
//    32kc + 16 + 4g + s - 4 above);
//  * B fragments are produced WHILE the layer runs (pieces go k-chunk-major): chunk kc+1's input-layer values (layer 1)
//    or its slice of layer 1's epilogue (layer 2) are computed in quarters inside chunk kc's MFMA runs, hidden behind
//    the matrix pipe; two accumulator sets instead of 192 fragment registers;
//  * LDS is the weight stage shared by the four waves: 48 KB pieces (256 rows x 32 k x 3 planes, pre-swizzled image)
//    arrive by LDS-DMA, double-buffered, one raw s_barrier per piece of 96 MFMAs = 1536 matrix-pipe cycles per wave;
//  * output layer 512 -> 3, the RK4 state and its update are wave-local (state component d of column j lives in lane
//    16 d + j).
//
// One evaluation of the ODE function is program text shared with the adaptive solve (ode_dp5.hip) and the two solves that write a
// tape (ode_train_fwd.hip, ode_sample_tape.hip): ode_x6_setup.inc (LDS layout, constant tables, LDS-DMA, accumulators) and
// ode_x6_eval.inc (gate tables, the two layer passes, the output layer); the LDS sizes, the column exchange and the scheduling-region
// macros are in ode_x6.h.  This file adds the fixed-step RK4 loop with MovingBatchNorm at both ends, the weight pack and the entries.
//
// Measured at cfg-2 (160 frames x 2048 points, 8 RK4 steps): 51.3 ms per launch against 80.4 ms for the f32 kernel
// (DESIGN.md section 3 lists the steps from 64.8 ms and what is left: MFMA issue floor 26 ms, exposed VALU 3.6 ms,
// piece barriers ~6 ms, weight DMA 8-9.5 ms -- the 3 MB of split weights go L2 -> LDS once per 64 points and stage).
#include "ode_x6.h"

template <bool DIV>
__global__ __launch_bounds__(256, 1) void cnf_rk4_x6_kernel(CnfX6Args a)
{
    const int tid = threadIdx.x, lane0 = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g0 = lane0 >> 4;
    XC_FRAME_STEPS(a, bt, S, !DIV)
    // DIV: a wave's 16 columns are 8 points (j < 8) and their 8 tangent columns (j >= 8); the workgroup owns 32 points
    const int col = DIV ? blockIdx.x * (XC_COLS / 2) + 8 * wave + (lane0 & 7) : blockIdx.x * XC_COLS + 16 * wave + (lane0 & 15);
    const bool tg0 = DIV && (lane0 & 8);
    const bool cvalid = col < a.n;
    const int ccol = cvalid ? col : a.n - 1;
    const float *hy = a.hyper + (long)bt * a.ldh;
    constexpr int GOFF = 0, BOFF = 3 * XC_H + 3;
    const int sd = g0 < 3 ? g0 : 0;   // state component of this lane (lanes g == 3 carry a copy of component 0, never stored)

#include "ode_x6_setup.inc"

    float y, kacc = 0.f, kprev = 0.f;
    float lp = 0.f, lacc = 0.f;   // DIV: log-density state of point j, owned by lane (g = 3, j < 8)
    {
        float v = a.y_in[((long)bt * a.n + ccol) * 3 + sd];
        if (a.mbn_in) v = mbn_apply(a.mbn_in, sd, a.reverse, v);
        y = v;
        if (DIV) {
            if (tg0) y = a.e[((long)bt * a.n + ccol) * 3 + sd];     // tangent lanes carry e_d (constant over the solve) in the state register
            lp = a.logp_in ? a.logp_in[(long)bt * a.n + ccol] : 0.f;
            if (a.mbn_in) lp = mbn_shift_logp(a.mbn_in, a.reverse, lp);
        }
    }

    const double t0 = a.reverse ? (double)a.t_end : 0.0, t1 = a.reverse ? 0.0 : (double)a.t_end;
    const double h = (t1 - t0) / (double)S;
    const float hh = (float)h, h2 = (float)(0.5 * h), h6 = (float)(h / 6.0);

    // the first piece of layer 1; every layer pass leaves the NEXT pass's first piece in flight
    dma(a.w1x, 0, lane0 * 16);

    for (int step = 0; step < S; ++step) {
#pragma unroll 1
        for (int stage = 0; stage < 4; ++stage) {
            const double tc = (stage == 0) ? 0.0 : (stage == 3 ? 1.0 : 0.5);
            const float t = (float)(t0 + (double)step * h + tc * h);
            const float aw = (stage == 0) ? 0.f : (stage == 3 ? hh : h2);
#define XC_STAGE_INPUT ((stage == 0 || tg) ? y : y + aw * kprev)   // tangent lanes keep e (kprev stays 0 there)
#define XC_LAYERS_ON (!(a.diag & 2))                               // debug build: CASPR_X6_DIAG bit 1 times a stage without its layer passes
#include "ode_x6_eval.inc"
            if (!DIV || !tg) {
                kprev = od;
                kacc = (stage == 0) ? od : ((stage == 3) ? kacc + od : kacc + 2.0f * od);
            }
            if (DIV) {
                // -divergence estimate = -(e . J e) (odefunc.py:26,136): tangent lanes (g < 3) hold e_g and all of J e
                float dv = (tg && g < 3) ? ystage * od : 0.f;
                dv += __shfl_xor(dv, 16);
                dv += __shfl_xor(dv, 32);
                const float nd = -xc_partner(dv);            // lands in the point's value column (every g)
                lacc = (stage == 0) ? nd : ((stage == 3) ? lacc + nd : lacc + 2.0f * nd);
            }
        }
        if (!DIV || !tg0) y = y + h6 * kacc;
        if (DIV) lp = lp + h6 * lacc;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the prefetch left in flight by the last layer pass

    if (DIV && cvalid && g0 == 3 && !tg0) {
        if (a.mbn_out) lp = mbn_shift_logp(a.mbn_out, a.reverse, lp);
        a.logp_out[(long)bt * a.n + col] = lp;
    }
    if (cvalid && g0 < 3 && !tg0) {
        float v = y;
        if (a.mbn_out) v = mbn_apply(a.mbn_out, sd, a.reverse, v);
        a.y_out[((long)bt * a.n + col) * 3 + sd] = v;
    }
}

// (512, ldw) f32 hidden-layer weight -> [row half 2][k chunk 16][plane 3][row 0..255][piece'][8 bf16], k listed in the
// D-fragment order of the producing layer (see the header): piece g, element q <-> k = 32 kc + (q < 4 ? 4g + q : 16 + 4g + q - 4)
__global__ void pack_weight_cnf_x6_kernel(const float *__restrict__ w, int ldw, unsigned char *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // (row half * 16 + chunk) * 1024 + row * 4 + piece
    if (i >= 2 * 16 * 1024) return;
    const int piece = i & 3, row = (i >> 2) & 255;
    const int ck = i >> 10, kc = ck & 15, mt = ck >> 4;
    const int co = mt * 256 + row;
    float hs[3][8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int k = 32 * kc + (q < 4 ? 4 * piece + q : 16 + 4 * piece + q - 4);
        xc_split(w[(long)co * ldw + k], hs[0][q], hs[1][q], hs[2][q]);
    }
    const int sw = (0 - (row >> 2)) & 3;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        u32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = xc_pack(hs[pl][2 * q], hs[pl][2 * q + 1]);
        *(u32x4 *)(out + (long)ck * XC_PIECE + pl * XC_PA + row * 64 + ((piece ^ sw) << 4)) = v;
    }
}

#ifdef CASPR_DEBUG_HOOKS
static unsigned long long *g_x6_trace = nullptr;
extern "C" void caspr_debug_set_x6_trace(unsigned long long *dev_buf) { g_x6_trace = dev_buf; }   // debug build only: >= 512 u64
#endif
// one buffer per hidden layer holds BOTH images: [0, XC_PACK) the 48 KB-piece layout of cnf_rk4_x6_kernel (divergence
// variant), [XC_PACK, XC_PACK + XW_PACK) the 24 KB-piece fragment-order layout of cnf_rk4_x6w_kernel (sampling)
#define XC_PACK (2L * 16 * XC_PIECE)
extern "C" long caspr_cnf_x6_packed_bytes(void) { return XC_PACK + XW_PACK; }

extern "C" int caspr_pack_weight_cnf_x6(const float *w, int ldw, void *packed, void *stream)
{
    CASPR_REQUIRE(w && packed && ldw >= XC_H, "pack_weight_cnf_x6: bad arguments");
    CASPR_REQUIRE(((uintptr_t)packed % 16) == 0, "pack_weight_cnf_x6: packed must be 16-byte aligned");
    pack_weight_cnf_x6_kernel<<<2 * 16 * 1024 / 256, 256, 0, (hipStream_t)stream>>>(w, ldw, (unsigned char *)packed);
    caspr_cnf_x6w_pack(w, ldw, (unsigned char *)packed + XC_PACK, (hipStream_t)stream);
    CASPR_CHECK_LAUNCH("pack_weight_cnf_x6");
    return CASPR_OK;
}

// steps_tab / max_steps / order: the per-frame table of caspr_cnf_rk4_x6_frames_f32 (sampling only), NULL / 0 / NULL from the plain entry
static int cnf_rk4_x6_run(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0,
                          const float *b0, const void *w1x, const float *b1, const void *w2x, const float *b2,
                          const float *w3, const float *b3, int H, float t_end, int steps, int reverse,
                          const float *mbn_in, const float *mbn_out, const float *e, const float *logp_in,
                          float *logp_out, float *y_out, int BT, int n, const int *steps_tab, int max_steps, const int *order, void *stream)
{
    CASPR_REQUIRE(y_in && hyper && tcol && w0 && b0 && w1x && b1 && w2x && b2 && w3 && b3 && y_out, "cnf_rk4_x6: null pointer");
    CASPR_REQUIRE(H == XC_H, "cnf_rk4_x6: hidden width %d unsupported (kernel is built for 512-512-512, flow.py:89)", H);
    CASPR_REQUIRE(BT > 0 && BT <= 65535 && n > 0 && steps > 0 && ldh >= 2 * (3 * H + 3), "cnf_rk4_x6: bad sizes");
    CASPR_REQUIRE((e == nullptr) == (logp_out == nullptr), "cnf_rk4_x6: e and logp_out must be given together");
    CASPR_REQUIRE(((uintptr_t)w1x % 16) == 0 && ((uintptr_t)w2x % 16) == 0 && ((uintptr_t)w0 % 16) == 0 && ((uintptr_t)w3 % 16) == 0,
                  "cnf_rk4_x6: weights must be 16-byte aligned");
    CnfX6Args a;
    a.y_in = y_in; a.hyper = hyper; a.tcol = tcol; a.w0 = w0; a.b0 = b0; a.b1 = b1; a.b2 = b2; a.w3 = w3; a.b3 = b3;
    a.mbn_in = mbn_in; a.mbn_out = mbn_out; a.w1x = (const unsigned char *)w1x; a.w2x = (const unsigned char *)w2x;
    a.e = e; a.logp_in = logp_in; a.logp_out = logp_out;
    a.trace = nullptr;
    CASPR_IF_DEBUG(a.trace = g_x6_trace;)
    a.diag = CASPR_DEBUG_ENV_INT("CASPR_X6_DIAG");   // timing experiments, debug build only
    const bool narrow = (reverse & CASPR_CNF_NARROW) != 0;      // the caller asks for the 64-point sampling kernel (include/caspr_hip.h)
    reverse &= 1;
    a.y_out = y_out; a.ldh = ldh; a.n = n; a.steps = steps; a.reverse = reverse; a.t_end = t_end;
    a.steps_tab = steps_tab; a.max_steps = max_steps; a.order = order;
    // Kernel choice by the presence of e only, never by BT or n: a frame's result does not depend on the batch around it.
    // Sampling (no divergence): the 128-point kernel of ode_bf16x6w.hip; the debug build can force the 64-point one
    // (CASPR_X6_NARROW=1) for A/B timing (tools/cnf_x6w_trace.py).
    if (!e && !narrow && CASPR_DEBUG_ENV_INT("CASPR_X6_NARROW") == 0) {
        a.w1x += XC_PACK;
        a.w2x += XC_PACK;
        const int rc = caspr_cnf_x6w_launch(a, BT, (hipStream_t)stream);
        if (rc != CASPR_OK) return rc;
        CASPR_CHECK_LAUNCH("cnf_rk4_x6 (128-point kernel)");
        return CASPR_OK;
    }
    static CasprLdsOptIn optin_s, optin_d;
    const hipError_t err = e ? caspr_lds_opt_in(optin_d, (const void *)cnf_rk4_x6_kernel<true>, XC_LDS)
                             : caspr_lds_opt_in(optin_s, (const void *)cnf_rk4_x6_kernel<false>, XC_LDS);
    if (err != hipSuccess) {
        caspr_set_error("cnf_rk4_x6: hipFuncSetAttribute failed: %s", hipGetErrorString(err));
        return CASPR_ELAUNCH;
    }
    if (e) cnf_rk4_x6_kernel<true><<<dim3(ceil_div(n, XC_COLS / 2), BT), dim3(256), XC_LDS, (hipStream_t)stream>>>(a);
    else cnf_rk4_x6_kernel<false><<<dim3(ceil_div(n, XC_COLS), BT), dim3(256), XC_LDS, (hipStream_t)stream>>>(a);
    CASPR_CHECK_LAUNCH("cnf_rk4_x6");
    return CASPR_OK;
}

extern "C" int caspr_cnf_rk4_x6_f32(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0,
                                    const float *b0, const void *w1x, const float *b1, const void *w2x, const float *b2,
                                    const float *w3, const float *b3, int H, float t_end, int steps, int reverse,
                                    const float *mbn_in, const float *mbn_out, const float *e, const float *logp_in,
                                    float *logp_out, float *y_out, int BT, int n, void *stream)
{
    return cnf_rk4_x6_run(y_in, hyper, ldh, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, H, t_end, steps, reverse, mbn_in, mbn_out, e, logp_in,
                          logp_out, y_out, BT, n, nullptr, 0, nullptr, stream);
}

// the sampling solve with a step count per frame (cnf.py:70-128 with logpx = None; flow.py:96-99)
extern "C" int caspr_cnf_rk4_x6_frames_f32(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0,
                                           const float *b0, const void *w1x, const float *b1, const void *w2x, const float *b2,
                                           const float *w3, const float *b3, int H, float t_end, int reverse,
                                           const float *mbn_in, const float *mbn_out, float *y_out, int BT, int n,
                                           const int *steps_tab, int max_steps, const int *order, void *stream)
{
    CASPR_REQUIRE(steps_tab, "cnf_rk4_x6_frames: null step table");
    CASPR_REQUIRE(max_steps >= 1 && max_steps <= 4096, "cnf_rk4_x6_frames: max_steps %d outside 1..4096", max_steps);
    return cnf_rk4_x6_run(y_in, hyper, ldh, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, H, t_end, max_steps, reverse, mbn_in, mbn_out, nullptr,
                          nullptr, nullptr, y_out, BT, n, steps_tab, max_steps, order, stream);
}
