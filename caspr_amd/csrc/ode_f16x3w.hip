// ode_f16x3w.hip -- the point-CNF SAMPLING solve on THREE f16 products per f32 product (config.cnf_split = "f16x3"): the geometry of
// ode_bf16x6w.hip (128 points per workgroup, a wave owns 32 points and all 512 units, layer 1's 256 accumulators in the hand-managed
// accumulator file, layer 2 in four passes, weights through an LDS ring by LDS-DMA, MovingBatchNorm prologue / epilogue, layers 0 and
// 3 in f32) with half the matrix-pipe instructions.  The body is a copy of that kernel's on purpose (as ode_dp5.hip's and
// ode_train_fwd.hip's are of the 64-point kernel); read its header first, this one lists the differences.
//
//  * the scheme: an f32 operand x 2^k is split into two f16 planes by round-to-nearest (p1 = rne16(x), p2 = rne16(x - p1): 22
//    significant bits), and  a . b ~ a2 b1 + a1 b2 + a1 b1  on v_mfma_f32_32x32x16_f16, smallest terms first.  The dropped a2 b2 is
//    about 2^-24 |a| |b|.  tests/f16x3_ref.py is the contract, tests/test_f16x3_emulation.py its error against f64;
//  * the exponent range: hidden activations come out of a softplus and are scaled by 2^4 (|x| < 4094 stays finite in f16; anything
//    above 2^-7 keeps both planes normal), a layer's weights by the power of two that puts max |W| in [2^14, 2^15) -- computed ON THE
//    DEVICE at pack time (max-reduction, no host round trip) and stored behind the pack, where this kernel reads it.  Both scales are
//    exact; they are undone in the stage's gate tables (g1 2^-s1 with the next layer's 2^4 folded in, g2 2^-(4 + s2)), at no cost;
//  * the kernel carries the SCALED activation X = 16 softplus(x): the 2^4 sits in the tables of the producing layer, and
//    softplus works on X directly (exp2 of |X| log2 e / 16, 16 ln 2 outside): the same roundings as on x, no extra instruction;
//  * the accumulator file in layer 2 holds the two f16 PLANES of hidden layer 1's activations, not X: pass 0 splits a group of four
//    values once and writes its four plane words over the four sums; passes 1-3 read them back as B operands and do no arithmetic
//    (the bf16x6 kernel has to keep X: three bf16 planes are 48 bits a value);
//  * plane values below 2^-14 (f16 subnormals) are flushed to zero explicitly, so nothing depends on the pipe's subnormal handling;
//  * range guard: a lane tracks the maximum of the X it splits; a point whose maximum is not below 65520 (not finite in f16) gets NaN
//    in all three outputs and the launch's status word is set (ops.check_deferred_errors reports it and names cnf_split="bf16x6");
//  * weights: 16 KB pieces [k-step 2][row tile 4][plane 2][1 KB fragment], 24 MFMAs (768 matrix-pipe cycles) each, through an
//    EIGHT-deep ring: a piece lasts half as long as the bf16x6 kernel's, so the same flight time needs twice the pieces in flight.
//    Piece s + 7 is issued (4 LDS-DMA instructions per wave) while piece s is multiplied, into the slot piece s - 1 left at the
//    barrier in its last region; that barrier waits with vmcnt(24): the six younger pieces may still be in flight;
//  * a region is one k-step x two row tiles = 6 MFMAs, one scheduling slot each; slots 0-3 read the next region's four fragments; the
//    producers run two micro-steps per slot in pass 0 of layer 2 (the same work per k-step under half the MFMAs).
//
// One evaluation of the ODE function is program text shared with the adaptive solve (ode_dp5_f16x3w.hip): ode_h3w.h (layout, softplus
// and split micro-steps), ode_h3w_setup.inc (LDS layout, constant tables), ode_h3w_ring.inc (LDS-DMA, the first pieces, the registers)
// and ode_h3w_eval.inc (gate tables, input layer, the two hidden layers up to the output layer's partial sums).  This file adds the
// switches of the text, the fixed-step RK4 loop with MovingBatchNorm at both ends, the range-guard epilogue, the weight pack and the entries.

// XW_EXP (debug flavours only, build.py CASPR_XW_EXP): 16 = no phase stamps; 65536 / 131072 = the instruction stream of the parent for
// ONE item of "the wave's instruction stream" (DESIGN.md 3): the f32 compare-and-select flush, an address and an M0 write per LDS-DMA
// instruction.  Same output bits with either set.  1048576 / 2097152 = NO flush of plane 1 / plane 2 (WRONG results where a plane
// value is an f16 subnormal: what tests/test_cnf_f16x3_flush_band.py must notice).
#ifndef XW_EXP
#define XW_EXP 0
#endif
#define XH_OLD_FLUSH ((XW_EXP & 65536) != 0)
#define XH_OLD_DMA ((XW_EXP & 131072) != 0)
#define XH_NO_FLUSH1 ((XW_EXP & 1048576) != 0)
#define XH_NO_FLUSH2 ((XW_EXP & 2097152) != 0)
// debug build (tools/cnf_h3w_trace.py): s_memtime stamps of workgroup (0,0), thread 0, RK4 step 0, sixteen slots per stage: 0 stage head,
// 1 tables built, 2 chunk 0 of the input layer done, 3 layer 1 done, 4 + 2 q the K loop of pass q done, 5 + 2 q its epilogue, 12 stage end.
// The stamped kernel does NOT fit its registers (115 VGPRs spilled with the tested compiler, as the bf16x6 kernel's stamped flavour spills
// 134): its scratch traffic shares vmcnt with the weight ring, so the split is indicative and a stamped stage is far slower than a real one
#if defined(CASPR_DEBUG_HOOKS) && !(XW_EXP & 16)
#define XH_STAMP(i) if (a.trace && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0 && step == 0) a.trace[16 * stage + (i)] = __builtin_amdgcn_s_memtime();
#else
#define XH_STAMP(i)
#endif
#include "ode_h3w.h"

struct CnfH3Args : CnfX6Args {
    unsigned *status;                     // one word per launch, zeroed in front of it: != 0 <-> the range guard tripped
};

__global__ __launch_bounds__(256, 1) void cnf_rk4_h3w_kernel(CnfH3Args a)
{
    const int tid = threadIdx.x, lane0 = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    XC_FRAME_STEPS(a, bt, S, true)
#include "ode_h3w_setup.inc"

    const int col = blockIdx.x * XH_PTS + 32 * wave + (lane0 & 31);
    const bool cvalid = col < a.n;
    const int ccol = cvalid ? col : a.n - 1;
    float y[3], kacc[3] = {0.f, 0.f, 0.f}, kprev[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        float v = a.y_in[((long)bt * a.n + ccol) * 3 + d];
        if (a.mbn_in) v = mbn_apply(a.mbn_in, d, a.reverse, v);
        y[d] = v;
    }

    // (the table registers: the same text in cnf_dp5_h3w_kernel, see ode_h3w_setup.inc)
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

    const double t0 = a.reverse ? (double)a.t_end : 0.0, t1 = a.reverse ? 0.0 : (double)a.t_end;
    const double h = (t1 - t0) / (double)S;
    const float hh = (float)h, h2 = (float)(0.5 * h), h6 = (float)(h / 6.0);

#include "ode_h3w_ring.inc"

    for (int step = 0; step < S; ++step) {
#pragma unroll 1
        for (int stage = 0; stage < 4; ++stage) {
            const double tc = (stage == 0) ? 0.0 : (stage == 3 ? 1.0 : 0.5);
            const float t = (float)(t0 + (double)step * h + tc * h);
            const float aw = (stage == 0) ? 0.f : (stage == 3 ? hh : h2);
#define XH_STAGE_INPUT                                                                                        \
    float ys[3];                                                                                              \
    _Pragma("unroll") for (int d = 0; d < 3; ++d) ys[d] = (stage == 0) ? y[d] : y[d] + aw * kprev[d];
#include "ode_h3w_eval.inc"

            // ---- output ConcatSquash (no softplus: odefunc.py:103): the two halves of a column hold disjoint rows
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                float v = part[d];
                v += __shfl_xor(v, 32);
                const float od = fmaf(v, s_g3[d], s_g3[4 + d]);
                kprev[d] = od;
                kacc[d] = (stage == 0) ? od : ((stage == 3) ? kacc[d] + od : kacc[d] + 2.0f * od);
            }
            XH_STAMP(12)
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) y[d] = y[d] + h6 * kacc[d];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the pieces left in flight by the last stage

    // range guard: the two halves of a column split disjoint units of the same point
    xmax = fmaxf(xmax, __shfl_xor(xmax, 32));
    const bool bad = !(xmax < XH_F16_LIMIT);
    if (cvalid && lane0 < 32) {
        if (bad) atomicOr(a.status, 1u);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            float v = y[d];
            if (a.mbn_out) v = mbn_apply(a.mbn_out, d, a.reverse, v);
            a.y_out[((long)bt * a.n + col) * 3 + d] = bad ? __uint_as_float(0x7fc00000u) : v;
        }
    }
}

// ---- pack: (512, ldw) f32 -> [row quarter 4][k chunk 16][k-step 2][row tile 4][plane 2][lane 64][8 f16] + tail ----------------------
// lane (i = l & 31, h = l >> 5) of fragment (rq, kc, ks, rt) holds row 128 rq + 32 rt + i, k slots s = 0..7 <-> k = 32 kc + 16 ks +
// (s & 3) + 8 (s >> 2) + 4 h (the D-fragment order of the producing layer, as the bf16x6 wide pack)
__global__ void h3_weight_max_kernel(const float *__restrict__ w, int ldw, unsigned *__restrict__ tail)
{
    unsigned m = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < XC_H * XC_H; i += gridDim.x * blockDim.x)
        m = max(m, __float_as_uint(w[(long)(i >> 9) * ldw + (i & 511)]) & 0x7fffffffu);      // |w|: non-negative floats order as their bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0) atomicMax(tail + 1, m);
}
// (h3_shift: f16x3_common.h)
__global__ void pack_weight_cnf_h3_kernel(const float *__restrict__ w, int ldw, unsigned char *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // ((rq * 16 + kc) * 8 + ks * 4 + rt) * 64 + lane
    if (i >= 4 * 16 * 8 * 64) return;
    unsigned *tail = (unsigned *)(out + XH_PACK);
    const int sh = h3_shift(tail[1]);
    if (i == 0) ((int *)tail)[0] = sh;
    const int l = i & 63, fr = (i >> 6) & 7, ck = i >> 9;
    const int rt = fr & 3, ks = fr >> 2, kc = ck & 15, rq = ck >> 4;
    const int row = 128 * rq + 32 * rt + (l & 31), hh = l >> 5;
    float p1[8], p2[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int k = 32 * kc + 16 * ks + (s & 3) + 8 * (s >> 2) + 4 * hh;
        float x = ldexpf(w[(long)row * ldw + k], sh);
        if (fabsf(x) < XH_FLUSH) x = 0.0f;
        p1[s] = (float)(_Float16)x;
        float r = x - p1[s];
        if (fabsf(r) < XH_FLUSH) r = 0.0f;
        p2[s] = r;
    }
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        u32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = pl ? xh_cvt_pk(p2[2 * q], p2[2 * q + 1]) : xh_cvt_pk(p1[2 * q], p1[2 * q + 1]);
        *(u32x4 *)(out + (long)ck * XH_PIECE + ((long)(fr * 2 + pl) * 64 + l) * 16) = v;
    }
}

extern "C" long caspr_cnf_h3_packed_bytes(void) { return XH_PACK + XH_TAIL; }

extern "C" int caspr_pack_weight_cnf_h3(const float *w, int ldw, void *packed, void *stream)
{
    CASPR_REQUIRE(w && packed && ldw >= XC_H, "pack_weight_cnf_h3: bad arguments");
    CASPR_REQUIRE(((uintptr_t)packed % 16) == 0, "pack_weight_cnf_h3: packed must be 16-byte aligned");
    unsigned char *out = (unsigned char *)packed;
    const hipError_t err = hipMemsetAsync(out + XH_PACK, 0, XH_TAIL, (hipStream_t)stream);
    if (err != hipSuccess) {
        caspr_set_error("pack_weight_cnf_h3: hipMemsetAsync failed: %s", hipGetErrorString(err));
        return CASPR_ELAUNCH;
    }
    h3_weight_max_kernel<<<64, 256, 0, (hipStream_t)stream>>>(w, ldw, (unsigned *)(out + XH_PACK));
    pack_weight_cnf_h3_kernel<<<4 * 16 * 8 * 64 / 256, 256, 0, (hipStream_t)stream>>>(w, ldw, out);
    CASPR_CHECK_LAUNCH("pack_weight_cnf_h3");
    return CASPR_OK;
}

#ifdef CASPR_DEBUG_HOOKS
static unsigned long long *g_h3_trace = nullptr;
// 64 words; see XH_STAMP
extern "C" void caspr_debug_set_h3_trace(unsigned long long *dev_buf) { g_h3_trace = dev_buf; }
#endif

// steps_tab / max_steps / order: the per-frame table of caspr_cnf_rk4_h3_frames_f32, NULL / 0 / NULL from the plain entry
static int cnf_rk4_h3_run(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0,
                          const float *b0, const void *w1h, const float *b1, const void *w2h, const float *b2,
                          const float *w3, const float *b3, int H, float t_end, int steps, int reverse,
                          const float *mbn_in, const float *mbn_out, unsigned *status, float *y_out, int BT, int n,
                          const int *steps_tab, int max_steps, const int *order, void *stream)
{
    CASPR_REQUIRE(y_in && hyper && tcol && w0 && b0 && w1h && b1 && w2h && b2 && w3 && b3 && y_out && status, "cnf_rk4_h3: null pointer");
    CASPR_REQUIRE(H == XC_H, "cnf_rk4_h3: hidden width %d unsupported (kernel is built for 512-512-512, flow.py:89)", H);
    CASPR_REQUIRE(BT > 0 && BT <= 65535 && n > 0 && steps > 0 && ldh >= 2 * (3 * H + 3), "cnf_rk4_h3: bad sizes");
    CASPR_REQUIRE(((uintptr_t)w1h % 16) == 0 && ((uintptr_t)w2h % 16) == 0 && ((uintptr_t)w0 % 16) == 0 && ((uintptr_t)w3 % 16) == 0,
                  "cnf_rk4_h3: weights must be 16-byte aligned");
    CnfH3Args a;
    a.y_in = y_in; a.hyper = hyper; a.tcol = tcol; a.w0 = w0; a.b0 = b0; a.b1 = b1; a.b2 = b2; a.w3 = w3; a.b3 = b3;
    a.mbn_in = mbn_in; a.mbn_out = mbn_out; a.w1x = (const unsigned char *)w1h; a.w2x = (const unsigned char *)w2h;
    a.e = nullptr; a.logp_in = nullptr; a.logp_out = nullptr; a.trace = nullptr; a.diag = 0;
    CASPR_IF_DEBUG(a.trace = g_h3_trace;)
    a.y_out = y_out; a.ldh = ldh; a.n = n; a.steps = steps; a.reverse = reverse & 1; a.t_end = t_end;
    a.status = status;
    a.steps_tab = steps_tab; a.max_steps = max_steps; a.order = order;
    static CasprLdsOptIn optin;
    hipError_t err = caspr_lds_opt_in(optin, (const void *)cnf_rk4_h3w_kernel, XH_LDS);
    if (err != hipSuccess) {
        caspr_set_error("cnf_rk4_h3: hipFuncSetAttribute failed: %s", hipGetErrorString(err));
        return CASPR_ELAUNCH;
    }
    err = hipMemsetAsync(status, 0, sizeof(unsigned), (hipStream_t)stream);
    if (err != hipSuccess) {
        caspr_set_error("cnf_rk4_h3: hipMemsetAsync failed: %s", hipGetErrorString(err));
        return CASPR_ELAUNCH;
    }
    cnf_rk4_h3w_kernel<<<dim3(ceil_div(n, XH_PTS), BT), dim3(256), XH_LDS, (hipStream_t)stream>>>(a);
    CASPR_CHECK_LAUNCH("cnf_rk4_h3");
    return CASPR_OK;
}

extern "C" int caspr_cnf_rk4_h3_f32(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0,
                                    const float *b0, const void *w1h, const float *b1, const void *w2h, const float *b2,
                                    const float *w3, const float *b3, int H, float t_end, int steps, int reverse,
                                    const float *mbn_in, const float *mbn_out, unsigned *status, float *y_out, int BT, int n, void *stream)
{
    return cnf_rk4_h3_run(y_in, hyper, ldh, tcol, w0, b0, w1h, b1, w2h, b2, w3, b3, H, t_end, steps, reverse, mbn_in, mbn_out, status, y_out,
                          BT, n, nullptr, 0, nullptr, stream);
}

// the f16x3 sampling solve with a step count per frame (cnf.py:70-128 with logpx = None; flow.py:96-99)
extern "C" int caspr_cnf_rk4_h3_frames_f32(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0,
                                           const float *b0, const void *w1h, const float *b1, const void *w2h, const float *b2,
                                           const float *w3, const float *b3, int H, float t_end, int reverse,
                                           const float *mbn_in, const float *mbn_out, unsigned *status, float *y_out, int BT, int n,
                                           const int *steps_tab, int max_steps, const int *order, void *stream)
{
    CASPR_REQUIRE(steps_tab, "cnf_rk4_h3_frames: null step table");
    CASPR_REQUIRE(max_steps >= 1 && max_steps <= 4096, "cnf_rk4_h3_frames: max_steps %d outside 1..4096", max_steps);
    return cnf_rk4_h3_run(y_in, hyper, ldh, tcol, w0, b0, w1h, b1, w2h, b2, w3, b3, H, t_end, max_steps, reverse, mbn_in, mbn_out, status,
                          y_out, BT, n, steps_tab, max_steps, order, stream);
}
