// ode_train_fwd.hip -- the TRAINING forward of one point-CNF block as one launch (train/flow_grad.py: CnfBlockSolve): fixed-step RK4 in
// the forward direction with the Hutchinson divergence and a given e, and no layer product ever leaves the chip.
//
// The ODE function evaluation is the one of ode_bf16x6.hip (divergence variant), shared with it as text (ode_x6_setup.inc,
// ode_x6_eval.inc with DIV = true): a wave owns 8 points + their 8 tangent columns and all 512 hidden units, both hidden layers on
// the bf16 matrix pipe in the exact three-way split with f32 accumulation, weight pieces by LDS-DMA.  This file adds the RK4 loop
// around it and what is written:
//  * besides (x_T, logp_T) every evaluation's point state goes to memory: the stage input (S, 4, BT, n, 3) that the reverse sweep
//    rebuilds ONE evaluation's tape from, and the stage outputs a = dy/dt (S, 4, BT, n, 3), nd = -e^T J e (S, 4, BT, n) that the
//    gradient with respect to the step size needs.  12 + 12 + 4 bytes per point and evaluation: the only thing that grows with S;
//  * REG = true (caspr_cnf_block_reg_fwd_f32; train/flow_grad.py: CnfBlockSolveReg) also integrates the two regularisers of Finlay et
//    al. 2020, r' = (|a|^2, |J e|^2), r(0) = 0, by the same RK4 weights as the log-density, and writes every evaluation's integrands
//    kq (S, 4, BT, n, 2) and r_T (BT, n, 2): the value lanes hold a, the tangent lanes J e, so both squares are two cross-lane sums away.
//    Everything REG = false computes is left alone: x_T, logp_T, ys, ka, knd of the REG launch are the plain launch's bits;
//  * the end time is read from device memory (the training step holds sqrt_end_time^2 as a tensor: no host read-back);
//  * no MovingBatchNorm at either end (autograd keeps those), forward direction only.
// Every store is a plain vector store by the lane that owns the value; no atomics; a point's result depends on its frame's
// gates and its own column only, never on the batch around it.
#include "ode_x6.h"

struct CnfTrainFwdArgs {
    const float *y_in, *hyper, *tcol, *w0, *b0, *b1, *b2, *w3, *b3;
    const float *e, *logp_in;     // Hutchinson noise (BT,n,3), initial log-density (BT,n)
    const float *t_end;           // one float in device memory
    const unsigned char *w1x, *w2x;
    float *y_out, *logp_out;      // (BT,n,3), (BT,n)
    float *ys, *ka, *knd;         // [steps][4][BT][n][3], [steps][4][BT][n][3], [steps][4][BT][n]
    int ldh, n, steps;
};
// the plain kernel's argument block is the one above, byte for byte; REG = true appends its two outputs
template <bool REG> struct CnfTrainFwdArgsOf : CnfTrainFwdArgs {};
template <> struct CnfTrainFwdArgsOf<true> : CnfTrainFwdArgs {
    float *kq, *r_out;            // [steps][4][BT][n][2] = (|a|^2, |J e|^2), (BT,n,2)
};

template <bool REG>
__global__ __launch_bounds__(256, 1) void cnf_train_fwd_kernel(CnfTrainFwdArgsOf<REG> a)
{
    constexpr bool DIV = true;
    const int tid = threadIdx.x, lane0 = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g0 = lane0 >> 4;
    const int bt = blockIdx.y;
    // a wave's 16 columns are 8 points (j < 8) and their 8 tangent columns (j >= 8); the workgroup owns 32 points
    const int col = blockIdx.x * (XC_COLS / 2) + 8 * wave + (lane0 & 7);
    const bool tg0 = lane0 & 8;
    const bool cvalid = col < a.n;
    const int ccol = cvalid ? col : a.n - 1;
    const float *hy = a.hyper + (long)bt * a.ldh;
    constexpr int GOFF = 0, BOFF = 3 * XC_H + 3;
    const int sd = g0 < 3 ? g0 : 0;   // state component of this lane (lanes g == 3 carry a copy of component 0, never stored)

#include "ode_x6_setup.inc"

    float y, kacc = 0.f, kprev = 0.f;
    float lp = 0.f, lacc = 0.f;   // log-density state of point j, owned by lane (g = 3, j < 8)
    float r[2] = {0.f, 0.f}, racc[2] = {0.f, 0.f};   // REG: the regularisers' integrals of point j, r(0) = 0, owned as lp is
    y = tg0 ? a.e[((long)bt * a.n + ccol) * 3 + sd] : a.y_in[((long)bt * a.n + ccol) * 3 + sd];   // tangent lanes carry e_d (constant over the solve)
    lp = a.logp_in[(long)bt * a.n + ccol];

    const double t0 = 0.0;
    const double h = (double)a.t_end[0] / (double)a.steps;
    const float hh = (float)h, h2 = (float)(0.5 * h), h6 = (float)(h / 6.0);

    // the first piece of layer 1; every layer pass leaves the NEXT pass's first piece in flight
    dma(a.w1x, 0, lane0 * 16);

    for (int step = 0; step < a.steps; ++step) {
#pragma unroll 1
        for (int stage = 0; stage < 4; ++stage) {
            const double tc = (stage == 0) ? 0.0 : (stage == 3 ? 1.0 : 0.5);
            const float t = (float)(t0 + (double)step * h + tc * h);
            const float aw = (stage == 0) ? 0.f : (stage == 3 ? hh : h2);
#define XC_STAGE_INPUT ((stage == 0 || tg) ? y : y + aw * kprev)   // tangent lanes keep e (kprev stays 0 there)
#define XC_LAYERS_ON true
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
                float qa = 0.f, qj = 0.f;
                if constexpr (REG) {
                    // |a|^2 on the value lanes, |J e|^2 on the tangent lanes: lanes g == 3 carry a copy of component 0 and stay out
                    float qv = (g < 3) ? od * od : 0.f;
                    qv += __shfl_xor(qv, 16);
                    qv += __shfl_xor(qv, 32);
                    qa = qv;
                    qj = xc_partner(qv);                     // the tangent column's sum, in the point's value column (as nd)
                    racc[0] = (stage == 0) ? qa : ((stage == 3) ? racc[0] + qa : racc[0] + 2.0f * qa);
                    racc[1] = (stage == 0) ? qj : ((stage == 3) ? racc[1] + qj : racc[1] + 2.0f * qj);
                }
                // ---- what the reverse sweep needs of this evaluation: its input and its outputs, by the lanes that own them
                const int colx = blockIdx.x * (XC_COLS / 2) + 8 * wave + (j & 7);
                if (!tg && colx < a.n) {
                    const long ev = ((long)(step * 4 + stage) * gridDim.y + bt) * a.n + colx;
                    if (g < 3) {
                        a.ys[ev * 3 + g] = ystage;
                        a.ka[ev * 3 + g] = od;
                    } else {
                        a.knd[ev] = nd;
                        if constexpr (REG) {
                            a.kq[ev * 2] = qa;
                            a.kq[ev * 2 + 1] = qj;
                        }
                    }
                }
            }
        }
        if (!DIV || !tg0) y = y + h6 * kacc;
        if (DIV) lp = lp + h6 * lacc;
        if constexpr (REG) {
            r[0] = r[0] + h6 * racc[0];
            r[1] = r[1] + h6 * racc[1];
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the prefetch left in flight by the last layer pass

    if (cvalid && g0 == 3 && !tg0) a.logp_out[(long)bt * a.n + col] = lp;
    if (cvalid && g0 < 3 && !tg0) a.y_out[((long)bt * a.n + col) * 3 + sd] = y;
    if constexpr (REG) {
        if (cvalid && g0 == 3 && !tg0) {
            a.r_out[((long)bt * a.n + col) * 2] = r[0];
            a.r_out[((long)bt * a.n + col) * 2 + 1] = r[1];
        }
    }
}

// the two entries' common body: `who` names the entry in its messages, REG chooses the instantiation (kq / r_out: REG only)
template <bool REG>
static int cnf_train_fwd_launch(const char *who, const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0, const float *b0,
                                const void *w1x, const float *b1, const void *w2x, const float *b2, const float *w3, const float *b3, int H,
                                const float *t_end, int steps, const float *e, const float *logp_in, float *logp_out, float *y_out, float *r_out,
                                float *ys, float *ka, float *knd, float *kq, int BT, int n, void *stream)
{
    CASPR_REQUIRE(y_in && hyper && tcol && w0 && b0 && w1x && b1 && w2x && b2 && w3 && b3 && t_end && e && logp_in && logp_out && y_out && ys && ka && knd &&
                  (!REG || (r_out && kq)), "%s: null pointer", who);
    CASPR_REQUIRE(H == XC_H, "%s: hidden width %d unsupported (kernel is built for 512-512-512, flow.py:89)", who, H);
    CASPR_REQUIRE(BT > 0 && BT <= 65535 && n > 0 && steps > 0 && ldh >= 2 * (3 * H + 3), "%s: bad sizes", who);
    CASPR_REQUIRE(((uintptr_t)w1x % 16) == 0 && ((uintptr_t)w2x % 16) == 0 && ((uintptr_t)w0 % 16) == 0 && ((uintptr_t)w3 % 16) == 0,
                  "%s: weights must be 16-byte aligned", who);
    CnfTrainFwdArgsOf<REG> a;
    a.y_in = y_in; a.hyper = hyper; a.tcol = tcol; a.w0 = w0; a.b0 = b0; a.b1 = b1; a.b2 = b2; a.w3 = w3; a.b3 = b3;
    a.e = e; a.logp_in = logp_in; a.t_end = t_end; a.w1x = (const unsigned char *)w1x; a.w2x = (const unsigned char *)w2x;
    a.y_out = y_out; a.logp_out = logp_out; a.ys = ys; a.ka = ka; a.knd = knd;
    a.ldh = ldh; a.n = n; a.steps = steps;
    if constexpr (REG) { a.kq = kq; a.r_out = r_out; }
    static CasprLdsOptIn optin;                        // one per instantiation
    const hipError_t err = caspr_lds_opt_in(optin, (const void *)cnf_train_fwd_kernel<REG>, XC_LDS);
    if (err != hipSuccess) {
        caspr_set_error("%s: hipFuncSetAttribute failed: %s", who, hipGetErrorString(err));
        return CASPR_ELAUNCH;
    }
    cnf_train_fwd_kernel<REG><<<dim3(ceil_div(n, XC_COLS / 2), BT), dim3(256), XC_LDS, (hipStream_t)stream>>>(a);
    CASPR_CHECK_LAUNCH(who);
    return CASPR_OK;
}

extern "C" int caspr_cnf_train_fwd_f32(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0, const float *b0,
                                       const void *w1x, const float *b1, const void *w2x, const float *b2, const float *w3, const float *b3,
                                       int H, const float *t_end, int steps, const float *e, const float *logp_in, float *logp_out,
                                       float *y_out, float *ys, float *ka, float *knd, int BT, int n, void *stream)
{
    return cnf_train_fwd_launch<false>("cnf_train_fwd", y_in, hyper, ldh, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, H, t_end, steps, e, logp_in, logp_out,
                                       y_out, nullptr, ys, ka, knd, nullptr, BT, n, stream);
}

extern "C" int caspr_cnf_block_reg_fwd_f32(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0, const float *b0,
                                           const void *w1x, const float *b1, const void *w2x, const float *b2, const float *w3, const float *b3,
                                           int H, const float *t_end, int steps, const float *e, const float *logp_in, float *logp_out,
                                           float *y_out, float *r_out, float *ys, float *ka, float *knd, float *kq, int BT, int n, void *stream)
{
    return cnf_train_fwd_launch<true>("cnf_block_reg_fwd", y_in, hyper, ldh, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, H, t_end, steps, e, logp_in, logp_out,
                                      y_out, r_out, ys, ka, knd, kq, BT, n, stream);
}
