// ode_sample_tape_h3w.hip -- the SAMPLING solve of one point-CNF block WITH THE TAPE its gradient needs (ode_sample_tape.hip's
// interface and tape; config.cnf_tape_split = "f16x3"), on the 128-point f16x3 evaluation that decode() runs at inference
// (ode_f16x3w.hip): the third driver around that evaluation, after the fixed-step RK4 solve and the adaptive Dormand-Prince solve
// (ode_dp5_f16x3w.hip).  The evaluation is shared with them as text (ode_h3w.h, ode_h3w_setup.inc, ode_h3w_ring.inc,
// ode_h3w_eval.inc); read ode_f16x3w.hip's and ode_sample_tape.hip's headers first, this one lists what is particular to the combination.
//
//  * the loop is cnf_rk4_h3w_kernel's with reverse = 1 and no MovingBatchNorm at either end (autograd keeps those in torch): t0, h, hh,
//    h2, h6 and every stage time are formed in the same types and the same order, the stage input and the stage output by the same
//    expressions, so x(0) of a block is BIT FOR BIT what ops.cnf_rk4(..., w1h=, w2h=, reverse=True) returns for the same inputs, the
//    same float32 end time and the same step count.  The instruction stream is that kernel's as well (the flush on the f16 word, one
//    M0 write per piece): audit.audit_cnf_sample_tape_h3w asks of this object what audit_cnf_h3w asks of ode_f16x3w.o;
//  * the end time is read from device memory (one float), as in ode_sample_tape.hip;
//  * the tape has ode_sample_tape.hip's layout and meaning: ys[step][stage][position][point][3] is the stage input of every evaluation,
//    ka[step][stage][position][point][3] its output dy/dt, position = blockIdx.y.  Lanes l and l + 32 of a wave hold disjoint hidden
//    units of the SAME point and both carry its three components (the stage input from the start, the stage output after the
//    cross-half add): the lower half stores the stage input, the upper half the stage output, three dwords a lane each, plain vector
//    stores, the address a workgroup-uniform row plus one lane term.  Columns past n read the frame's last point and store nothing.
//    The stores share vmcnt with the weight ring: the piece barriers' vmcnt(24) stays correct with more operations outstanding (the
//    loads return in order among themselves), it only waits more conservatively;
//  * per-frame step counts and a launch order exactly as ode_sample_tape.hip (XC_FRAME_STEPS): frame order[p] is written at position
//    p, rows s < S_f only, the count clamped to 0..max_steps, a count of 0 returns before anything is read;
//  * RANGE GUARD as the inference kernel: a point whose largest scaled activation is not below 65520 gets NaN in its three components
//    of y_out and the launch's status word gets bit value 4 (XH_GUARD_TAPE; cnf_rk4_h3w_kernel owns 1, cnf_dp5_h3w_kernel 2).  The
//    tape rows of such a point hold whatever the arithmetic produced: x is NaN already, nothing downstream trusts them.
// No atomics but that atomicOr; no inline assembly beyond the shared text's and the final vmcnt(0).
#define XH_OLD_FLUSH 0
#define XH_OLD_DMA 0
#define XH_NO_FLUSH1 0
#define XH_NO_FLUSH2 0
#define XH_STAMP(i)
#include "ode_h3w.h"

#define XH_GUARD_TAPE 4u         // the status word's bit of this kernel

struct CnfSampleTapeH3Args {
    const float *y_in, *hyper, *tcol, *w0, *b0, *b1, *b2, *w3, *b3;
    const float *t_end;           // one float in device memory
    const unsigned char *w1x, *w2x;   // the pack_cnf_h3 packs
    float *y_out;                 // (BT,n,3)
    float *ys, *ka;               // [steps][4][BT][n][3] stage inputs, stage outputs; with a table [max_steps][4][position][n][3]
    unsigned *status;             // one word per launch, zeroed in front of it: XH_GUARD_TAPE set <-> the range guard tripped
    int ldh, n, steps;
    // the *_frames_* entry only (NULL / 0 / NULL otherwise), as CnfSampleTapeArgs
    const int *steps_tab;
    int max_steps;
    const int *order;
};

__global__ __launch_bounds__(256, 1) void cnf_sample_tape_h3w_kernel(CnfSampleTapeH3Args a)
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
    for (int d = 0; d < 3; ++d) y[d] = a.y_in[((long)bt * a.n + ccol) * 3 + d];

    // (the table registers: the same text in cnf_rk4_h3w_kernel and cnf_dp5_h3w_kernel, see ode_h3w_setup.inc)
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

    // reversed time axis: from t_end down to 0, h < 0; the expressions of cnf_rk4_h3w_kernel with reverse = 1
    const float t_end = a.t_end[0];
    const double t0 = (double)t_end, t1 = 0.0;
    const double h = (t1 - t0) / (double)S;
    const float hh = (float)h, h2 = (float)(0.5 * h), h6 = (float)(h / 6.0);

    // the tape: an evaluation's row of this workgroup row's position is (step * 4 + stage) * ev_rows + pos_row floats into ys / ka
    // (workgroup-uniform), the lane's point 3 col further: the lower half of a wave stores stage inputs, the upper half stage outputs
    const long ev_rows = (long)gridDim.y * a.n * 3, pos_row = (long)blockIdx.y * a.n * 3;
    const bool st_in = cvalid && lane0 < 32, st_out = cvalid && lane0 >= 32;

#include "ode_h3w_ring.inc"

    for (int step = 0; step < S; ++step) {
#pragma unroll 1
        for (int stage = 0; stage < 4; ++stage) {
            const double tc = (stage == 0) ? 0.0 : (stage == 3 ? 1.0 : 0.5);
            const float t = (float)(t0 + (double)step * h + tc * h);
            const float aw = (stage == 0) ? 0.f : (stage == 3 ? hh : h2);
            const long ev = (long)(step * 4 + stage) * ev_rows + pos_row;
#define XH_STAGE_INPUT                                                                                        \
    float ys[3];                                                                                              \
    _Pragma("unroll") for (int d = 0; d < 3; ++d) ys[d] = (stage == 0) ? y[d] : y[d] + aw * kprev[d];         \
    if (st_in) {                                                                                              \
        float *tp = a.ys + ev + 3 * col;                                                                      \
        _Pragma("unroll") for (int d = 0; d < 3; ++d) tp[d] = ys[d];                                          \
    }
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
            if (st_out) {
                float *tp = a.ka + ev + 3 * col;
#pragma unroll
                for (int d = 0; d < 3; ++d) tp[d] = kprev[d];
            }
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) y[d] = y[d] + h6 * kacc[d];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the pieces left in flight by the last stage

    // range guard: the two halves of a column split disjoint units of the same point
    xmax = fmaxf(xmax, __shfl_xor(xmax, 32));
    const bool bad = !(xmax < XH_F16_LIMIT);
    if (st_in) {
        if (bad) atomicOr(a.status, XH_GUARD_TAPE);
#pragma unroll
        for (int d = 0; d < 3; ++d) a.y_out[((long)bt * a.n + col) * 3 + d] = bad ? __uint_as_float(0x7fc00000u) : y[d];
    }
}

// one launch path of both entries: steps_tab == NULL is the uniform solve (`steps` for every frame, tape position = frame)
static int cnf_sample_tape_h3_launch(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0, const float *b0, const void *w1h,
                                     const float *b1, const void *w2h, const float *b2, const float *w3, const float *b3, int H, const float *t_end,
                                     int steps, const int *steps_tab, int max_steps, const int *order, unsigned *status, float *y_out, float *ys,
                                     float *ka, int BT, int n, void *stream)
{
    CASPR_REQUIRE(y_in && hyper && tcol && w0 && b0 && w1h && b1 && w2h && b2 && w3 && b3 && t_end && y_out && ys && ka && status,
                  "cnf_sample_tape_h3: null pointer");
    CASPR_REQUIRE(H == XC_H, "cnf_sample_tape_h3: hidden width %d unsupported (kernel is built for 512-512-512, flow.py:89)", H);
    CASPR_REQUIRE(BT > 0 && BT <= 65535 && n > 0 && ldh >= 2 * (3 * H + 3), "cnf_sample_tape_h3: bad sizes");
    CASPR_REQUIRE(n >= XH_PTS, "cnf_sample_tape_h3: n = %d is below the kernel's 128-point workgroup: launch caspr_cnf_sample_tape_f32 / "
                  "caspr_cnf_sample_tape_frames_f32 (the 64-point kernel) for it", n);
    if (steps_tab) {
        CASPR_REQUIRE(max_steps >= 1 && max_steps <= 4096, "cnf_sample_tape_h3_frames: max_steps %d outside 1..4096", max_steps);
    } else {
        CASPR_REQUIRE(steps > 0 && steps <= (1 << 20), "cnf_sample_tape_h3: bad sizes");
    }
    CASPR_REQUIRE(((uintptr_t)w1h % 16) == 0 && ((uintptr_t)w2h % 16) == 0 && ((uintptr_t)w0 % 16) == 0 && ((uintptr_t)w3 % 16) == 0,
                  "cnf_sample_tape_h3: weights must be 16-byte aligned");
    CnfSampleTapeH3Args a;
    a.y_in = y_in; a.hyper = hyper; a.tcol = tcol; a.w0 = w0; a.b0 = b0; a.b1 = b1; a.b2 = b2; a.w3 = w3; a.b3 = b3;
    a.t_end = t_end; a.w1x = (const unsigned char *)w1h; a.w2x = (const unsigned char *)w2h;
    a.y_out = y_out; a.ys = ys; a.ka = ka; a.status = status;
    a.ldh = ldh; a.n = n; a.steps = steps;
    a.steps_tab = steps_tab; a.max_steps = max_steps; a.order = order;
    static CasprLdsOptIn optin;
    hipError_t err = caspr_lds_opt_in(optin, (const void *)cnf_sample_tape_h3w_kernel, XH_LDS);
    if (err != hipSuccess) {
        caspr_set_error("cnf_sample_tape_h3: hipFuncSetAttribute failed: %s", hipGetErrorString(err));
        return CASPR_ELAUNCH;
    }
    err = hipMemsetAsync(status, 0, sizeof(unsigned), (hipStream_t)stream);
    if (err != hipSuccess) {
        caspr_set_error("cnf_sample_tape_h3: hipMemsetAsync failed: %s", hipGetErrorString(err));
        return CASPR_ELAUNCH;
    }
    cnf_sample_tape_h3w_kernel<<<dim3(ceil_div(n, XH_PTS), BT), dim3(256), XH_LDS, (hipStream_t)stream>>>(a);
    CASPR_CHECK_LAUNCH("cnf_sample_tape_h3");
    return CASPR_OK;
}

// cnf.py:70-128 (reverse = True, logpx = None) as caspr.py:262 runs it in decode(), on the evaluation of caspr_cnf_rk4_h3_f32, with the
// tape of train/flow_grad.py: CnfSampleSolve
extern "C" int caspr_cnf_sample_tape_h3_f32(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0, const float *b0,
                                            const void *w1h, const float *b1, const void *w2h, const float *b2, const float *w3, const float *b3,
                                            int H, const float *t_end, int steps, unsigned *status, float *y_out, float *ys, float *ka, int BT,
                                            int n, void *stream)
{
    return cnf_sample_tape_h3_launch(y_in, hyper, ldh, tcol, w0, b0, w1h, b1, w2h, b2, w3, b3, H, t_end, steps, nullptr, 0, nullptr, status, y_out, ys,
                                     ka, BT, n, stream);
}

// the same solve with a step count per frame (train/flow_grad.py: CnfSampleSolveFrames): steps_tab (BT), clamped to 0..max_steps = the
// step rows of ys / ka; order (BT) or NULL; the tape in launch order
extern "C" int caspr_cnf_sample_tape_h3_frames_f32(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0,
                                                   const float *b0, const void *w1h, const float *b1, const void *w2h, const float *b2,
                                                   const float *w3, const float *b3, int H, const float *t_end, const int32_t *steps_tab,
                                                   int max_steps, const int32_t *order, unsigned *status, float *y_out, float *ys, float *ka,
                                                   int BT, int n, void *stream)
{
    CASPR_REQUIRE(steps_tab, "cnf_sample_tape_h3_frames: null step table");
    return cnf_sample_tape_h3_launch(y_in, hyper, ldh, tcol, w0, b0, w1h, b1, w2h, b2, w3, b3, H, t_end, 0, steps_tab, max_steps, order, status,
                                     y_out, ys, ka, BT, n, stream);
}
