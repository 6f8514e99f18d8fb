// ode_sample_tape.hip -- the SAMPLING solve of one point-CNF block (cnf.py:70-128 with reverse = True and logpx = None, as
// caspr.py:262 calls it from decode()) as one launch that also writes the tape its gradient needs (train/flow_grad.py:
// CnfSampleSolve): fixed-step RK4 from t_end down to 0, no divergence, and no layer product ever leaves the chip.
//
// The ODE function evaluation is the 64-point sampling evaluation of ode_bf16x6.hip (cnf_rk4_x6_kernel<false>), shared with it as
// text (ode_x6_setup.inc, ode_x6_eval.inc with DIV = false): a wave owns 16 points and all 512 hidden units, both hidden layers on
// the bf16 matrix pipe (v_mfma_f32_16x16x32_bf16) in the exact three-way split with f32 accumulation, weight pieces by LDS-DMA into
// a double buffer.  This file adds the RK4 loop around it and what is written:
//  * besides x(0) every evaluation's point state goes to memory: the stage input (S, 4, BT, n, 3) that the reverse sweep rebuilds
//    ONE evaluation's tape from, and the stage output dy/dt (S, 4, BT, n, 3) that the gradient with respect to the step size needs.
//    12 + 12 bytes per point and evaluation: the only thing that grows with S;
//  * a step count per frame and a launch order (caspr_cnf_sample_tape_frames_f32; XC_FRAME_STEPS of ode_x6.h, as the sampling kernels
//    of inference): workgroup row p = blockIdx.y works on frame bt = order[p] with S_bt steps of h = -t_end / S_bt and writes its tape
//    at POSITION p, rows s < S_bt only.  With the longest frames first, the frames still active at step s are a prefix of the tape's
//    frame axis, which the reverse sweep slices (train/flow_grad.py: CnfSampleSolveFrames);
//  * the end time is read from device memory (the differentiable route holds sqrt_end_time^2 as a tensor: no host read-back);
//  * no MovingBatchNorm at either end (autograd keeps those), reverse direction only.
// Every store is a plain vector store by the lane that owns the value; no atomics; a point's result depends on its frame's gates
// and its own column only, never on the batch around it.  The columns of a partial workgroup (n % 64 != 0) read the frame's last
// point and write nothing.
#include "ode_x6.h"

struct CnfSampleTapeArgs {
    const float *y_in, *hyper, *tcol, *w0, *b0, *b1, *b2, *w3, *b3;
    const float *t_end;           // one float in device memory
    const unsigned char *w1x, *w2x;
    float *y_out;                 // (BT,n,3)
    float *ys, *ka;               // [steps][4][BT][n][3] stage inputs, stage outputs; with a table [max_steps][4][position][n][3]
    int ldh, n, steps;
    // the *_frames_* entry only (NULL / 0 / NULL otherwise), as CnfX6Args: frame bt takes min(max(steps_tab[bt], 0), max_steps) steps
    // (max_steps = the step rows of ys / ka: the clamp keeps the stores inside the tape), row blockIdx.y works on frame order[blockIdx.y]
    const int *steps_tab;
    int max_steps;
    const int *order;
};

__global__ __launch_bounds__(256, 1) void cnf_sample_tape_kernel(CnfSampleTapeArgs a)
{
    constexpr bool DIV = false;   // no tangent columns: a wave's 16 columns are 16 points
    const int tid = threadIdx.x, lane0 = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g0 = lane0 >> 4;
    XC_FRAME_STEPS(a, bt, S, true)
    // a wave's 16 columns are 16 points; the workgroup owns 64 points of frame bt
    const int col = blockIdx.x * XC_COLS + 16 * wave + (lane0 & 15);
    const bool cvalid = col < a.n;
    const int ccol = cvalid ? col : a.n - 1;
    const float *hy = a.hyper + (long)bt * a.ldh;
    constexpr int GOFF = 0, BOFF = 3 * XC_H + 3;
    const int sd = g0 < 3 ? g0 : 0;   // state component of this lane (lanes g == 3 carry a copy of component 0, never stored)

#include "ode_x6_setup.inc"

    float y = a.y_in[((long)bt * a.n + ccol) * 3 + sd], kacc = 0.f, kprev = 0.f;

    // reversed time axis: from t_end down to 0 (cnf.py:92-93 flips the integration times), h < 0
    const double t0 = (double)a.t_end[0];
    const double h = (0.0 - t0) / (double)S;
    const float hh = (float)h, h2 = (float)(0.5 * h), h6 = (float)(h / 6.0);

    // the first piece of layer 1; every layer pass leaves the NEXT pass's first piece in flight
    dma(a.w1x, 0, lane0 * 16);

    for (int step = 0; step < S; ++step) {
#pragma unroll 1
        for (int stage = 0; stage < 4; ++stage) {
            const double tc = (stage == 0) ? 0.0 : (stage == 3 ? 1.0 : 0.5);
            const float t = (float)(t0 + (double)step * h + tc * h);
            const float aw = (stage == 0) ? 0.f : (stage == 3 ? hh : h2);
#define XC_STAGE_INPUT ((stage == 0) ? y : y + aw * kprev)
#define XC_LAYERS_ON true
#include "ode_x6_eval.inc"
            kprev = od;
            kacc = (stage == 0) ? od : ((stage == 3) ? kacc + od : kacc + 2.0f * od);
            // ---- what the reverse sweep needs of this evaluation: its input and its output, by the lanes that own them
            // (lane (g, j), g < 3, owns component g of point j; the columns past n and the copies in g == 3 write nothing), at the
            // workgroup row's POSITION of the frame axis (= the frame itself without a launch order)
            const int colx = blockIdx.x * XC_COLS + 16 * wave + j;
            if (g < 3 && colx < a.n) {
                const long ev = (((long)(step * 4 + stage) * gridDim.y + blockIdx.y) * a.n + colx) * 3 + g;
                a.ys[ev] = ystage;
                a.ka[ev] = od;
            }
        }
        y = y + h6 * kacc;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the prefetch left in flight by the last layer pass

    if (cvalid && g0 < 3) a.y_out[((long)bt * a.n + col) * 3 + sd] = y;
}

// one launch path of both entries: steps_tab == NULL is the uniform solve (`steps` for every frame, tape position = frame)
static int cnf_sample_tape_launch(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0, const float *b0, const void *w1x,
                                  const float *b1, const void *w2x, const float *b2, const float *w3, const float *b3, int H, const float *t_end,
                                  int steps, const int *steps_tab, int max_steps, const int *order, float *y_out, float *ys, float *ka, int BT, int n,
                                  void *stream)
{
    CASPR_REQUIRE(y_in && hyper && tcol && w0 && b0 && w1x && b1 && w2x && b2 && w3 && b3 && t_end && y_out && ys && ka, "cnf_sample_tape: null pointer");
    CASPR_REQUIRE(H == XC_H, "cnf_sample_tape: hidden width %d unsupported (kernel is built for 512-512-512, flow.py:89)", H);
    CASPR_REQUIRE(BT > 0 && BT <= 65535 && n > 0 && ldh >= 2 * (3 * H + 3), "cnf_sample_tape: bad sizes");
    if (steps_tab) {
        CASPR_REQUIRE(max_steps >= 1 && max_steps <= 4096, "cnf_sample_tape_frames: max_steps %d outside 1..4096", max_steps);
    } else {
        CASPR_REQUIRE(steps > 0 && steps <= (1 << 20), "cnf_sample_tape: bad sizes");
    }
    CASPR_REQUIRE(((uintptr_t)w1x % 16) == 0 && ((uintptr_t)w2x % 16) == 0 && ((uintptr_t)w0 % 16) == 0 && ((uintptr_t)w3 % 16) == 0,
                  "cnf_sample_tape: weights must be 16-byte aligned");
    CnfSampleTapeArgs a;
    a.y_in = y_in; a.hyper = hyper; a.tcol = tcol; a.w0 = w0; a.b0 = b0; a.b1 = b1; a.b2 = b2; a.w3 = w3; a.b3 = b3;
    a.t_end = t_end; a.w1x = (const unsigned char *)w1x; a.w2x = (const unsigned char *)w2x;
    a.y_out = y_out; a.ys = ys; a.ka = ka;
    a.ldh = ldh; a.n = n; a.steps = steps;
    a.steps_tab = steps_tab; a.max_steps = max_steps; a.order = order;
    static CasprLdsOptIn optin;
    const hipError_t err = caspr_lds_opt_in(optin, (const void *)cnf_sample_tape_kernel, XC_LDS);
    if (err != hipSuccess) {
        caspr_set_error("cnf_sample_tape: hipFuncSetAttribute failed: %s", hipGetErrorString(err));
        return CASPR_ELAUNCH;
    }
    cnf_sample_tape_kernel<<<dim3(ceil_div(n, XC_COLS), BT), dim3(256), XC_LDS, (hipStream_t)stream>>>(a);
    CASPR_CHECK_LAUNCH("cnf_sample_tape");
    return CASPR_OK;
}

// cnf.py:70-128 (reverse = True, logpx = None) as caspr.py:262 runs it in decode(), with the tape of train/flow_grad.py: CnfSampleSolve
extern "C" int caspr_cnf_sample_tape_f32(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0, const float *b0,
                                         const void *w1x, const float *b1, const void *w2x, const float *b2, const float *w3, const float *b3,
                                         int H, const float *t_end, int steps, float *y_out, float *ys, float *ka, int BT, int n, void *stream)
{
    return cnf_sample_tape_launch(y_in, hyper, ldh, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, H, t_end, steps, nullptr, 0, nullptr, y_out, ys, ka, BT, n, stream);
}

// the same solve with a step count per frame (caspr.py:262 again; train/flow_grad.py: CnfSampleSolveFrames): steps_tab (BT), clamped
// to 0..max_steps = the step rows of ys / ka; order (BT) or NULL; the tape in launch order
extern "C" int caspr_cnf_sample_tape_frames_f32(const float *y_in, const float *hyper, int ldh, const float *tcol, const float *w0, const float *b0,
                                                const void *w1x, const float *b1, const void *w2x, const float *b2, const float *w3, const float *b3,
                                                int H, const float *t_end, const int32_t *steps_tab, int max_steps, const int32_t *order, float *y_out,
                                                float *ys, float *ka, int BT, int n, void *stream)
{
    CASPR_REQUIRE(steps_tab, "cnf_sample_tape_frames: null step table");
    return cnf_sample_tape_launch(y_in, hyper, ldh, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, H, t_end, 0, steps_tab, max_steps, order, y_out, ys, ka, BT, n, stream);
}
