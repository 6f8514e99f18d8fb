// ode_latent_dp5_adjoint.inc -- the reverse sweep of the adaptive latent solve (latent_ode_model.py:45-70,85-99: the reference trains
// through odeint_adjoint on dopri5; ode_latent_dp5.hip is the solve, caspr_latent_dopri5_tape_f32 its taping form).  The derivative
// is the one of the forward's OWN discrete map with its accepted step sequence held fixed (DESIGN.md section 4): per sequence the
// accepted steps n = 0 .. N-1 from z_n with size dt_n,
//     k1 = f(z_n), k_s = f(z_n + dt_n sum_q BETA[s][q] k_q) (s = 2..6), z_{n+1} = z_n + dt_n sum_q BETA[7][q] k_q, k7 = f(z_{n+1}),
// a stamp at a step's end reads z_{n+1}, a stamp strictly inside it the quartic dp5_interp(z_n, z_{n+1}, y_mid, k1, k7, dt_n) at
// theta = (t - t0_n) / dt_n with y_mid = z_n + dt_n sum_q CMID[q] k_q, a stamp equal to times[0] reads z_0.  Every dt_n, t0_n, theta
// and every accept / reject decision is a constant; rejected attempts and the initial-step selection contribute nothing.
//
// One launch with the structure of latent_dp5_kernel: one 512-thread workgroup per 16 sequences (the columns of the f32 MFMA tile),
// weights streamed through the same register ring (ldp_layer), no inter-workgroup communication, no spin waits, no atomics.
//  * the outer loop runs n = Nmax-1 .. 0, Nmax the largest accepted count among the workgroup's finished columns, read from LDS behind
//    a barrier: workgroup-uniform, bounded by max_steps.  A column with fewer steps idles with dt = 0, z = 0 and zero adjoints until
//    its own last step comes up; an unfinished sequence (counters' finished word 0) idles throughout and gets NaN in its gz row;
//  * per step the wave that owns a column (wave w: columns 2w, 2w + 1, lane = component) scatters gout of the step's stamps by the
//    interpolant's coefficients -- the stamps with t0_n < t <= t1_n, t0_n rebuilt with the forward's f64 running sum and compared as
//    the forward compares -- then the workgroup recomputes stages 1..6 from the taped (z_n, dt_n) with the forward's own evaluation
//    text (ode_latent_dp5_eval.inc), storing every evaluation's layer inputs (x, h1, h2, h3) as rows, and runs six vector-Jacobian
//    products in reverse order: f(z_{n+1}) [which is step n + 1's stage 1, or the evaluation at the final state], stages 6 .. 2.
//    A product is the four-layer chain on the TRANSPOSED packed weights W3^T, W2^T, W1^T, W0^T with tanh' = 1 - h^2 read back from
//    the rows; each layer's input is stored as that layer's delta row.  The adjoint of k1 is carried to step n - 1 as the adjoint of
//    its k7; after the loop one more product takes it through f(z_0): 1 + 6 N evaluations per sequence;
//  * rows: evaluation e of sequence b (e = 6 n + s - 1 for stage s of step n, 6 N for the final state) is row b (1 + 6 max_steps) + e
//    of all eight buffers.  Rows a sequence does not use are never written: the caller zero-fills, and dW_l = delta_l^T input_l,
//    db_l = colsum(delta_l) are one weight-gradient product per layer over all rows.
// A sequence's gz row and rows are bit-identical whichever column, workgroup or batch it sits in (MFMA columns are independent and an
// idling column adds zeros).
//
// A text fragment of ode_latent_dp5.hip's translation unit (included at its end: the library's list of sources stays as it is): it
// reads that file's tableau (LDP_BETA, LDP_CMID) and ode_latent_dp5.h, and redefines the evaluation text's two hooks.
#undef LDP_EVAL_IN
#undef LDP_EVAL_ROW

// the hooks of ode_latent_dp5_eval.inc: the recomputation stores the evaluation's layer inputs as rows (evaluation eoff of the step
// whose first row is s_rb[column]; only_last: only for the columns whose last step this is -- the evaluation at the final state)
#define LDA_ROW_OF(c) ((s_rb[c] >= 0 && (!only_last || s_last[c])) ? (long)s_rb[c] + eoff : -1L)
#define LDP_EVAL_IN(row, i, d, c, v)                      \
    {                                                     \
        const long row_ = LDA_ROW_OF(c);                  \
        if (row_ >= 0) rows_x[row_ * xw + d] = v;         \
    }
#define LDP_EVAL_ROW(l, r, v)                                               \
    {                                                                       \
        const long row_ = LDA_ROW_OF(j);                                    \
        if (row_ >= 0) st4(rows_h##l + row_ * H + (r) * 16 + 4 * g, v);     \
    }

__global__ __launch_bounds__(512) void latent_dp5_adjoint_kernel(const float *__restrict__ gout, const float *__restrict__ times, int B, int Tu, int D,
                                                                 int H, int max_steps, const int *__restrict__ counters,
                                                                 const float *__restrict__ tape_z, const float *__restrict__ tape_dt,
                                                                 const float *__restrict__ w0p, const float *__restrict__ b0,
                                                                 const float *__restrict__ w1p, const float *__restrict__ b1,
                                                                 const float *__restrict__ w2p, const float *__restrict__ b2,
                                                                 const float *__restrict__ w3p, const float *__restrict__ b3,
                                                                 const float *__restrict__ w3t, const float *__restrict__ w2t,
                                                                 const float *__restrict__ w1t, const float *__restrict__ w0t,
                                                                 float *rows_x, int xw, float *rows_h1, float *rows_h2, float *rows_h3,
                                                                 float *__restrict__ del0, float *__restrict__ del1, float *__restrict__ del2,
                                                                 float *__restrict__ del3, float *__restrict__ gz)
{
    __shared__ __attribute__((aligned(16))) float s_in[16 * LDP_NCOL * 4];
    __shared__ __attribute__((aligned(16))) float s_h1[128 * LDP_NCOL * 4], s_h2[128 * LDP_NCOL * 4];
    __shared__ float s_z[LDP_EL], s_k[6][LDP_EL];                    // z_n and k1..k6 of the step; element (d, c) at d * 16 + c
    __shared__ float s_az0[LDP_EL], s_az1[LDP_EL], s_ak[7][LDP_EL];   // adjoints of z_n, z_{n+1}, k1..k7
    __shared__ float s_gx[LDP_EL];                                    // a vector-Jacobian product's result
    __shared__ float s_dt[LDP_NCOL];
    __shared__ int s_N[LDP_NCOL], s_rb[LDP_NCOL], s_last[LDP_NCOL];   // accepted steps (0: idles throughout); the step's first row or -1; last step
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, j = lane & 15;
    const int b0i = blockIdx.x * LDP_NCOL;
    const int KC0 = 2 * ((D + 31) / 32), KCH = 2 * ((H + 31) / 32);
    const int RTH = (H + 15) / 16, RTD = (D + 15) / 16;
    const int rows_per_seq = 1 + 6 * max_steps;

    for (int i = tid; i < LDP_EL; i += 512) {
        s_z[i] = s_az0[i] = s_az1[i] = s_gx[i] = 0.f;
#pragma unroll
        for (int q = 0; q < 6; ++q) s_k[q][i] = 0.f;
#pragma unroll
        for (int q = 0; q < 7; ++q) s_ak[q][i] = 0.f;
    }
    for (int i = tid; i < 16 * LDP_NCOL * 4; i += 512) s_in[i] = 0.f;   // K padding rows stay zero
    for (int i = tid; i < 128 * LDP_NCOL * 4; i += 512) { s_h1[i] = 0.f; s_h2[i] = 0.f; }
    if (tid < LDP_NCOL) {
        const int b = b0i + tid;
        const bool ok = b < B && counters[(long)b * 4 + 3] != 0;
        s_N[tid] = ok ? min(counters[(long)b * 4], max_steps) : 0;
        s_dt[tid] = 0.f;
        s_rb[tid] = -1;
        s_last[tid] = 0;
    }
    __syncthreads();
    int Nmax = 0;
#pragma unroll
    for (int c = 0; c < LDP_NCOL; ++c) Nmax = max(Nmax, s_N[c]);        // workgroup-uniform: read behind the barrier

    int eoff = 0;
    bool only_last = false;
#include "ode_latent_dp5_eval.inc"

    // dL/d(stage input) from dL/d(stage output) `a` of evaluation eoff: s_gx = J^T a, the layers' inputs stored as delta rows
    auto vjp = [&](const float *a) {
        for (int i = tid; i < LDP_EL; i += 512) {
            const int d = i / LDP_NCOL, c = i % LDP_NCOL;
            if (d < D) {
                const float v = a[i];
                s_in[btile_off(d >> 2, c, LDP_NCOL) + (d & 3)] = v;
                if (s_rb[c] >= 0) del3[((long)s_rb[c] + eoff) * xw + d] = v;
            }
        }
        __syncthreads();
        const long row = s_rb[j] >= 0 ? (long)s_rb[j] + eoff : -1L;
        auto hidden = [&](const float *hrows, float *del, float *dst, int r, f32x4 a4) {   // delta = (W^T delta') (1 - h^2)
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row >= 0) {
                const f32x4 h = ld4(hrows + row * H + r * 16 + 4 * g);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = a4[q] * (1.f - h[q] * h[q]);
                st4(del + row * H + r * 16 + 4 * g, v);
            }
            st4(dst + btile_off(r * 4 + g, j, LDP_NCOL), v);
        };
        for (int rt = wave * 4; rt < RTH; rt += 32)
            ldp_layer<4>(w3t, KC0, rt, s_in, lane, [&](int r, f32x4 a4) { hidden(rows_h3, del2, s_h1, r, a4); });
        __syncthreads();
        for (int rt = wave * 4; rt < RTH; rt += 32)
            ldp_layer<4>(w2t, KCH, rt, s_h1, lane, [&](int r, f32x4 a4) { hidden(rows_h2, del1, s_h2, r, a4); });
        __syncthreads();
        for (int rt = wave * 4; rt < RTH; rt += 32)
            ldp_layer<4>(w1t, KCH, rt, s_h2, lane, [&](int r, f32x4 a4) { hidden(rows_h1, del0, s_h1, r, a4); });
        __syncthreads();
        if (wave < RTD)
            ldp_layer<1>(w0t, KCH, wave, s_h1, lane, [&](int r, f32x4 a4) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int d = r * 16 + 4 * g + q;
                    if (d < D) s_gx[d * LDP_NCOL + j] = a4[q];
                }
            });
        __syncthreads();
    };

    // ---- the control state of this wave's two columns (wave-uniform), lane = component d
    const bool dv = lane < D;
    const int ei[2] = {lane * LDP_NCOL + 2 * wave, lane * LDP_NCOL + 2 * wave + 1};
    const float t_first = times[0];
    int hi[2] = {Tu, Tu};                 // the stamps [hi, Tu) have been scattered: a finished column's last step ends behind all of them

    for (int n = Nmax - 1; n >= 0; --n) {
        // ---- this step's (z_n, dt_n); gout of its stamps onto z_n, z_{n+1}, y_mid, k1, k7; y_mid onto z_n and k1..k7
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const int c = 2 * wave + cc, e = ei[cc];
            const long b = b0i + c;
            const int N = s_N[c];
            const bool act = n < N;
            float dt = 0.f, z = 0.f;
            double a0 = 0.0, a1 = 0.0, am = 0.0, aa = 0.0, ab = 0.0;
            if (act) {
                const float *dts = tape_dt + b * max_steps;
                dt = dts[n];
                if (dv) z = tape_z[(b * max_steps + n) * D + lane];
                double t0 = 0.0;
                for (int m = 0; m < n; ++m) t0 += (double)dts[m];      // the forward's running sum (tc += (double)dt)
                const double t1 = t0 + (double)dt, h = (double)dt;
                int i = hi[cc];
                while (i > 0 && (double)(times[i - 1] - t_first) > t0) {   // ascending stamps: this step's are the tail of [0, hi)
                    --i;
                    const double tn = (double)(times[i] - t_first);
                    const double gv = dv ? (double)gout[(b * Tu + i) * D + lane] : 0.0;
                    if (tn == t1)
                        a1 += gv;
                    else {                                             // d dp5_interp / d (y0, y1, ymid, f0, f1) at x  (dp5_rules.h)
                        const double x = (tn - t0) / (t1 - t0), x2 = x * x, x3 = x2 * x, x4 = x2 * x2;
                        a0 += gv * (1.0 - 8.0 * x4 + 18.0 * x3 - 11.0 * x2);
                        a1 += gv * (-8.0 * x4 + 14.0 * x3 - 5.0 * x2);
                        am += gv * (16.0 * x4 - 32.0 * x3 + 16.0 * x2);
                        aa += gv * h * (-2.0 * x4 + 5.0 * x3 - 4.0 * x2 + x);
                        ab += gv * h * (2.0 * x4 - 3.0 * x3 + x2);
                    }
                }
                hi[cc] = i;
            }
            const float amf = (float)am;
            s_z[e] = z;
            s_az1[e] = s_az0[e] + (float)a1;                            // carried: the adjoint of step n + 1's start state
            s_az0[e] = (float)a0 + amf;
            s_ak[6][e] = s_ak[0][e] + (float)ab + dt * LDP_CMID[6] * amf;   // carried: the adjoint of step n + 1's k1 (FSAL)
            s_ak[0][e] = (float)aa + dt * LDP_CMID[0] * amf;
#pragma unroll
            for (int q = 1; q < 6; ++q) s_ak[q][e] = dt * LDP_CMID[q] * amf;
            if (lane == 0) {
                s_dt[c] = dt;
                s_rb[c] = act ? (int)(b * rows_per_seq + 6 * n) : -1;
                s_last[c] = act && n == N - 1;
            }
        }
        __syncthreads();
        int need7 = 0;
#pragma unroll
        for (int c = 0; c < LDP_NCOL; ++c) need7 |= s_last[c];        // workgroup-uniform

        // ---- stages 1..6 again, rows 6 n .. 6 n + 5; the evaluation at the final state for the columns that end here (row 6 N)
        only_last = false;
#pragma unroll 1
        for (int s = 1; s <= 6; ++s) {
            eoff = s - 1;
            write_in(s == 1 ? 0 : s);
            dyn(s_k[s - 1]);
        }
        if (need7) {
            only_last = true;
            eoff = 6;
            write_in(7);
            dyn(s_gx);                                                // the value is not needed: k7 enters through its adjoint only
            only_last = false;
        }

        // ---- f(z_{n+1}): adj z_{n+1} += J^T adj k7; then z_{n+1} = z_n + dt sum_q BETA[7][q] k_q
        eoff = 6;
        vjp(s_ak[6]);
        for (int i = tid; i < LDP_EL; i += 512) {
            const float a = s_az1[i] + s_gx[i], dt = s_dt[i % LDP_NCOL];
            s_az0[i] += a;
#pragma unroll
            for (int q = 0; q < 6; ++q)
                if (LDP_BETA[7][q] != 0.f) s_ak[q][i] += dt * LDP_BETA[7][q] * a;
        }
        __syncthreads();
        // ---- stages 6 .. 2: x_s = z_n + dt sum_q BETA[s][q] k_q
#pragma unroll 1
        for (int s = 6; s >= 2; --s) {
            eoff = s - 1;
            vjp(s_ak[s - 1]);
            for (int i = tid; i < LDP_EL; i += 512) {
                const float a = s_gx[i], dt = s_dt[i % LDP_NCOL];
                s_az0[i] += a;
                for (int q = 0; q + 2 <= s; ++q)
                    if (LDP_BETA[s][q] != 0.f) s_ak[q][i] += dt * LDP_BETA[s][q] * a;
            }
            __syncthreads();
        }
    }

    // ---- f(z_0) (row 0 of every sequence that took a step), then gz = adj z_0 + J^T adj k1 + gout of the stamps equal to times[0]
    eoff = 0;
    vjp(s_ak[0]);
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
        const int c = 2 * wave + cc, e = ei[cc];
        const long b = b0i + c;
        if (b >= B || !dv) continue;
        float v = s_az0[e] + s_gx[e];
        if (counters[b * 4 + 3] == 0)
            v = __builtin_nanf("");
        else {
            double a = 0.0;
            for (int i = 0; i < hi[cc]; ++i) a += (double)gout[(b * Tu + i) * D + lane];
            v += (float)a;
        }
        gz[b * D + lane] = v;
    }
}

extern "C" int caspr_latent_dopri5_adjoint_f32(const float *gout, const float *times, int B, int Tu, int D, int H, int max_steps,
                                               const int32_t *counters, const float *tape_z, const float *tape_dt, const float *w0p,
                                               const float *b0, const float *w1p, const float *b1, const float *w2p, const float *b2,
                                               const float *w3p, const float *b3, const float *w3tp, const float *w2tp, const float *w1tp,
                                               const float *w0tp, float *rows_x, int xw, float *rows_h1, float *rows_h2, float *rows_h3,
                                               float *d0, float *d1, float *d2, float *d3, float *gz, void *stream)
{
    CASPR_REQUIRE(gout && times && counters && tape_z && tape_dt && w0p && w1p && w2p && w3p && b0 && b1 && b2 && b3 && w3tp && w2tp && w1tp && w0tp &&
                      rows_x && rows_h1 && rows_h2 && rows_h3 && d0 && d1 && d2 && d3 && gz,
                  "latent_dopri5_adjoint: null pointer");
    CASPR_REQUIRE(B > 0 && Tu > 0 && max_steps > 0 && D > 0 && H > 0 && xw >= D && xw % 4 == 0,
                  "latent_dopri5_adjoint: bad sizes B=%d Tu=%d D=%d H=%d max_steps=%d xw=%d", B, Tu, D, H, max_steps, xw);
    CASPR_REQUIRE((long)B * (1 + 6 * (long)max_steps) < (1L << 31), "latent_dopri5_adjoint: B (1 + 6 max_steps) = %ld rows do not fit 31 bits",
                  (long)B * (1 + 6 * (long)max_steps));
    if (!(D <= 64 && H <= 512 && H % 64 == 0)) {
        caspr_set_error("latent_dopri5_adjoint: unsupported sizes D=%d H=%d (need D<=64, H<=512, H %% 64 == 0)", D, H);
        return CASPR_EUNSUP;
    }
    latent_dp5_adjoint_kernel<<<dim3(ceil_div(B, LDP_NCOL)), dim3(512), 0, (hipStream_t)stream>>>(
        gout, times, B, Tu, D, H, max_steps, (const int *)counters, tape_z, tape_dt, w0p, b0, w1p, b1, w2p, b2, w3p, b3, w3tp, w2tp, w1tp, w0tp, rows_x, xw,
        rows_h1, rows_h2, rows_h3, d0, d1, d2, d3, gz);
    CASPR_CHECK_LAUNCH("latent_dopri5_adjoint");
    return CASPR_OK;
}
