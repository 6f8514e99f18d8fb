// ode_latent_dp5_eval.inc -- the ONE text of the latent dynamics' evaluation (latent_ode_model.py:139-147: Linear-Tanh x3, Linear) on the
// 16 columns of a workgroup, read by latent_dp5_kernel<TAPE> (ode_latent_dp5.hip) and by the reverse sweep's recomputation
// (ode_latent_dp5_adjoint.inc): write_in(row) forms a stage input in s_in, dyn(kout) evaluates s_in -> kout.  A text fragment and
// not a function: it defines the two lambdas in the including kernel's scope and reads tid, lane, wave, g, j, D, KC0, KCH, RTH, RTD,
// the B-tiles s_in / s_h1 / s_h2, the state arrays s_z / s_k / s_dt, the tableau LDP_BETA and the eight parameter pointers from it.
// The includer's hooks: LDP_EVAL_IN(row, i, d, c, v) on component d of column c of a stage input (the solve keeps y_new, the reverse
// sweep stores the row), LDP_EVAL_ROW(l, r, v) on the tanh output v (rows 16 r + 4 g .. + 3 of column j) of hidden layer l = 1, 2, 3
// (empty in the solve, the row store of the layer inputs in the reverse sweep).
    // s_in = z + dt_c * sum_q LDP_BETA[row][q] k_{q+1} as a B-tile (row d, col c); row 7 is y_new
    auto write_in = [&](int row) {
        for (int i = tid; i < LDP_EL; i += 512) {
            const int d = i / LDP_NCOL, c = i % LDP_NCOL;
            if (d < D) {
                float acc = 0.f;
                for (int q = 0; q + 2 <= row && q < 6; ++q) {
                    const float bq = LDP_BETA[row][q];
                    if (bq != 0.f) acc += bq * s_k[q][i];
                }
                if (row == 1) acc = s_k[0][i];
                const float v = s_z[i] + s_dt[c] * acc;
                s_in[btile_off(d >> 2, c, LDP_NCOL) + (d & 3)] = v;
                LDP_EVAL_IN(row, i, d, c, v)
            }
        }
    };
    auto dyn = [&](float *kout) {  // s_in -> kout ; latent_ode_model.py:139-147 (Linear-Tanh x3, Linear)
        __syncthreads();
        for (int rt = wave * 4; rt < RTH; rt += 32)
            ldp_layer<4>(w0p, KC0, rt, s_in, lane, [&](int r, f32x4 a) {
                const f32x4 bb = ld4(b0 + r * 16 + 4 * g);
                f32x4 v;
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = tanhf(a[q] + bb[q]);
                LDP_EVAL_ROW(1, r, v)
                st4(s_h1 + btile_off(r * 4 + g, j, LDP_NCOL), v);
            });
        __syncthreads();
        for (int rt = wave * 4; rt < RTH; rt += 32)
            ldp_layer<4>(w1p, KCH, rt, s_h1, lane, [&](int r, f32x4 a) {
                const f32x4 bb = ld4(b1 + r * 16 + 4 * g);
                f32x4 v;
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = tanhf(a[q] + bb[q]);
                LDP_EVAL_ROW(2, r, v)
                st4(s_h2 + btile_off(r * 4 + g, j, LDP_NCOL), v);
            });
        __syncthreads();
        for (int rt = wave * 4; rt < RTH; rt += 32)
            ldp_layer<4>(w2p, KCH, rt, s_h2, lane, [&](int r, f32x4 a) {
                const f32x4 bb = ld4(b2 + r * 16 + 4 * g);
                f32x4 v;
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = tanhf(a[q] + bb[q]);
                LDP_EVAL_ROW(3, r, v)
                st4(s_h1 + btile_off(r * 4 + g, j, LDP_NCOL), v);
            });
        __syncthreads();
        if (wave < RTD)
            ldp_layer<1>(w3p, KCH, wave, s_h1, lane, [&](int r, f32x4 a) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int d = r * 16 + 4 * g + q;
                    if (d < D) kout[d * LDP_NCOL + j] = a[q] + b3[d];
                }
            });
        __syncthreads();
    };
