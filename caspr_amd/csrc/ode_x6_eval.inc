// ode_x6_eval.inc -- ONE evaluation of the point CNF's ODE function on the 64-point bf16x6 geometry (ode_bf16x6.hip's header describes
// it): the gate tables of time t, the two 512 x 512 hidden layers on the bf16 matrix pipe in the exact three-way split, the 512 -> 3
// output layer.  Program TEXT, included inside the stage loop of cnf_rk4_x6_kernel, cnf_dp5_kernel, cnf_train_fwd_kernel and
// cnf_sample_tape_kernel, not a function: the lambdas below are the including kernel's own, and its compiled code is what it was when
// every kernel carried this text itself (an always-inline function around it already changes the register allocation).
//   the including file defines, and this file #undefs at its end:
//     XC_STAGE_INPUT  expression: this lane's state float at the stage's input (it may use `tg`: the lane's column is a tangent column)
//     XC_LAYERS_ON    condition around the two layer passes (true, but for the debug build's timing experiments)
//   expects in scope : DIV (compile-time bool: with the Hutchinson tangent columns), `a` (its .w1x, .w2x, .tcol, .b0 .. .b3), hy, GOFF,
//                      BOFF, tid, wave, lane0, sd, t (the evaluation's time, float), and what ode_x6_setup.inc leaves behind
//   leaves behind    : lane, g, j, tg, ystage (the stage input), o[3] (dy/dt of the lane's column; tangent columns: J e) and
//                      od = o[sd]; the NEXT evaluation's first weight piece is in flight
// Opaque copy of the lane id: everything derived from it (LDS offsets, DMA offsets, table addresses) is
// recomputed per stage instead of being hoisted out of the stage loop and spilled (as in ode.hip).
int lane = lane0;
asm volatile("" : "+v"(lane));
const int g = lane >> 4, j = lane & 15, lane16 = lane * 16;
// A-fragment read offset inside a plane: row (lane & 15) of a 16-row tile, piece g, swizzled as the pack
const int aoff = j * 64 + ((g ^ ((0 - (j >> 2)) & 3)) << 4);
__syncthreads();   // the previous stage's epilogues are done with the gate tables
for (int i = tid; i < 3 * XC_H; i += 256) {
    const float gt = sigmoid_fast(hy[GOFF + i] + t * a.tcol[GOFF + i]);
    const float hb = hy[BOFF + i] + t * a.tcol[BOFF + i];
    const float bl = i < XC_H ? a.b0[i] : (i < 2 * XC_H ? a.b1[i - XC_H] : a.b2[i - 2 * XC_H]);
    s_gate[i] = gt;
    s_hb[i] = bl * gt + hb;
}
if (tid < 3) {
    const float gt = sigmoid_fast(hy[GOFF + 3 * XC_H + tid] + t * a.tcol[GOFF + 3 * XC_H + tid]);
    const float hb = hy[BOFF + 3 * XC_H + tid] + t * a.tcol[BOFF + 3 * XC_H + tid];
    s_g3[tid] = gt;
    s_g3[4 + tid] = a.b3[tid] * gt + hb;
}
__syncthreads();

// ---- stage input of this lane's column, all three components
const bool tg = DIV && (lane & 8);               // this lane's column is a tangent column
const float ystage = XC_STAGE_INPUT;             // tangent lanes: e
const int jp = DIV ? (j & 7) : j;                // the point's value column
const float y0 = __shfl(ystage, jp), y1 = __shfl(ystage, 16 + jp), y2 = __shfl(ystage, 32 + jp);
float e0 = 0.f, e1 = 0.f, e2 = 0.f;              // DIV: the point's noise vector
if (DIV) {
    e0 = __shfl(ystage, 8 + jp);
    e1 = __shfl(ystage, 24 + jp);
    e2 = __shfl(ystage, 40 + jp);
}
// gated softplus layer on a value / tangent column pair (odefunc.py:98-105 and its forward-mode derivative):
//   value   : softplus(pre)                 pre = gate * (W h) + bias  (the VALUE column's, `pre`)
//   tangent : gate * (W h_t) * sigmoid(pre)                            (`lin_t` = gate * (W h_t))
// with u = e^-|pre| shared: softplus = max(pre, 0) + ln(1 + u), sigmoid = (pre >= 0 ? 1 : u) / (1 + u)
auto act_pair = [&](float pre, float lin_t) __attribute__((always_inline)) -> float {
    if (!DIV) return softplus_fast(pre);
    const float u = __builtin_amdgcn_exp2f(fabsf(pre) * -1.44269504088896341f);
    const float w1 = 1.0f + u;
    const float sp = fmaxf(pre, 0.0f) + 0.69314718055994531f * __builtin_amdgcn_logf(w1);
    const float sg = (pre >= 0.0f ? 1.0f : u) * __builtin_amdgcn_rcpf(w1);
    return tg ? lin_t * sg : sp;
};

// ---- producers of B fragments, a quarter (two k-slots) at a time; the tables of a half chunk one region earlier
auto put_pair = [&](int kc, int q, float v0, float v1) __attribute__((always_inline)) {
    unsigned p1, p2, p3;
    xc_split_pair(v0, v1, p1, p2, p3);
    bkw[kc & 1][0][q] = p1;
    bkw[kc & 1][1][q] = p2;
    bkw[kc & 1][2][q] = p3;
};
// input layer 3 -> 512 (diffeq_layers.py:83-90 + softplus): slots 2q, 2q+1 of chunk kc = units 32kc + 16h + 4g + r
auto tab_in = [&](int kc, int hf) __attribute__((always_inline)) {
    const int c = 32 * kc + 16 * hf + 4 * g;
    tg_ = ld4(s_gate + c);
    tb = ld4(s_hb + c);
    tw[0] = ld4(s_w0 + 3 * c);
    tw[1] = ld4(s_w0 + 3 * c + 4);
    tw[2] = ld4(s_w0 + 3 * c + 8);
};
auto quad_in = [&](int kc, int q) __attribute__((always_inline)) {
    const float w[12] = {tw[0][0], tw[0][1], tw[0][2], tw[0][3], tw[1][0], tw[1][1], tw[1][2], tw[1][3], tw[2][0], tw[2][1], tw[2][2], tw[2][3]};
    float v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int r = 2 * (q & 1) + e;
        const float pre = (w[3 * r] * y0 + w[3 * r + 1] * y1 + w[3 * r + 2] * y2) * tg_[r] + tb[r];
        const float lin_t = DIV ? (w[3 * r] * e0 + w[3 * r + 1] * e1 + w[3 * r + 2] * e2) * tg_[r] : 0.f;
        v[e] = act_pair(pre, lin_t);
    }
    put_pair(kc, q, v[0], v[1]);
};
// epilogue of hidden layer 1 for chunk kc of layer 2: units 32kc + 16h + 4g + r = rows of acc1[2kc + h]
auto tab_e1 = [&](int kc, int hf) __attribute__((always_inline)) {
    const int c = 32 * kc + 16 * hf + 4 * g;
    tg_ = ld4(s_gate + XC_H + c);
    tb = ld4(s_hb + XC_H + c);
};
auto quad_e1 = [&](int kc, int q) __attribute__((always_inline)) {
    float v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int r = 2 * (q & 1) + e;
        const float lin = acc1[2 * kc + (q >> 1)][r] * tg_[r];
        float pre = lin + tb[r];
        if (DIV) pre = xc_value_pre(pre);                // the value column's pre-activation
        v[e] = act_pair(pre, lin);
    }
    put_pair(kc, q, v[0], v[1]);
};

// 4 / 20 MFMAs of four row tiles: smallest terms first; term-major, i.e. four independent accumulators between
// dependent MFMAs
auto mma_head = [&](f32x4 (&acc)[32], const bf16x8 (&af)[4][3], const u32x4 (&b)[3], int m0) __attribute__((always_inline)) {
    const bf16x8 b0 = __builtin_bit_cast(bf16x8, b[0]);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[m0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u][2], b0, acc[m0 + u], 0, 0, 0);
};
auto mma_tail = [&](f32x4 (&acc)[32], const bf16x8 (&af)[4][3], const u32x4 (&b)[3], int m0) __attribute__((always_inline)) {
    const bf16x8 b0 = __builtin_bit_cast(bf16x8, b[0]), b1 = __builtin_bit_cast(bf16x8, b[1]), b2 = __builtin_bit_cast(bf16x8, b[2]);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[m0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u][1], b1, acc[m0 + u], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[m0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u][0], b2, acc[m0 + u], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[m0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u][1], b0, acc[m0 + u], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[m0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u][0], b1, acc[m0 + u], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[m0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[u][0], b0, acc[m0 + u], 0, 0, 0);
};

// One layer pass.  A piece (48 KB, k chunk p >> 1, row half p & 1) is four groups of four row tiles (24 MFMAs each),
// read into two fragment sets alternately and skewed by one group: a scheduling region = the 12 reads of group
// G+1, interleaved two per MFMA with the first MFMAs of the 20 that remain of group G ("tail"), then the first
// four MFMAs of group G+1 ("head") -- hipcc waits with lgkmcnt(0), never a counted wait, before the first use of
// a set, and at the head that wait is free.  Six of the eight regions of a k chunk also carry a quarter of the
// next chunk's B fragments (VALU) or the table reads for it.  sched_group_barrier builds the patterns,
// sched_barrier(0) closes a region (hipcc otherwise sinks every read to just before its use): the XC_REGION_* macros of
// ode_x6.h.  The last group of piece p-1 finishes after the barrier of piece p.
auto layer = [&](const unsigned char *wx, const unsigned char *wnext, f32x4 (&acc)[32], auto tab, auto quad) __attribute__((always_inline)) {
#pragma unroll
    for (int mi = 0; mi < 32; ++mi) acc[mi] = (f32x4){0.f, 0.f, 0.f, 0.f};
    bf16x8 af0[4][3], af1[4][3];
    auto rd = [&](bf16x8 (&af)[4][3], const unsigned char *A, int G) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) af[u][pl] = *(const bf16x8 *)(A + pl * XC_PA + (4 * G + u) * 1024);
    };
#pragma unroll
    for (int p = 0; p < XC_NPIECE; ++p) {
        // piece p (its DMA was issued one piece ago) has landed once nothing is outstanding; lgkmcnt: this wave's
        // reads of the buffer about to be refilled.  Raw barrier: no compiler-added waits.
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();   // piece p is there for every wave; everybody is done with buffer (p + 1) & 1
        asm volatile("" ::: "memory");
        const int kc = p >> 1, mt = p & 1;
        const int kcp = (p - 1) >> 1, mtp = (p - 1) & 1;
        const bool more = kc + 1 < 16;   // a next chunk to produce
        const unsigned char *wq = p + 1 < XC_NPIECE ? wx : wnext;
        const int pn = p + 1 < XC_NPIECE ? p + 1 : 0;
        const unsigned char *A = wbuf + (p & 1) * XC_PIECE + aoff;
        // region 0: read group 0 | the rest of the previous piece's group 3 | first MFMAs of group 0
        __builtin_amdgcn_sched_barrier(0);
        rd(af0, A, 0);
        dma(wq, pn, lane16, 0, 4);
        if (p > 0) mma_tail(acc, af1, bkw[kcp & 1], 16 * mtp + 12);
        mma_head(acc, af0, bkw[kc & 1], 16 * mt);
        if (more && mt == 0) {
            tab(kc + 1, 0);
            XC_REGION_TAB
        } else if (more) {
            quad(kc + 1, 2);
            XC_REGION_VALU
        } else {
            XC_REGION_PLAIN
        }
        // region 1
        rd(af1, A, 1);
        dma(wq, pn, lane16, 4, 8);
        mma_tail(acc, af0, bkw[kc & 1], 16 * mt);
        mma_head(acc, af1, bkw[kc & 1], 16 * mt + 4);
        if (more) {
            quad(kc + 1, mt == 0 ? 0 : 3);
            XC_REGION_VALU
        } else {
            XC_REGION_PLAIN
        }
        // region 2
        rd(af0, A, 2);
        dma(wq, pn, lane16, 8, 12);
        mma_tail(acc, af1, bkw[kc & 1], 16 * mt + 4);
        mma_head(acc, af0, bkw[kc & 1], 16 * mt + 8);
        if (more && mt == 0) {
            quad(kc + 1, 1);
            XC_REGION_VALU
        } else {
            XC_REGION_PLAIN
        }
        // region 3
        rd(af1, A, 3);
        mma_tail(acc, af0, bkw[kc & 1], 16 * mt + 8);
        mma_head(acc, af1, bkw[kc & 1], 16 * mt + 12);
        if (more && mt == 0) {
            tab(kc + 1, 1);
            XC_REGION_TAB
        } else {
            XC_REGION_PLAIN
        }
    }
    mma_tail(acc, af1, bkw[((XC_NPIECE - 1) >> 1) & 1], 16 * ((XC_NPIECE - 1) & 1) + 12);
};

float part[3] = {0.f, 0.f, 0.f};
if (XC_LAYERS_ON) {
    // chunk 0 of layer 1 up front (exposed: 1/16 of the input layer)
    tab_in(0, 0);
    quad_in(0, 0);
    quad_in(0, 1);
    tab_in(0, 1);
    quad_in(0, 2);
    quad_in(0, 3);
    layer(a.w1x, a.w2x, acc1, tab_in, quad_in);
    // chunk 0 of layer 2
    tab_e1(0, 0);
    quad_e1(0, 0);
    quad_e1(0, 1);
    tab_e1(0, 1);
    quad_e1(0, 2);
    quad_e1(0, 3);
    layer(a.w2x, a.w1x, acc2, tab_e1, quad_e1);
}
{
    // ---- epilogue of hidden layer 2 + the 512 -> 3 output layer as a per-lane partial dot product (tables one
    // row tile ahead)
    int le = lane;   // opaque again: the table addresses must not be hoisted above the product loop
    asm volatile("" : "+v"(le));
    const int ge = le >> 4;
    f32x4 tq[2][5];
    auto ld_e2 = [&](int set, int mi) __attribute__((always_inline)) {
        const int c = 16 * mi + 4 * ge;
        tq[set][0] = ld4(s_gate + 2 * XC_H + c);
        tq[set][1] = ld4(s_hb + 2 * XC_H + c);
        tq[set][2] = ld4(s_w3 + c);
        tq[set][3] = ld4(s_w3 + XC_H + c);
        tq[set][4] = ld4(s_w3 + 2 * XC_H + c);
    };
    ld_e2(0, 0);
#pragma unroll
    for (int mi = 0; mi < 32; ++mi) {
        if (mi + 1 < 32) ld_e2((mi + 1) & 1, mi + 1);
        __builtin_amdgcn_sched_barrier(0);
        const f32x4 gt = tq[mi & 1][0], hb = tq[mi & 1][1], wx3 = tq[mi & 1][2], wy3 = tq[mi & 1][3], wz3 = tq[mi & 1][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float lin = acc2[mi][r] * gt[r];
            float pre = lin + hb[r];
            if (DIV) pre = xc_value_pre(pre);
            const float hv = act_pair(pre, lin);
            part[0] += wx3[r] * hv;
            part[1] += wy3[r] * hv;
            part[2] += wz3[r] * hv;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}
// ---- output ConcatSquash (no softplus: odefunc.py:103): sum the four lane groups, every lane gets all three
float o[3];
#pragma unroll
for (int d = 0; d < 3; ++d) {
    float v = part[d];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    o[d] = (DIV && tg) ? v * s_g3[d] : v * s_g3[d] + s_g3[4 + d];    // tangent columns: J e has no bias term
}
const float od = sd == 0 ? o[0] : (sd == 1 ? o[1] : o[2]);
#undef XC_STAGE_INPUT
#undef XC_LAYERS_ON
