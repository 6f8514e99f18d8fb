// ode_h3w_eval.inc -- ONE evaluation of the point CNF's ODE function on the 128-point f16x3 geometry (ode_f16x3w.hip's header describes
// it), up to the per-lane partial sums of the 512 -> 3 output layer: the gate tables of time t, the input layer, hidden layer 1 into the
// hand-managed accumulator file, hidden layer 2 in four passes with its epilogue.  Program TEXT, included inside the stage loop of
// cnf_rk4_h3w_kernel and cnf_dp5_h3w_kernel, not a function: the lambdas below are the including kernel's own, and its compiled code is
// what it was when each kernel carried this text itself (tools/code_object_diff.py).
//   the including file defines, and this file #undefs at its end:
//     XH_STAGE_INPUT   statements behind the table build that leave the stage's input of the lane's point in `float ys[3]` (declaring it,
//                      or assigning one that outlives the stage loop)
//   expects in scope : the switches and XH_STAMP of ode_h3w.h, tid, lane0, t (the evaluation's time, float), `stage` and `step` where
//                      XH_STAMP names them, and what ode_h3w_setup.inc leaves behind
//   leaves behind    : lane, hq, lane16, part[3] (this lane's share of the output layer's three sums: lanes l and l + 32 hold disjoint
//                      rows of the same point), xmax raised to the largest X split; the NEXT evaluation's first seven pieces in flight
int lane = lane0;
asm volatile("" : "+v"(lane));     // opaque: nothing derived from the lane id is hoisted out of the stage loop
const int hq = (lane >> 5) * 4, lane16 = lane * 16;
// layer 1 accumulates from zero (issued before the barrier: overlaps the other waves' arrival)
XH_STAMP(0)
xw_for<0, 256>([&](auto N) XW_INL { xw_acc_zero<decltype(N)::value>(); });
__syncthreads();   // the previous stage's epilogues are done with the tables
// (RK4 stages 1 and 2 both sit at t + h / 2 and build the same tables; skipping the second build and its barrier was measured and
// is not worth a branch here: the launch is as fast with it, DESIGN.md 3)
#pragma unroll
for (int u = 0; u < 2; ++u) {
    const int i = tid + 256 * u;
    const float g0 = sigmoid_fast(fmaf(t, kc_tg[u][0], kc_g[u][0]));
    s_hb0[i] = fmaf(kc_b[u][0], g0, fmaf(t, kc_tb[u][0], kc_hb[u][0])) * act;
    s_w0g[i] = s_w0[3 * i] * g0 * act;
    s_w0g[XC_H + i] = s_w0[3 * i + 1] * g0 * act;
    s_w0g[2 * XC_H + i] = s_w0[3 * i + 2] * g0 * act;
    const float g1 = sigmoid_fast(fmaf(t, kc_tg[u][1], kc_g[u][1]));
    s_g1[i] = g1 * un1;
    s_hb1[i] = fmaf(kc_b[u][1], g1, fmaf(t, kc_tb[u][1], kc_hb[u][1])) * act;
    const float g2 = sigmoid_fast(fmaf(t, kc_tg[u][2], kc_g[u][2]));
    s_g2[i] = g2 * un2;
    s_hb2[i] = fmaf(kc_b[u][2], g2, fmaf(t, kc_tb[u][2], kc_hb[u][2]));
}
if (tid < 3) {
    const float gt = sigmoid_fast(fmaf(t, k3_tg, k3_g));
    s_g3[tid] = gt;
    s_g3[4 + tid] = fmaf(k3_b, gt, fmaf(t, k3_tb, k3_hb));
}
__syncthreads();
XH_STAMP(1)

XH_STAGE_INPUT

// barrier in front of the next sequence piece (placed in the last region of a piece): this wave's share of it has
// landed once at most the 24 DMA instructions of the six younger pieces are outstanding; lgkmcnt: this wave's
// reads of the ring slot that the DMA issued in the next piece refills
auto piece_head = [&]() XW_INL {
    asm volatile("s_waitcnt vmcnt(24) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
};
// one scheduling slot per MFMA: MFMA i of a region multiplies term i >> 1 (smallest first: a2 b1, a1 b2, a1 b1) into
// row tile i & 1 of the pair; slots 0-3 also read the four fragments of the NEXT region, `fill` adds the slot's
// producer micro-steps.  The MFMA goes first, fenced (see ode_bf16x6w.hip)
constexpr int TA[3] = {1, 0, 0}, TB[3] = {0, 1, 0};
auto region_a = [&](auto T0C, const f16x8 (&fc)[2][2], const u32x4 (&b)[2], f16x8 (&fn)[2][2], const unsigned char *An_, auto &&fill) XW_INL {
    constexpr int T0 = decltype(T0C)::value;
    const f16x8 bb[2] = {__builtin_bit_cast(f16x8, b[0]), __builtin_bit_cast(f16x8, b[1])};
    xw_for<0, 6>([&](auto I) XW_INL {
        constexpr int i = decltype(I)::value;
        xh_mfma_a<T0 + (i & 1), (i < 2)>(fc[i & 1][TA[i >> 1]], bb[TB[i >> 1]]);
        XW_FENCE;
        if constexpr (i < 4) fn[i >> 1][i & 1] = *(const f16x8 *)(An_ + i * XH_FRAG);
        fill(I);
        XW_FENCE;
    });
};
// ... the last region of a piece: the next piece's barrier after the first two MFMAs, its first fragments after it
auto region_a_last = [&](auto T0C, const f16x8 (&fc)[2][2], const u32x4 (&b)[2], f16x8 (&fn)[2][2], const unsigned char *An_, auto &&fill) XW_INL {
    constexpr int T0 = decltype(T0C)::value;
    const f16x8 bb[2] = {__builtin_bit_cast(f16x8, b[0]), __builtin_bit_cast(f16x8, b[1])};
    xw_for<0, 6>([&](auto I) XW_INL {
        constexpr int i = decltype(I)::value;
        if constexpr (i == 2) {
            piece_head();
            XW_FENCE;
        }
        xh_mfma_a<T0 + (i & 1), (i < 2)>(fc[i & 1][TA[i >> 1]], bb[TB[i >> 1]]);
        XW_FENCE;
        if constexpr (i >= 2) fn[(i - 2) >> 1][(i - 2) & 1] = *(const f16x8 *)(An_ + (i - 2) * XH_FRAG);
        fill(I);
        XW_FENCE;
    });
};
// layer 2: row tiles c0, c1 in hipcc's registers
auto region_v = [&](f32x16 &c0, f32x16 &c1, const f16x8 (&fc)[2][2], const u32x4 (&b)[2], f16x8 (&fn)[2][2], const unsigned char *An_, auto &&fill) XW_INL {
    const f16x8 bb[2] = {__builtin_bit_cast(f16x8, b[0]), __builtin_bit_cast(f16x8, b[1])};
    xw_for<0, 6>([&](auto I) XW_INL {
        constexpr int i = decltype(I)::value;
        if constexpr ((i & 1) == 0) c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fc[0][TA[i >> 1]], bb[TB[i >> 1]], c0, 0, 0, 0);
        else c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fc[1][TA[i >> 1]], bb[TB[i >> 1]], c1, 0, 0, 0);
        XW_FENCE;
        if constexpr (i < 4) fn[i >> 1][i & 1] = *(const f16x8 *)(An_ + i * XH_FRAG);
        fill(I);
        XW_FENCE;
    });
};
auto region_v_last = [&](f32x16 &c0, f32x16 &c1, const f16x8 (&fc)[2][2], const u32x4 (&b)[2], f16x8 (&fn)[2][2], const unsigned char *An_, auto &&fill) XW_INL {
    const f16x8 bb[2] = {__builtin_bit_cast(f16x8, b[0]), __builtin_bit_cast(f16x8, b[1])};
    xw_for<0, 6>([&](auto I) XW_INL {
        constexpr int i = decltype(I)::value;
        if constexpr (i == 2) {
            piece_head();
            XW_FENCE;
        }
        if constexpr ((i & 1) == 0) c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fc[0][TA[i >> 1]], bb[TB[i >> 1]], c0, 0, 0, 0);
        else c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fc[1][TA[i >> 1]], bb[TB[i >> 1]], c1, 0, 0, 0);
        XW_FENCE;
        if constexpr (i >= 2) fn[(i - 2) >> 1][(i - 2) & 1] = *(const f16x8 *)(An_ + (i - 2) * XH_FRAG);
        fill(I);
        XW_FENCE;
    });
};

// ================= layer 1: 16 chunks x 4 row quarters, sequence pieces 0..63 =================
// B fragment of k-step t (T = t >> 1, u = t & 1), lane (j, h): slot s <-> unit 32 T + 16 u + (s & 3) + 8 (s >> 2) + 4 h:
// group 0 (slots 0-3, words 0, 1) = four consecutive units from ub = 16 t + 4 h, group 1 (words 2, 3) from ub + 8
f32x4 tin[4];         // input-layer tables of the group being produced: hb0, w0g x / y / z (all x 16)
XwPair pa, pb;
auto l1_tab = [&](int ub) XW_INL {
    tin[0] = ld4(s_hb0 + ub);
    tin[1] = ld4(s_w0g + ub);
    tin[2] = ld4(s_w0g + XC_H + ub);
    tin[3] = ld4(s_w0g + 2 * XC_H + ub);
};
auto l1_pre = [&](XwPair &p, int pr) XW_INL {      // units 2 pr, 2 pr + 1 of the group
    p.x0 = fmaf(tin[1][2 * pr], ys[0], fmaf(tin[2][2 * pr], ys[1], fmaf(tin[3][2 * pr], ys[2], tin[0][2 * pr])));
    p.x1 = fmaf(tin[1][2 * pr + 1], ys[0], fmaf(tin[2][2 * pr + 1], ys[1], fmaf(tin[3][2 * pr + 1], ys[2], tin[0][2 * pr + 1])));
};
// the six micro-steps of pair pr of a group, one per slot of a region
auto l1_pair_step = [&](auto I, u32x4 (&bw)[2], int grp, int pr) XW_INL {
    constexpr int i = decltype(I)::value;
    if constexpr (i == 0) l1_pre(pa, pr);
    if constexpr (i == 1) xh_sp1(pa);
    if constexpr (i == 2) xw_sp2(pa);
    if constexpr (i == 3) xh_sp3(pa, xmax);
    if constexpr (i == 4) xh_split1(pa, ones);
    if constexpr (i == 5) xh_split2(pa, bw, 2 * grp + pr, ones);
};
// chunk 0 of the input layer up front (exposed: 1/16 of the input layer)
#pragma unroll
for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int grp = 0; grp < 2; ++grp) {
        l1_tab(16 * ks + 8 * grp + hq);
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            l1_pre(pa, pr);
            xh_sp1(pa);
            xw_sp2(pa);
            xh_sp3(pa, xmax);
            xh_split1(pa, ones);
            xh_split2(pa, b1w[0][ks], 2 * grp + pr, ones);
        }
    }
XW_FENCE;
XH_STAMP(2)
#pragma unroll 1
for (int it = 0; it < 8; ++it) {
    xw_for<0, 8>([&](auto PC) XW_INL {
        constexpr int pc = decltype(PC)::value, par = pc >> 2, rq = pc & 3;   // chunk kc = 2 it + par, ring slot = pc
        const int s1 = 8 * it + pc;                                            // sequence piece
        const unsigned char *A = wbuf + pc * XH_PIECE + lane16;
        const unsigned char *An = wbuf + ((pc + 1) & (XH_RING - 1)) * XH_PIECE + lane16;
        // producers of chunk kc + 1 (B set par ^ 1): piece rq makes group (ks = rq >> 1, grp = rq & 1): tables in
        // region 0, one pair in regions 1 and 2 each.  (Chunk 16 does not exist: the last pass produces chunk 0 once
        // more -- values the range guard has already seen -- into a B set nobody multiplies.  Skipping it takes a uniform
        // branch in each of the 13 producer slots of pieces 4-7: hipcc turns those into more instructions in the seven
        // passes that produce than the eighth saves, DESIGN.md 3.)
        const int ubn = 32 * ((2 * it + par + 1) & 15) + 16 * (rq >> 1) + 8 * (rq & 1) + hq;
        u32x4 (&bn)[2] = b1w[par ^ 1][rq >> 1];
        const unsigned char *dsrc = nullptr;     // this wave's share of piece s1 + 7 in the pack (dma_open)
        auto dma = [&](auto I0) XW_INL {
            if constexpr (XH_OLD_DMA) dma1(s1 + 7, lane16, decltype(I0)::value);
            else dma_kb(dsrc, lane16, I0);
        };
        // region 0: k-step 0, row tiles 0, 1 (fX) | reads k-step 0, row tiles 2, 3 -> fY
        region_a(std::integral_constant<int, 4 * rq>{}, fX, b1w[par][0], fY, A + 4 * XH_FRAG, [&](auto I) XW_INL {
            constexpr int i = decltype(I)::value;
            if constexpr (i == 0) l1_tab(ubn);
            if constexpr (i == 3 && !XH_OLD_DMA) dsrc = dma_open(s1 + 7);
            if constexpr (i == 4) dma(std::integral_constant<int, 0>{});
        });
        // region 1: k-step 0, row tiles 2, 3 (fY) | reads k-step 1, row tiles 0, 1 -> fX
        region_a(std::integral_constant<int, 4 * rq + 2>{}, fY, b1w[par][0], fX, A + 8 * XH_FRAG, [&](auto I) XW_INL {
            constexpr int i = decltype(I)::value;
            l1_pair_step(I, bn, rq & 1, 0);
            if constexpr (i == 3) dma(std::integral_constant<int, 1>{});
        });
        // region 2: k-step 1, row tiles 0, 1 (fX) | reads k-step 1, row tiles 2, 3 -> fY
        region_a(std::integral_constant<int, 4 * rq>{}, fX, b1w[par][1], fY, A + 12 * XH_FRAG, [&](auto I) XW_INL {
            constexpr int i = decltype(I)::value;
            l1_pair_step(I, bn, rq & 1, 1);
            if constexpr (i == 3) dma(std::integral_constant<int, 2>{});
        });
        // region 3: the last kilobyte of piece s1 + 7 | barrier of the next piece | k-step 1, row tiles 2, 3 (fY) | reads
        // the next piece's k-step 0, row tiles 0, 1 -> fX
        region_a_last(std::integral_constant<int, 4 * rq + 2>{}, fY, b1w[par][1], fX, An, [&](auto I) XW_INL {
            constexpr int i = decltype(I)::value;
            if constexpr (i == 1) dma(std::integral_constant<int, 3>{});
        });
    });
}
XH_STAMP(3)

// ================= layer 2: four passes of 16 pieces, sequence pieces 64 + 16 q + kc =================
float part[3] = {0.f, 0.f, 0.f};
f32x4 tt[2][2];       // gate1 / hb1 of a group, [region parity][gate | bias], read one region ahead
float qv[4];
auto l2_tab = [&](int set, int t_, int grp) XW_INL {
    const int c = 16 * t_ + 8 * grp + hq;
    tt[set][0] = ld4(s_g1 + c);
    tt[set][1] = ld4(s_hb1 + c);
};
// Producer of group GRP of k-step T_ (registers a[16 (T_ >> 1) + 8 (T_ & 1) + 4 GRP + r], r = 0..3), by slot.  FIRST
// pass: gate / bias / softplus / split, and the group's four plane words (p1, p2 of pair a, p1, p2 of pair b: two f16
// planes of a value pair are exactly two 32-bit words) take the place of the four sums in the accumulator file; later
// passes: four reads straight into the B planes, no arithmetic (the range guard has seen every X in pass 0).
auto l2_step = [&](auto I, auto TC, auto GC, auto FC, u32x4 (&bw)[2], int set) XW_INL {
    constexpr int i = decltype(I)::value, t_ = decltype(TC)::value, grp = decltype(GC)::value;
    constexpr bool first = decltype(FC)::value;
    constexpr int base = 16 * (t_ >> 1) + 8 * (t_ & 1) + 4 * grp;
    if constexpr (first) {
        if constexpr (i == 0) {
            qv[0] = xw_acc_rd<base>();
            qv[1] = xw_acc_rd<base + 1>();
            qv[2] = xw_acc_rd<base + 2>();
            qv[3] = xw_acc_rd<base + 3>();
            pa.x0 = fmaf(qv[0], tt[set][0][0], tt[set][1][0]);
            pa.x1 = fmaf(qv[1], tt[set][0][1], tt[set][1][1]);
            pb.x0 = fmaf(qv[2], tt[set][0][2], tt[set][1][2]);
            pb.x1 = fmaf(qv[3], tt[set][0][3], tt[set][1][3]);
        }
        if constexpr (i == 1) {
            xh_sp1(pa);
            xh_sp1(pb);
        }
        if constexpr (i == 2) {
            xw_sp2(pa);
            xw_sp2(pb);
        }
        if constexpr (i == 3) {
            xh_sp3(pa, xmax);
            xh_sp3(pb, xmax);
        }
        if constexpr (i == 4) {
            xh_split1(pa, ones);
            xh_split1(pb, ones);
        }
        if constexpr (i == 5) {
            xh_split2(pa, bw, 2 * grp, ones);
            xh_split2(pb, bw, 2 * grp + 1, ones);
            xh_acc_wr_u<base>(bw[0][2 * grp]);
            xh_acc_wr_u<base + 1>(bw[1][2 * grp]);
            xh_acc_wr_u<base + 2>(bw[0][2 * grp + 1]);
            xh_acc_wr_u<base + 3>(bw[1][2 * grp + 1]);
        }
    } else {
        if constexpr (i == 0) {
            bw[0][2 * grp] = xh_acc_rd_u<base>();
            bw[1][2 * grp] = xh_acc_rd_u<base + 1>();
            bw[0][2 * grp + 1] = xh_acc_rd_u<base + 2>();
            bw[1][2 * grp + 1] = xh_acc_rd_u<base + 3>();
        }
    }
};
auto pass = [&](int q, auto FC) XW_INL {
    constexpr bool first = decltype(FC)::value;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[mi][r] = 0.f;
    // k-step 0 of this pass up front (exposed); the tables of (k-step 1, group 0) for region 0
    if constexpr (first) {
        l2_tab(0, 0, 0);
        l2_tab(1, 0, 1);
    }
    xw_for<0, 6>([&](auto I) XW_INL { l2_step(I, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, FC, b2w[0], 0); });
    xw_for<0, 6>([&](auto I) XW_INL { l2_step(I, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{}, FC, b2w[0], 1); });
    if constexpr (first) l2_tab(0, 1, 0);
    // passes 1-3: the plane words go from the accumulator read straight into hipcc's first MFMA, which does not see a
    // VALU write in the asm statement and pads nothing: the two wait states by hand
    else asm volatile("s_nop 1");
    XW_FENCE;
    xw_for<0, 16>([&](auto KC) XW_INL {
        constexpr int kc = decltype(KC)::value;
        const int sq = 64 + 16 * q + kc;
        const unsigned char *A = wbuf + (kc & (XH_RING - 1)) * XH_PIECE + lane16;            // sq & 7 == kc & 7
        const unsigned char *An = wbuf + ((kc + 1) & (XH_RING - 1)) * XH_PIECE + lane16;
        constexpr int tb = 2 * kc + 1, tn = (kc < 15 ? 2 * kc + 2 : 0);
        const unsigned char *dsrc = nullptr;     // this wave's share of piece sq + 7 in the pack (dma_open)
        auto dma = [&](auto I0) XW_INL {
            if constexpr (XH_OLD_DMA) dma1(sq + 7, lane16, decltype(I0)::value);
            else dma_kb(dsrc, lane16, I0);
        };
        // k-step t + 1 is produced during k-step t: group 0 in the region of row tiles 0, 1 (tables in tt[0]), group 1 in
        // the region of row tiles 2, 3 (tt[1]); slot 3 of a region reads the tables of the next region's group
        // region 0: k-step 2 kc, row tiles 0, 1 (fX) | reads row tiles 2, 3 -> fY | group 0 of k-step tb
        region_v(acc2[0], acc2[1], fX, b2w[0], fY, A + 4 * XH_FRAG, [&](auto I) XW_INL {
            constexpr int i = decltype(I)::value;
            l2_step(I, std::integral_constant<int, tb>{}, std::integral_constant<int, 0>{}, FC, b2w[1], 0);
            if constexpr (first && i == 3) l2_tab(1, tb, 1);
            if constexpr (i == 3 && !XH_OLD_DMA) dsrc = dma_open(sq + 7);
            if constexpr (i == 4) dma(std::integral_constant<int, 0>{});
        });
        // region 1: k-step 2 kc, row tiles 2, 3 (fY) | reads tb, row tiles 0, 1 -> fX | group 1 of tb
        region_v(acc2[2], acc2[3], fY, b2w[0], fX, A + 8 * XH_FRAG, [&](auto I) XW_INL {
            constexpr int i = decltype(I)::value;
            l2_step(I, std::integral_constant<int, tb>{}, std::integral_constant<int, 1>{}, FC, b2w[1], 1);
            if constexpr (first && kc < 15 && i == 3) l2_tab(0, tn, 0);
            if constexpr (i == 4) dma(std::integral_constant<int, 1>{});
        });
        // region 2: k-step tb, row tiles 0, 1 (fX) | reads tb, row tiles 2, 3 -> fY | group 0 of k-step tb + 1
        region_v(acc2[0], acc2[1], fX, b2w[1], fY, A + 12 * XH_FRAG, [&](auto I) XW_INL {
            constexpr int i = decltype(I)::value;
            if constexpr (kc < 15) l2_step(I, std::integral_constant<int, tn>{}, std::integral_constant<int, 0>{}, FC, b2w[0], 0);
            if constexpr (first && kc < 15 && i == 3) l2_tab(1, tn, 1);
            if constexpr (i == 4) dma(std::integral_constant<int, 2>{});
        });
        // region 3: the last kilobyte of piece sq + 7 | barrier of the next piece | k-step tb, row tiles 2, 3 (fY) | reads
        // the next piece's first fragments -> fX | group 1 of k-step tb + 1
        region_v_last(acc2[2], acc2[3], fY, b2w[1], fX, An, [&](auto I) XW_INL {
            constexpr int i = decltype(I)::value;
            if constexpr (kc < 15) l2_step(I, std::integral_constant<int, tn>{}, std::integral_constant<int, 1>{}, FC, b2w[0], 1);
            if constexpr (first && kc < 15 && i == 3) l2_tab(0, tn + 1, 0);
            if constexpr (i == 1) dma(std::integral_constant<int, 3>{});
        });
    });
    XH_STAMP(4 + 2 * q)
    // ---- epilogue of hidden layer 2 for rows 128 q .. 128 q + 127 + their share of the 512 -> 3 output layer:
    // acc2[rt] register r <-> unit 128 q + 32 rt + 8 (r >> 2) + 4 h + (r & 3); s_g2 carries the unscale 2^-(4 + s2)
    int le = lane;   // opaque again: the table addresses must not be hoisted above the product loop
    asm volatile("" : "+v"(le));
    const int cq = 128 * q + (le >> 5) * 4;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int c = cq + 32 * rt + 8 * rr;
            const f32x4 gt = ld4(s_g2 + c), hb = ld4(s_hb2 + c);
            const f32x4 wx3 = ld4(s_w3 + c), wy3 = ld4(s_w3 + XC_H + c), wz3 = ld4(s_w3 + 2 * XC_H + c);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float hv = softplus_fast(fmaf(acc2[rt][4 * rr + r], gt[r], hb[r]));
                part[0] = fmaf(wx3[r], hv, part[0]);
                part[1] = fmaf(wy3[r], hv, part[1]);
                part[2] = fmaf(wz3[r], hv, part[2]);
            }
        }
    XW_FENCE;
    XH_STAMP(5 + 2 * q)
};
int q0 = 0;
asm volatile("" : "+s"(q0));     // opaque: the piece addresses of pass 0 are computed like those of passes 1-3 (SALU)
pass(q0, std::true_type{});
#pragma unroll 1
for (int q = 1; q < 4; ++q) pass(q, std::false_type{});
#undef XH_STAGE_INPUT
