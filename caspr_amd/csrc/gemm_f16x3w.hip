// gemm_f16x3w.hip -- the 128-point x 512-channel pointwise conv of gemm_bf16x6w.hip on THREE f16 products per f32 product
// (config.conv_split = "f16x3"): the same geometry (a wave owns 128 channels x all 128 points of the tile, 256 accumulators in the
// hand-managed accumulator file, weights straight from global memory in fragment order, split activation of the running 32-k chunk
// in LDS, persistent channel-tile-major stream of k-chunks, statistics epilogue) with half the matrix-pipe instructions.  The body is
// a copy of that kernel's on purpose (as ode_f16x3w.hip's is of ode_bf16x6w.hip); read its header first, this one lists the
// differences.
//
//  * the scheme (tests/conv_f16x3_ref.py restates it, tests/f16x3_ref.py is the split's contract): the activation after the
//    producer's GroupNorm / ReLU is multiplied by 2^4, the layer's weights by the power of two 2^s that puts max |W| in [2^14, 2^15)
//    (found ON THE DEVICE at pack time, stored behind the pack and read here once per workgroup); each is split into two f16 planes
//    by round-to-nearest (p1 = rne16(x), p2 = rne16(x - p1)); w . x ~ w2 x1 + w1 x2 + w1 x1 on v_mfma_f32_32x32x16_f16, smallest
//    terms first; the read-out multiplies an accumulator by 2^-(4 + s), exactly, before bias / per-batch bias.  Statistics are taken
//    from the unscaled values, as in the parent;
//  * conv inputs are SIGNED (the channels in front of in_relu_from, the plain form): the split flushes by magnitude.  Plane values
//    below 2^-14 are flushed to zero explicitly; nothing depends on the pipe's subnormal handling;
//  * range guard: a value that is not below 65520 in magnitude after the 2^4 scale (a NaN or an infinity included) is replaced by
//    NaN before the split: its hi-plane word is an f16 NaN, its lo-plane word zero, and all 512 outputs of that row in this tile
//    come out NaN through the MFMA -- never a silently wrong number.  A lane keeps the maximum magnitude (as bits) of what it splits;
//    at the end of the kernel one lane per wave that saw such a value sets the launch's status word with atomicOr.  The GroupNorm
//    statistics of a batch entry that contains such a row are NaN;
//  * weight pack [channel tile][k-step][wave 4][row tile 4][plane 2][fragment]: 8 fragment loads per wave and k-step (12 before);
//  * LDS: [k-step 2][column tile 4][plane 2][fragment] = 16 KB per chunk buffer, two buffers + the statistics region = 40 KB.
//
// The schedule, re-derived: a chunk is 96 MFMAs = 16 regions (k-step, column-tile pair, row tile) of 6 slots, R0..R15, and lasts
// 3072 matrix-pipe cycles -- half the parent's.  Everything that comes from memory is therefore asked for earlier, counted in regions:
//  * raw activation rows: TWO chunks ahead without a third register set.  The 16 values of a thread's row live in four quads; the
//    quad of pairs (2q, 2q + 1) of the chunk being staged (c1) is free once its second pair is transformed (R4 + 2q, slot 0) and is
//    reloaded in the next slot with the same quad of chunk c3: 31 regions (5952 cycles, the parent's 6144) before it is consumed;
//  * weights: fragment pair (set, row tile) is reloaded in the region after its last use -- set 0 (k-step 0) of row tile rt in
//    R5 + rt with the next chunk's, set 1 in R13 + rt (row tile 3: R0 of the next chunk) -- 11 regions = 2112 cycles ahead of its
//    next use (the parent: 8 regions of 12 = 3072);
//  * staging of chunk c1: scale / shift loads in R0 slot 5; pair g in R3 + g: transform + guard in slot 0, first plane in slot 2,
//    second plane in slot 4; the two plane writes of half 0 in R7 slots 1 / 3, of half 1 in R11 slots 1 / 3; barrier in front of R12;
//  * fragment reads (4 per column-tile pair): slots 0-3 of R0 (k-step 0, pair 1), R6 (k-step 1, pair 0), R8 (k-step 1, pair 1) and,
//    behind the barrier, R12 (next chunk, k-step 0, pair 0).
// Contract: Cin % 32 == 0, P % 128 == 0, Cout % 512 == 0 per launch (the remainder of the channels stays on the bf16x6 kernels).
#include "f16x3_common.h"

// XW_EXP (debug flavours, build.py CASPR_XW_EXP): timing experiments, WRONG results: 2048 no weight loads inside the K loop,
// 4096 no activation staging inside the K loop, 8192 no epilogue
#ifndef XW_EXP
#define XW_EXP 0
#endif
#define CH_TP 128
#define CH_TM 512
#define CH_FRAG 1024
#define CH_BCHUNK (2 * 4 * 2 * CH_FRAG)     // split activation of one 32-k chunk: [k-step 2][column tile 4][plane 2][fragment]
#define CH_SPART (2 * CH_BCHUNK)            // STATS: [512 channels] {mean, M2, max, min} of the tile being finished: a region of its own
#define CH_LDS (2 * CH_BCHUNK + CH_TM * 16)
#define CH_LIMIT_BITS 0x477ff000u           // the bits of 65520.0f: |x| as bits >= this <-> not finite in f16 (NaN and infinity included)

struct ConvHArgs {
    const unsigned char *wpk, *wtail;
    const float *bias, *bbias, *X;
    float *Y;
    f32x4 *part;
    unsigned *status;
    int ldx, ldy, P, Cin, Cout, in_relu, relu_from, Mt, Pt, part_stride, bb_stride, ntiles, mt0;
};

// One chunk of the flattened (tile, k-chunk) sequence a workgroup walks through: everything here is wave-uniform (SGPRs).
struct ChChunk {
    int lin;                      // tile id (channel-tile-major over the whole problem)
    int kc;                       // 32-k chunk inside the tile
    int mt, b, pt;                // its channel tile, batch entry, point tile
};

template <bool FUSED, bool STATS>
__global__ __launch_bounds__(256, 1) void conv1x1_h3w_kernel(ConvHArgs a, const float *__restrict__ in_scale, const float *__restrict__ in_shift)
{
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    const int tid = threadIdx.x, lane0 = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // tile order and the stream of chunks: as conv1x1_x6w_kernel
    const int G = gridDim.x;
    const int npt = a.ntiles / a.Mt;                  // point tiles over all batch entries
    const int nk = a.Cin / 32;
    const int nmine = (a.ntiles - (int)blockIdx.x + G - 1) / G;
    const int total = nmine * nk;                     // chunks of this workgroup
    const int lin_last = blockIdx.x + (nmine - 1) * G;
    // the scale the pack step chose: W 2^s is what the planes hold
    const float un = ldexpf(1.0f, -(XH_ACT_SHIFT + *(const int *)a.wtail));
    const float act = (float)(1 << XH_ACT_SHIFT);

    auto decode = [&](ChChunk &c) XW_INL {
        const int mtl = c.lin / npt;
        const int gpt = c.lin - mtl * npt;
        c.mt = a.mt0 + mtl;                 // a launch may cover a RANGE of channel tiles (mt0 .. mt0 + Mt - 1)
        c.b = gpt / a.Pt;
        c.pt = gpt - c.b * a.Pt;
    };
    // the chunk after c in this workgroup's stream; past the end it stays on the last chunk (whatever is loaded / staged for it
    // again is harmless and never consumed)
    auto advance = [&](ChChunk &c) XW_INL {
        if (c.kc + 1 < nk) {
            c.kc += 1;
        } else if (c.lin != lin_last) {
            c.kc = 0;
            c.lin += G;
            decode(c);
        }
    };

    // activation staging: thread = (row xr of the tile, k-step xh of the chunk: 16 consecutive k); xh is wave-uniform
    const int xr = tid & 127, xh = wave >> 1;
    const unsigned xoff = (unsigned)xr * (unsigned)a.ldx + 16u * xh;                  // floats, inside the tile's 128 rows
    float scv[16], shv[16];       // the scale / shift of the thread's 16 channels of the chunk being staged (SGPRs: wave-uniform)
    const unsigned wdst = ((xh * 4 + (xr >> 5)) * 2) * CH_FRAG + (xr & 31) * 16;     // + plane * CH_FRAG + half * 512
    // weights: [channel tile][k-step][wave][row tile 4][plane 2][fragment]: 8 KB per wave and k-step
    const long wstep = 4L * 8 * CH_FRAG;

    f16x8 afr[2][4][2];           // weight fragments [k-step parity][row tile][plane]
    f16x8 bfr[2][2][2];           // activation fragments [column-tile pair][tile of the pair][plane]
    f32x4 xra[4], xrb[4];         // 16 raw values of the thread's row: one set holds the chunk being staged / the one three ahead, quad by quad
    u32x4 pv[2][2];               // their two planes [half of the k-step][plane]
    XwPair sp;
    unsigned xm = 0;              // range guard: the largest |value| (as bits) this lane has split

    auto aload = [&](const ChChunk &c, int ks, auto SETC, auto RTC) XW_INL {        // the two planes of row tile RT of k-step ks of chunk c -> set SET
        constexpr int set = decltype(SETC)::value, rt = decltype(RTC)::value;
        if constexpr ((XW_EXP & 2048) != 0) return;
        const unsigned char *p = a.wpk + ((long)c.mt * (2 * nk) * 4 + wave) * (8 * CH_FRAG) + (long)(2 * c.kc + ks) * wstep + rt * 2 * CH_FRAG + lane0 * 16;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) afr[set][rt][pl] = *(const f16x8 *)(p + pl * CH_FRAG);
    };
    auto gload1 = [&](f32x4 (&xv)[4], const ChChunk &c, auto QC) XW_INL {             // quad Q of the thread's row of chunk c
        constexpr int q = decltype(QC)::value;
        const float *base = a.X + ((long)c.b * a.P + c.pt * CH_TP) * a.ldx + c.kc * 32;      // wave-uniform
        xv[q] = ld4(base + xoff + 4 * q);
    };
    auto sload = [&](const ChChunk &c) XW_INL {
        if constexpr (FUSED) {
            const float *sc = in_scale + (long)c.b * a.Cin + 16 * xh + c.kc * 32, *sh = in_shift + (long)c.b * a.Cin + 16 * xh + c.kc * 32;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                scv[q] = sc[q];
                shv[q] = sh[q];
            }
        }
    };
    // pair m (values 2m, 2m + 1 of the thread's 16) of chunk kc: producer transform, 2^4, range guard; then the split micro-steps
    auto st_pre = [&](const f32x4 (&xv)[4], int kc, auto MC) XW_INL {
        constexpr int m = decltype(MC)::value;
        float v0 = xv[m >> 1][(2 * m) & 3], v1 = xv[m >> 1][(2 * m + 1) & 3];
        if constexpr (FUSED) {
            // the ReLU switches on at a multiple of 8 channels (checked by the host)
            const float lo = (a.in_relu && kc * 32 + 16 * xh + 2 * m >= a.relu_from) ? 0.f : -INFINITY;
            v0 = fmaxf(fmaf(v0, scv[2 * m], shv[2 * m]), lo);
            v1 = fmaxf(fmaf(v1, scv[2 * m + 1], shv[2 * m + 1]), lo);
        }
        v0 *= act;                // exact: 16 x the parent kernel's operand
        v1 *= act;
        const unsigned b0 = __float_as_uint(v0) & 0x7fffffffu, b1 = __float_as_uint(v1) & 0x7fffffffu;
        xm = max(xm, max(b0, b1));
        sp.x0 = b0 >= CH_LIMIT_BITS ? __uint_as_float(0x7fc00000u) : v0;
        sp.x1 = b1 >= CH_LIMIT_BITS ? __uint_as_float(0x7fc00000u) : v1;
    };
    auto st_split1 = [&]() XW_INL {          // first plane (flushed by magnitude) + remainder; a NaN stays a NaN
        const float a0 = fabsf(sp.x0) < XH_FLUSH ? 0.0f : sp.x0, a1 = fabsf(sp.x1) < XH_FLUSH ? 0.0f : sp.x1;
        sp.p1 = xh_cvt_pk(a0, a1);
        const xh_f16x2 hv = __builtin_bit_cast(xh_f16x2, sp.p1);
        sp.r0 = a0 - (float)hv[0];
        sp.r1 = a1 - (float)hv[1];
    };
    auto st_split2 = [&](auto MC) XW_INL {   // second plane: a remainder that is not at least 2^-14 (a NaN's included) is zero
        constexpr int m = decltype(MC)::value;
        const float r0 = fabsf(sp.r0) >= XH_FLUSH ? sp.r0 : 0.0f, r1 = fabsf(sp.r1) >= XH_FLUSH ? sp.r1 : 0.0f;
        pv[m >> 2][0][m & 3] = sp.p1;
        pv[m >> 2][1][m & 3] = xh_cvt_pk(r0, r1);
    };
    auto st_write = [&](int buf, auto HC, auto PC) XW_INL {
        constexpr int hf = decltype(HC)::value, pl = decltype(PC)::value;
        *(u32x4 *)(lds + buf * CH_BCHUNK + wdst + pl * CH_FRAG + hf * 512) = pv[hf][pl];
    };
    // fragment read: tile i >> 1 of the pair CTP of k-step ks of the chunk in buffer buf, plane i & 1
    auto bread = [&](int buf, int ks, auto CTPC, auto IC) XW_INL {
        constexpr int ctp = decltype(CTPC)::value, i = decltype(IC)::value;
        bfr[ctp][i >> 1][i & 1] = *(const f16x8 *)(lds + buf * CH_BCHUNK + ((ks * 4 + 2 * ctp + (i >> 1)) * 2 + (i & 1)) * CH_FRAG + lane0 * 16);
    };

    // ---- the stream's live positions: the chunk being multiplied, the next one (staged under it), ..., the one three ahead (loaded under it)
    ChChunk c0, c1, c2, c3;
    c0.lin = blockIdx.x;
    c0.kc = 0;
    decode(c0);
    c1 = c0;
    advance(c1);
    c2 = c1;
    advance(c2);
    c3 = c2;
    advance(c3);

    xw_for<0, 256>([&](auto N) XW_INL { xw_acc_zero<decltype(N)::value>(); });
    // ---- prologue (once per workgroup): both weight sets of chunk 0, chunk 0 staged (exposed), its first fragments; chunk 1 -> xrb,
    // chunk 2 -> xra behind the staging of chunk 0
    xw_for<0, 4>([&](auto RT) XW_INL {
        aload(c0, 0, std::integral_constant<int, 0>{}, RT);
        aload(c0, 1, std::integral_constant<int, 1>{}, RT);
    });
    xw_for<0, 4>([&](auto Q) XW_INL { gload1(xra, c0, Q); });
    sload(c0);
    xw_for<0, 4>([&](auto Q) XW_INL { gload1(xrb, c1, Q); });
    xw_for<0, 8>([&](auto M) XW_INL {
        st_pre(xra, 0, M);
        st_split1();
        st_split2(M);
    });
    XW_FENCE;
    xw_for<0, 4>([&](auto Q) XW_INL { gload1(xra, c2, Q); });
    xw_for<0, 2>([&](auto H) XW_INL { xw_for<0, 2>([&](auto PL) XW_INL { st_write(0, H, PL); }); });
    __syncthreads();
    xw_for<0, 4>([&](auto I) XW_INL { bread(0, 0, std::integral_constant<int, 0>{}, I); });
    XW_FENCE;

    constexpr int TA[3] = {1, 0, 0}, TB[3] = {0, 1, 0};
    // one region = 6 MFMAs on accumulator tiles (RT, 2 CTP), (RT, 2 CTP + 1), one scheduling slot each
    auto region = [&](auto KSC, auto CTPC, auto RTC, auto &&fill) XW_INL {
        constexpr int ks = decltype(KSC)::value, ctp = decltype(CTPC)::value, rt = decltype(RTC)::value;
        xw_for<0, 6>([&](auto I) XW_INL {
            constexpr int i = decltype(I)::value;
            xh_mfma_a<4 * rt + 2 * ctp + (i & 1), (i < 2)>(afr[ks][rt][TA[i >> 1]], bfr[ctp][i & 1][TB[i >> 1]]);
            XW_FENCE;
            fill(I);
            XW_FENCE;
        });
    };

    // one 32-k chunk (c0) in LDS buffer cur: 16 regions; stages chunk c1 from xs into the other buffer and reloads xs, quad by quad,
    // with chunk c3.  c1 / c3 may belong to later tiles of this workgroup.
    auto chunk = [&](int cur, f32x4 (&xs)[4]) XW_INL {
        const int nxt = cur ^ 1;
        // what region R (0..15) does beside its MFMAs, by slot (see the file header)
        auto fill = [&](auto RC, auto I) XW_INL {
            constexpr int R = decltype(RC)::value, i = decltype(I)::value;
            // fragment reads
            if constexpr (R == 0 && i < 4) bread(cur, 0, std::integral_constant<int, 1>{}, I);
            if constexpr (R == 6 && i < 4) bread(cur, 1, std::integral_constant<int, 0>{}, I);
            if constexpr (R == 8 && i < 4) bread(cur, 1, std::integral_constant<int, 1>{}, I);
            if constexpr (R == 12 && i < 4) bread(nxt, 0, std::integral_constant<int, 0>{}, I);
            // weights, in the region after a fragment pair's last use
            if constexpr (R == 0 && i == 4) aload(c0, 1, std::integral_constant<int, 1>{}, std::integral_constant<int, 3>{});
            if constexpr (R >= 5 && R <= 8 && i == 5) aload(c1, 0, std::integral_constant<int, 0>{}, std::integral_constant<int, (R - 5) & 3>{});
            if constexpr (R >= 13 && i == 5) aload(c1, 1, std::integral_constant<int, 1>{}, std::integral_constant<int, (R - 13) & 3>{});
            // staging of chunk c1, reload of its registers with chunk c3
            if constexpr ((XW_EXP & 4096) == 0) {
                if constexpr (R == 0 && i == 5) sload(c1);
                if constexpr (R >= 3 && R <= 10) {
                    constexpr int g = (R - 3) & 7;
                    if constexpr (i == 0) st_pre(xs, c1.kc, std::integral_constant<int, g>{});
                    if constexpr (i == 1 && (g & 1)) gload1(xs, c3, std::integral_constant<int, (g >> 1)>{});
                    if constexpr (i == 2) st_split1();
                    if constexpr (i == 4) st_split2(std::integral_constant<int, g>{});
                }
                if constexpr ((R == 7 || R == 11) && (i == 1 || i == 3)) st_write(nxt, std::integral_constant<int, (R == 11)>{}, std::integral_constant<int, (i >> 1)>{});
            }
        };
        xw_for<0, 16>([&](auto RC) XW_INL {
            constexpr int R = decltype(RC)::value;
            if constexpr (R == 12) {
                // every wave's planes of chunk c1 are written (and this wave is done reading the buffer the chunk after that
                // will overwrite): one barrier per chunk
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                XW_FENCE;
            }
            region(std::integral_constant<int, (R >> 3)>{}, std::integral_constant<int, ((R >> 2) & 1)>{}, std::integral_constant<int, (R & 3)>{},
                   [&](auto I) XW_INL { fill(RC, I); });
        });
    };

    // ---- a tile's read-out: unscale, bias / per-batch bias, store (the stores drain under the next tile's products), statistics,
    // accumulators back to zero.  Everything the stream keeps in flight stays live across it.
    auto finish = [&](const ChChunk &c) XW_INL {
        if constexpr ((XW_EXP & 8192) != 0) return;
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");     // the last MFMAs' results, before the accumulator file is read
        const int lane = lane0, j = lane & 31, hq = (lane >> 5) * 4;
        const int p0 = c.pt * CH_TP;
        const int cw = c.mt * CH_TM + wave * 128;               // first channel of this wave
        f32x4 *spart = (f32x4 *)(lds + CH_SPART);
        xw_for<0, 4>([&](auto RT) XW_INL {
            constexpr int rt = decltype(RT)::value;
            float v[4][16];
            xw_for<0, 4>([&](auto CT) XW_INL {
                constexpr int ct = decltype(CT)::value;
                xw_for<0, 16>([&](auto R) XW_INL {
                    constexpr int r = decltype(R)::value;
                    v[ct][r] = xw_acc_rd<16 * (4 * rt + ct) + r>() * un;
                });
            });
            xw_for<0, 64>([&](auto N) XW_INL { xw_acc_zero<64 * rt + decltype(N)::value>(); });
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int co = cw + 32 * rt + 8 * rr + hq;
                f32x4 add = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (a.bias) add += ld4(a.bias + co);
                if (a.bbias) add += ld4(a.bbias + (long)c.b * a.bb_stride + co);
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[ct][4 * rr + r] += add[r];
                    if (!STATS || a.Y)
                        st4(a.Y + ((long)c.b * a.P + p0 + 32 * ct + j) * a.ldy + co, (f32x4){v[ct][4 * rr], v[ct][4 * rr + 1], v[ct][4 * rr + 2], v[ct][4 * rr + 3]});
                }
            }
            if (STATS) {
                // as conv1x1_x6w_kernel: mean first, then the squared deviations from it, max and min, through the transposing reduction
                float mean[16], q[16], mx[16], mn[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float s = (v[0][r] + v[1][r]) + (v[2][r] + v[3][r]);
                    mx[r] = fmaxf(fmaxf(v[0][r], v[1][r]), fmaxf(v[2][r], v[3][r]));
                    mn[r] = fminf(fminf(v[0][r], v[1][r]), fminf(v[2][r], v[3][r]));
                    s = xw_rows_add(row_allreduce_add<16>(s));
                    mean[r] = s * (1.0f / 128.0f);
                    float qq = 0.f;
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        const float d = v[ct][r] - mean[r];
                        qq = fmaf(d, d, qq);
                    }
                    q[r] = qq;
                }
                float mean2[2], q2[2], mx2[2], mn2[2];
                xw_treduce16(q, q2, XwAdd{});
                xw_treduce16(mx, mx2, XwMax{});
                xw_treduce16(mn, mn2, XwMin{});
                xw_treduce16(mean, mean2, XwFirst{});
                if ((lane & 3) == 0) {
                    const int bk = (lane >> 2) & 3, rho = (lane >> 4) & 1;
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int r = 8 * i + 4 * (bk & 1) + 2 * (bk >> 1) + rho;
                        spart[wave * 128 + 32 * rt + 8 * (r >> 2) + hq + (r & 3)] = (f32x4){mean2[i], q2[i], mx2[i], mn2[i]};
                    }
                }
            }
        });
        if (STATS) {
            // spart is rewritten one whole tile (>= 2 chunk barriers) later: the copy-out below is long done by then
            __syncthreads();
            for (int ch = tid; ch < CH_TM; ch += 256) a.part[((long)c.b * a.Pt + c.pt) * a.part_stride + c.mt * CH_TM + ch] = spart[ch];
        }
    };
    auto step = [&]() XW_INL {        // c0 is done: read its tile out if that was the tile's last chunk, move the positions on
        if (c0.kc == nk - 1) finish(c0);
        c0 = c1;
        c1 = c2;
        c2 = c3;
        advance(c3);
    };
#pragma unroll 1
    for (int g = 0; g < total; g += 2) {
        chunk(0, xrb);
        step();
        if (g + 1 < total) {
            chunk(1, xra);
            step();
        }
    }
    // range guard: one lane of a wave that split a value not finite in f16 reports it
    if (__any(xm >= CH_LIMIT_BITS) && lane0 == 0) atomicOr(a.status, 1u);
}

// ---- pack: (Cout, ldw) f32 [+ column offset / count] -> [channel tile of 512][k-step][wave 4][row tile 4][plane 2][lane 64][8 f16] + tail;
// lane (i = l & 31, h = l >> 5) of fragment (mt, t, w, rt) holds row 512 mt + 128 w + 32 rt + i (zero beyond Cout), k = 16 t + 8 h + s
__global__ void h3w_weight_max_kernel(const float *__restrict__ w, int ldw, int Cout, int col0, int Cin, unsigned *__restrict__ tail)
{
    unsigned m = 0;
    const long n = (long)Cout * Cin;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        m = max(m, __float_as_uint(w[(i / Cin) * ldw + col0 + (i % Cin)]) & 0x7fffffffu);      // |w|: non-negative floats order as their bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0) atomicMax(tail + 1, m);
}
__global__ void pack_weight_h3w_kernel(const float *__restrict__ w, int ldw, int Cout, int col0, int Cin, unsigned char *__restrict__ out, long total,
                                       unsigned *__restrict__ tail)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;   // ((mt * nks + t) * 16 + w * 4 + rt) * 64 + lane
    if (i >= total) return;
    const int sh = h3_shift(tail[1]);
    if (i == 0) ((int *)tail)[0] = sh;
    const int l = (int)(i & 63), wr = (int)((i >> 6) & 15);
    const long mk = i >> 10;
    const int nks = Cin / 16;
    const int t = (int)(mk % nks), mt = (int)(mk / nks);
    const int row = mt * CH_TM + (wr >> 2) * 128 + (wr & 3) * 32 + (l & 31), hh = l >> 5;
    float p1[8], p2[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        float x = row < Cout ? ldexpf(w[(long)row * ldw + col0 + 16 * t + 8 * hh + s], sh) : 0.f;
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
        *(u32x4 *)(out + ((mk * 16 + wr) * 2 + pl) * CH_FRAG + l * 16) = v;
    }
}

static long h3w_plane_bytes(int Cout, int Cin) { return (long)ceil_div(Cout, CH_TM) * (Cin / 16) * 16 * 2 * CH_FRAG; }

extern "C" long caspr_h3w_packed_bytes(int Cout, int Cin)
{
    if (Cout <= 0 || Cin <= 0 || Cin % 32) return 0;
    return h3w_plane_bytes(Cout, Cin) + XH_TAIL;
}

extern "C" int caspr_pack_weight_h3w(const float *w, int ldw, int Cout, int col0, int ncols, void *packed, void *stream)
{
    CASPR_REQUIRE(w && packed && Cout > 0 && ncols > 0 && ncols % 32 == 0 && col0 >= 0 && ldw >= col0 + ncols, "pack_weight_h3w: bad arguments");
    CASPR_REQUIRE(((uintptr_t)packed % 16) == 0, "pack_weight_h3w: packed must be 16-byte aligned");
    unsigned char *out = (unsigned char *)packed;
    unsigned *tail = (unsigned *)(out + h3w_plane_bytes(Cout, ncols));
    const hipError_t err = hipMemsetAsync(tail, 0, XH_TAIL, (hipStream_t)stream);
    if (err != hipSuccess) {
        caspr_set_error("pack_weight_h3w: hipMemsetAsync failed: %s", hipGetErrorString(err));
        return CASPR_ELAUNCH;
    }
    h3w_weight_max_kernel<<<256, 256, 0, (hipStream_t)stream>>>(w, ldw, Cout, col0, ncols, tail);
    const long total = (long)ceil_div(Cout, CH_TM) * (ncols / 16) * 16 * 64;
    pack_weight_h3w_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(w, ldw, Cout, col0, ncols, out, total, tail);
    CASPR_CHECK_LAUNCH("pack_weight_h3w");
    return CASPR_OK;
}

int caspr_conv_h3w_launch(const void *wpk, const void *wtail, unsigned *status, const float *bias, const float *bbias, int bb_stride, const float *X, int ldx,
                          const float *in_scale, const float *in_shift, int in_relu, int in_relu_from, float *Y, int ldy, int B, int P, int Cin, int mt_begin,
                          int mt_end, void *part, int part_stride, int reserve_cus, hipStream_t stream) __attribute__((visibility("hidden")));

// channel tiles mt_begin .. mt_end - 1 (512 channels each) of the layer, as caspr_conv_x6w_launch; wtail: the tail of the layer's pack
// (the scale), status: the word the range guard ORs into (never cleared here: the host owns it)
int caspr_conv_h3w_launch(const void *wpk, const void *wtail, unsigned *status, const float *bias, const float *bbias, int bb_stride, const float *X, int ldx,
                          const float *in_scale, const float *in_shift, int in_relu, int in_relu_from, float *Y, int ldy, int B, int P, int Cin, int mt_begin,
                          int mt_end, void *part, int part_stride, int reserve_cus, hipStream_t stream)
{
    ConvHArgs a;
    a.wpk = (const unsigned char *)wpk; a.wtail = (const unsigned char *)wtail; a.status = status; a.bias = bias; a.bbias = bbias; a.X = X; a.Y = Y;
    a.part = (f32x4 *)part; a.ldx = ldx; a.ldy = ldy; a.P = P; a.Cin = Cin; a.Cout = mt_end * CH_TM; a.in_relu = in_relu; a.relu_from = in_relu_from;
    a.Mt = mt_end - mt_begin; a.mt0 = mt_begin; a.Pt = P / CH_TP; a.part_stride = part_stride; a.bb_stride = bb_stride;
    const long ntiles = (long)B * a.Mt * a.Pt;
    a.ntiles = (int)ntiles;
    // persistent: one workgroup per CU (512 registers per lane: one wave per SIMD), each walking through its share of the tiles
    static int n_cu = 0;
    if (!n_cu) {
        int dev = 0, v = 0;
        (void)hipGetDevice(&dev);
        n_cu = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
    }
    long grid = n_cu - (reserve_cus > 0 ? reserve_cus : 0);
    if (grid < 1) grid = 1;
    const long nblk = ntiles < grid ? ntiles : grid;
    const bool fused = in_scale != nullptr, stats = part != nullptr;
#define CH_GO(F, S) conv1x1_h3w_kernel<F, S><<<dim3((unsigned)nblk), dim3(256), CH_LDS, stream>>>(a, in_scale, in_shift)     /* 40 KB: below the 64 KB opt-in limit */
    if (fused && stats) CH_GO(true, true);
    else if (fused) CH_GO(true, false);
    else if (stats) CH_GO(false, true);
    else CH_GO(false, false);
#undef CH_GO
    return CASPR_OK;
}
