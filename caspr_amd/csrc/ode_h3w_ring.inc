// ode_h3w_ring.inc -- the weight stream of the 128-point f16x3 evaluation (ode_h3w_eval.inc) and its registers: the LDS-DMA of a piece
// into the eight-deep ring, the first seven pieces issued, the first fragments read.  Program TEXT, included at kernel scope by
// cnf_rk4_h3w_kernel and cnf_dp5_h3w_kernel in front of their stage loops (see ode_h3w_setup.inc).
//   expects in scope : the switches of ode_h3w.h, `a` (its .w1x, .w2x), lane0, wave (workgroup-uniform), wbuf
//   leaves behind    : piece_src, dma1, dma_open, dma_kb, acc2, fX, fY, b1w, b2w, xmax, ones; pieces 0..6 of the stream in flight and the
//                      first fragments of piece 0 in fX
// Every evaluation leaves the next seven pieces in flight: the including kernel waits with vmcnt(0) behind its last one.

// The weight stream of one stage: 128 pieces, layer 1 chunk-major (s = 4 kc + rq), then layer 2 pass-major (s = 64 + 16 q + kc);
// piece (rq, kc) of a layer's pack sits at (rq * 16 + kc) * XH_PIECE.  Ring slot s & 7.  The index runs on from stage to stage of
// the launch (& 127: 128 pieces are a multiple of the ring)
auto piece_src = [&](int s_) -> const unsigned char * {
    s_ &= 127;
    const int l2 = s_ >> 6, t_ = s_ & 63;
    const int rq = l2 ? (t_ >> 4) : (t_ & 3), kc = l2 ? (t_ & 15) : (t_ >> 2);
    return (l2 ? a.w2x : a.w1x) + (long)(rq * 16 + kc) * XH_PIECE;
};
// LDS-DMA of kilobyte i0 (0..3) of this wave's 4 KB share of sequence piece s_: ONE global_load_lds_dwordx4 in the SADDR form (see
// ode_bf16x6w.hip); M0 has no other user in this kernel (audit.py)
auto dma1 = [&](int s_, int lane16, int i0) XW_INL {
    const unsigned char *src = piece_src(s_) + (wave * 4 + i0) * 1024;
    const unsigned dst = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)(wbuf + (s_ & (XH_RING - 1)) * XH_PIECE + (wave * 4 + i0) * 1024);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" : : "s"(dst), "v"(lane16), "s"(src) : "memory");
};
// ... and the four of a piece on ONE source address and ONE M0 write: kilobyte i0 is 1024 i0 further on both sides, which is
// what the instruction's immediate offset adds to the global AND to the LDS address.  dma_open (the wave's share of piece s_:
// M0 <- its place in the ring, returns its place in the pack) goes into the slot in front of the first dma_kb, so that an MFMA
// supplies the wait state between the M0 write and the load; M0 then stays put until the next piece's dma_open
auto dma_open = [&](int s_) XW_INL -> const unsigned char * {
    const unsigned dst = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)(wbuf + (s_ & (XH_RING - 1)) * XH_PIECE + wave * 4096);
    asm volatile("s_mov_b32 m0, %0" : : "s"(dst) : "memory");
    return piece_src(s_) + wave * 4096;
};
auto dma_kb = [&](const unsigned char *src, int lane16, auto I0) XW_INL {
    asm volatile("global_load_lds_dwordx4 %0, %1 offset:%c2" : : "v"(lane16), "s"(src), "i"(1024 * decltype(I0)::value) : "memory");
};

// pieces 0..6 in flight before the first one is consumed
#pragma unroll
for (int s_ = 0; s_ < XH_RING - 1; ++s_) {
    if constexpr (XH_OLD_DMA) {
#pragma unroll
        for (int i0 = 0; i0 < 4; ++i0) dma1(s_, lane0 * 16, i0);
    } else {
        const unsigned char *src = dma_open(s_);
        asm volatile("s_nop 0" ::: "memory");      // M0 write -> LDS-DMA: one wait state (no MFMA in between here)
        xw_for<0, 4>([&](auto I0) XW_INL { dma_kb(src, lane0 * 16, I0); });
    }
}

f32x16 acc2[4];               // layer 2: the 128 rows of the running pass
f16x8 fX[2][2], fY[2][2];     // A fragments: two sets of two row tiles x two planes
u32x4 b1w[2][2][2];           // layer 1 B planes [chunk parity][k-step of the chunk][plane]
u32x4 b2w[2][2];              // layer 2 B planes [k-step parity][plane]
float xmax = 0.0f;            // range guard: the largest scaled activation this lane has split
// for the flush of the plane words.  (Not materialised under the f32 flush, which has no use for it: xh_ones is an asm statement, and a
// register that only it touches still moves its neighbourhood.)
const unsigned ones = XH_OLD_FLUSH ? 0u : xh_ones();

// fragments of region 0 of piece 0 (k-step 0, row tiles 0, 1): the only exposed fragment read of the kernel
asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
__builtin_amdgcn_s_barrier();
asm volatile("" ::: "memory");
{
    const unsigned char *A0 = wbuf + lane0 * 16;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) fX[u][pl] = *(const f16x8 *)(A0 + (u * 2 + pl) * XH_FRAG);
}
