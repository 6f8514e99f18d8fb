// ode_x6_setup.inc -- what the 64-point bf16x6 evaluation (ode_x6_eval.inc) needs set up once per launch.  Program TEXT, included at
// kernel scope by cnf_rk4_x6_kernel, cnf_dp5_kernel, cnf_train_fwd_kernel and cnf_sample_tape_kernel, not a function: a function, even
// an always-inline lambda, changes the register allocation of kernels this close to their budget.
//   expects in scope : `a` (its .w0, .w3), tid, wave (workgroup-uniform)
//   leaves behind    : lds, wbuf, s_gate, s_hb, s_w0, s_w3, s_g3 (LDS beyond s_g3 + 8 is the including kernel's own), the `dma` lambda,
//                      acc1, acc2, bkw, tg_, tb, tw
// The including kernel launches with XC_LDS bytes of dynamic LDS (or more) and issues `dma(a.w1x, 0, lane0 * 16)` before its first
// evaluation: every layer pass expects its first piece in flight.
extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
unsigned char *wbuf = lds;                                  // [XC_RING][XC_PIECE]
float *s_gate = (float *)(lds + XC_RING * XC_PIECE);        // [3][512] sigmoid gates of layers 0,1,2
float *s_hb = s_gate + 3 * XC_H;                            // [3][512] layer bias * gate + hyper bias
float *s_w0 = s_hb + 3 * XC_H;                              // [512][3]
float *s_w3 = s_w0 + 3 * XC_H;                              // [3][512] output layer
float *s_g3 = s_w3 + 3 * XC_H;                              // [8]: gate3[3], hb3[3]

for (int i = tid; i < 3 * XC_H; i += 256) {
    s_w0[i] = a.w0[i];
    s_w3[i] = a.w3[i];
}

// LDS-DMA of piece p (k chunk p >> 1, row half p & 1) of a layer's pack [row half][k chunk][48 KB image] into
// buffer p & 1: scalar base + one 32-bit lane offset (anything lane-dependent that is hoisted out of the stage
// loop ends up in scratch).  12 wave-instructions of 1 KB per wave, issued in three parts.
auto dma = [&](const unsigned char *wx, int p, int lane16, int s0 = 0, int s1 = 12) {
    const unsigned char *src = wx + (long)((p & 1) * 16 + (p >> 1)) * XC_PIECE + (wave * 12) * 1024;
#pragma unroll
    for (int sl = s0; sl < s1; ++sl)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + sl * 1024 + lane16),
                                         (__attribute__((address_space(3))) void *)(wbuf + (p & 1) * XC_PIECE + (wave * 12 + sl) * 1024), 16, 0, 0);
};

// The B fragments of a layer input are PRODUCED WHILE THE LAYER RUNS: the pieces go k-chunk-major, so chunk kc+1's three
// planes (12 registers) are only needed when chunk kc's two pieces are done -- its input-layer values (layer 1) or its
// slice of layer 1's epilogue (layer 2: gate * acc + bias, softplus, split) are computed in quarters inside the
// MFMA runs of chunk kc, where the VALU work hides behind the matrix pipe.  Two accumulator sets (layer 1's is
// consumed chunk by chunk while layer 2 fills its own) instead of 192 fragment registers.
f32x4 acc1[32], acc2[32];
u32x4 bkw[2][3];              // B-fragment planes of the current / next k chunk, by chunk parity
f32x4 tg_, tb, tw[3];         // table values of the half chunk being produced (gate, bias, input-layer weights)
