// ode_h3w_setup.inc -- the LDS layout of the 128-point f16x3 evaluation (ode_h3w_eval.inc) and the tables that hold for the whole launch.
// Program TEXT, included at kernel scope by cnf_rk4_h3w_kernel and cnf_dp5_h3w_kernel, not a function: a function, even an always-inline
// lambda, changes the register allocation of kernels this close to their budget.  The rest of the once-per-launch setup is
// ode_h3w_ring.inc, included in front of the stage loop; between the two, each kernel loads its own state and the kc_* / k3_* table
// registers (that text is the same in both kernels and stays in both: where it stands among a kernel's own loads decides that kernel's
// register allocation, and it does not stand at either end of them).
//   expects in scope : `a` (its .hyper, .ldh, .w0, .w3, .w1x, .w2x), bt (the frame), tid
//   leaves behind    : lds, wbuf, s_hb0 .. s_g3 (LDS beyond s_g3 + 8 is the including kernel's own), hy, BOFF, sh1, sh2, act, un1, un2
// The including kernel launches with XH_LDS bytes of dynamic LDS (or more).
extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
unsigned char *wbuf = lds;                      // [XH_RING][XH_PIECE]
float *s_hb0 = (float *)(lds + XH_TAB);         // [512]     layer 0: (bias * gate + hyper bias) * 16
float *s_w0g = s_hb0 + XC_H;                    // [3][512]  layer 0: weight column d * gate * 16
float *s_g1 = s_w0g + 3 * XC_H;                 // [512]     sigmoid gate of hidden layer 1 * 2^-s1 (= gate * 2^-(4 + s1) * 16)
float *s_hb1 = s_g1 + XC_H;                     //           ... its bias * 16
float *s_g2 = s_hb1 + XC_H;                     // [512]     gate of hidden layer 2 * 2^-(4 + s2)
float *s_hb2 = s_g2 + XC_H;
float *s_w3 = s_hb2 + XC_H;                     // [3][512]  output layer
float *s_w0 = s_w3 + 3 * XC_H;                  // [512][3]  input layer (raw)
float *s_g3 = s_w0 + 3 * XC_H;                  // [8]: gate3[3], pad, hb3[3]

const float *hy = a.hyper + (long)bt * a.ldh;
constexpr int BOFF = 3 * XC_H + 3;

for (int i = tid; i < 3 * XC_H; i += 256) {
    s_w0[i] = a.w0[i];
    s_w3[i] = a.w3[i];
}
// the weight scales the pack kernel chose: W1 2^s1, W2 2^s2 are what the planes hold
const int sh1 = *(const int *)(a.w1x + XH_PACK), sh2 = *(const int *)(a.w2x + XH_PACK);
const float act = (float)(1 << XH_ACT_SHIFT), un1 = ldexpf(1.0f, -sh1), un2 = ldexpf(1.0f, -(XH_ACT_SHIFT + sh2));
