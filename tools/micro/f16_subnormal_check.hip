// f16_subnormal_check.hip -- does v_mfma_f32_32x32x16_f16 honour f16 SUBNORMAL operands?  One wave: A = 2^-15 (an f16 subnormal) in
// every slot, B = 1: every output is 16 x 2^-15 = 2^-11 if the pipe honours them, 0 if it flushes.  Recorded by
// tests/test_cnf_f16x3.py into the parity report; the f16x3 CNF kernel (csrc/ode_f16x3w.hip) flushes its planes explicitly and does
// not depend on the answer.
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
__global__ __launch_bounds__(64) void k(float *out)
{
    f16x8 a, b;
    for (int j = 0; j < 8; ++j) {
        a[j] = __builtin_bit_cast(_Float16, (unsigned short)0x0200);   // 2^-15
        b[j] = (_Float16)1.0f;
    }
    f32x16 c = {};
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    out[threadIdx.x] = c[0];
}
int main()
{
    float *d, h[64];
    if (hipMalloc(&d, sizeof(h)) != hipSuccess) return 2;
    k<<<1, 64>>>(d);
    if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    printf("mfma f16 subnormal operands: out = %g (2^-11 = %g)  honoured=%d\n", h[0], 1.0 / 2048, h[0] == 1.0f / 2048);
    return 0;
}
