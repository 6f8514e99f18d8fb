// dp5_rules.h -- the pure rules of the adaptive Dormand-Prince 5(4) controller as torchdiffeq 0.0.1 runs it (oracle.model.dopri5_solve
// restates it; its line numbers below): the ONE text of the step-size rule, the initial-step selection and the 4th-order interpolant
// that cnf_dp5_kernel<DIV> (ode_dp5.hip), cnf_dp5_h3w_kernel (ode_dp5_f16x3w.hip) and latent_dp5_kernel (ode_latent_dp5.hip) inline.
// The tableau is dp5_tables.inc.  Norms (which lanes, how many tensors) are the kernels' own: the rules take their results.
// Nothing here needs the GPU: a host compiler reads the file too (tools/dp5_rules_check.cpp, tests/test_dp5_shared.py).
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define DP5_RULE __host__ __device__ __forceinline__
#else
#define DP5_RULE static inline
#endif

#define DP5_SAFETY 0.9f
#define DP5_IFACTOR 10.0f
#define DP5_DFACTOR 0.2f

// the step after an attempt of step dt whose error ratio was r = mean((err / tol)^2), accepted or not   (model.py:252-257)
DP5_RULE float dp5_next_dt(float r, float dt)
{
    if (r == 0.f) return dt * DP5_IFACTOR;
    const float inv_d = r < 1.f ? 1.f : 1.f / DP5_DFACTOR;
    const float factor = fmaxf(1.f / DP5_IFACTOR, fminf(powf(sqrtf(r), 0.2f) / DP5_SAFETY, inv_d));
    return dt / factor;
}

// _select_initial_step, part 1 (model.py:226-228): h0 from d0 = rms(y / scale) and d1 = rms(f0 / scale).  On a state of several
// tensors d0 and d1 are the largest of the tensors' and quot() the largest of their dp5_quot.  quot is a callable, evaluated where
// the one-tensor expression evaluates it: with the quotient passed as a double all four kernels change (tools/code_object_diff.py,
// here / parent: cnf_dp5_kernel 20800 / 20808 and 25199 / 25202, cnf_dp5_h3w_kernel 14989 / 14988, latent_dp5_kernel 12402 / 12400)
DP5_RULE double dp5_quot(double d0, double d1) { return d0 / fmax(d1, 1e-300); }
template <typename Q>
DP5_RULE double dp5_h0(double d0, double d1, Q quot) { return (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * quot(); }
DP5_RULE double dp5_h0(double d0, double d1) { return dp5_h0(d0, d1, [=] { return dp5_quot(d0, d1); }); }

// part 2 (model.py:231-233): the first dt from d1, d2 = rms((f1 - f0) / scale) / h0 and h0.  The text is a macro: the two
// point-CNF kernels compile to other code through the function (tools/code_object_diff.py) and use the macro itself
#define DP5_FIRST_DT(d1, d2, h0) \
    fminf(100.f * (h0), ((d1) <= 1e-15f && (d2) <= 1e-15f) ? fmaxf(1e-6f, (h0) * 1e-3f) : powf(0.01f / fmaxf((d1), (d2)), 0.2f))
DP5_RULE float dp5_first_dt(float d1, float d2, float h0) { return DP5_FIRST_DT(d1, d2, h0); }

// the 4th-order interpolant of an accepted step of length h from (y0, f0) to (y1, f1) with the mid-point value ymid, in f64
// (model.py:263-267, 275): p(x) at x = (t - t0) / h in [0, 1].  The text is two macros -- the coefficients, declared in the
// caller's scope as A, B, C, D and y0d, and their Horner evaluation -- which the functions wrap; cnf_dp5_h3w_kernel (488 of 512
// VGPRs) compiles to other code through the functions and uses the macros themselves
#define DP5_INTERP_COEFS(y0, y1, ymid, f0, f1, h_)                                       \
    const double y0d = y0, y1d = y1, ymd = ymid, fa = f0, fb = f1, h = h_;               \
    const double A = 2.0 * h * (fb - fa) - 8.0 * (y1d + y0d) + 16.0 * ymd;               \
    const double B = h * (5.0 * fa - 3.0 * fb) + 18.0 * y0d + 14.0 * y1d - 32.0 * ymd;   \
    const double C = h * (fb - 4.0 * fa) - 11.0 * y0d - 5.0 * y1d + 16.0 * ymd;          \
    const double D = h * fa;
#define DP5_INTERP_HORNER(x) ((((A * (x) + B) * (x) + C) * (x) + D) * (x) + y0d)
struct Dp5Interp { double A, B, C, D, y0; };
DP5_RULE Dp5Interp dp5_interp(double y0, double y1, double ymid, double f0, double f1, double h_)
{
    DP5_INTERP_COEFS(y0, y1, ymid, f0, f1, h_)
    return Dp5Interp{A, B, C, D, y0d};
}
DP5_RULE double dp5_interp_at(const Dp5Interp &p, double x)
{
    const double A = p.A, B = p.B, C = p.C, D = p.D, y0d = p.y0;
    return DP5_INTERP_HORNER(x);
}
