// dp5_tables.inc -- the Dormand-Prince 5(4) tableau, Shampine's variant as torchdiffeq 0.0.1 dopri5.py: the ONE text of the tables that
// ode_dp5.hip, ode_dp5_f16x3w.hip and ode_latent_dp5.hip carry in constant memory.  Rows 0 and 1 of BETA are the two evaluations of
// the initial-step selection (y0 itself; y0 + h0 f0), rows 2..7 the six new stages of an attempt (the last one is y_new: FSAL).
//
// A text fragment and not a header: the arrays are non-static __constant__ variables, so every including file names its own copies
// -- #define DP5_TAB(x) <prefix>##x in front of the #include (DP_, DPH_, LDP_) -- and the host objects link; a file that never reads
// the stage times also defines DP5_TAB_NO_ALPHA.  (static tables would fold into the kernels and change their code: DESIGN.md §4.)
__constant__ float DP5_TAB(BETA)[8][6] = {
    {0.f, 0.f, 0.f, 0.f, 0.f, 0.f},
    {1.f, 0.f, 0.f, 0.f, 0.f, 0.f},
    {(float)(1.0 / 5), 0.f, 0.f, 0.f, 0.f, 0.f},
    {(float)(3.0 / 40), (float)(9.0 / 40), 0.f, 0.f, 0.f, 0.f},
    {(float)(44.0 / 45), (float)(-56.0 / 15), (float)(32.0 / 9), 0.f, 0.f, 0.f},
    {(float)(19372.0 / 6561), (float)(-25360.0 / 2187), (float)(64448.0 / 6561), (float)(-212.0 / 729), 0.f, 0.f},
    {(float)(9017.0 / 3168), (float)(-355.0 / 33), (float)(46732.0 / 5247), (float)(49.0 / 176), (float)(-5103.0 / 18656), 0.f},
    {(float)(35.0 / 384), 0.f, (float)(500.0 / 1113), (float)(125.0 / 192), (float)(-2187.0 / 6784), (float)(11.0 / 84)},
};
#ifndef DP5_TAB_NO_ALPHA
__constant__ double DP5_TAB(ALPHA)[8] = {0.0, 1.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
#endif
__constant__ float DP5_TAB(CERR)[7] = {(float)(35.0 / 384 - 1951.0 / 21600), 0.f, (float)(500.0 / 1113 - 22642.0 / 50085), (float)(125.0 / 192 - 451.0 / 720),
                                       (float)(-2187.0 / 6784 - -12231.0 / 42400), (float)(11.0 / 84 - 649.0 / 6300), (float)(-1.0 / 60.0)};
__constant__ float DP5_TAB(CMID)[7] = {(float)(6025192743.0 / 30085553152.0 / 2), 0.f, (float)(51252292925.0 / 65400821598.0 / 2),
                                       (float)(-2691868925.0 / 45128329728.0 / 2), (float)(187940372067.0 / 1594534317056.0 / 2),
                                       (float)(-1776094331.0 / 19743644256.0 / 2), (float)(11237099.0 / 235043384.0 / 2)};
#undef DP5_TAB
