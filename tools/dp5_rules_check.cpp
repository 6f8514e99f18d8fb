// dp5_rules_check.cpp -- the pure rules of the adaptive solves (caspr_amd/csrc/dp5_rules.h) compiled for the host and printed, for
// tests/test_dp5_shared.py to hold against oracle.model.dopri5_solve's arithmetic.  No GPU, no HIP: any C++11 compiler.
//   c++ -O2 -std=c++11 -I caspr_amd/csrc -o dp5_rules_check tools/dp5_rules_check.cpp
//   dp5_rules_check next r dt | h0 d0 d1 | first d1 d2 h0 | interp y0 y1 ymid f0 f1 h x
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dp5_rules.h"

int main(int argc, char **argv)
{
    double v[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = 2; i < argc && i < 9; ++i) v[i - 2] = strtod(argv[i], NULL);
    if (argc == 4 && !strcmp(argv[1], "next")) printf("%.9g\n", (double)dp5_next_dt((float)v[0], (float)v[1]));
    else if (argc == 4 && !strcmp(argv[1], "h0")) printf("%.17g\n", dp5_h0(v[0], v[1]));
    else if (argc == 5 && !strcmp(argv[1], "first")) printf("%.9g\n", (double)dp5_first_dt((float)v[0], (float)v[1], (float)v[2]));
    else if (argc == 9 && !strcmp(argv[1], "interp")) printf("%.17g\n", dp5_interp_at(dp5_interp(v[0], v[1], v[2], v[3], v[4], v[5]), v[6]));
    else return 2;
    return 0;
}
