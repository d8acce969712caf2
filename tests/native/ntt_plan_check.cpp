// ntt_plan_check.cpp -- prints ntt_plan (csrc/ntt_plan.h) for log_n = 0 .. 30, one line each: "<log_n>: m,q m,q ...".
// tests/test_host_lib.py compares the lines with tests/qap_model.py::plan.  Stand-alone host program, no HIP:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined ntt_plan_check.cpp && ./a.out
#include <cstdio>
#include "../../zksnake_amd/csrc/ntt_plan.h"

int main() {
    for (int log_n = 0; log_n <= 30; ++log_n) {
        zkmi::NttPass plan[8];
        const int passes = zkmi::ntt_plan(log_n, plan);
        printf("%d:", log_n);
        for (int i = 0; i < passes; ++i) printf(" %d,%d", plan[i].m, plan[i].q);
        printf("\n");
    }
    return 0;
}
