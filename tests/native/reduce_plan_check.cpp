// reduce_plan_check.cpp -- prints reduce_shape and reduce_plan (csrc/msm_reduce_plan.h), which MsmPlan sizes its buffers and
// launches its strided sums from, for the shapes tests/test_host_lib.py lists and compares with tests/reduce_model.py.  One line
// per (c, wide, groups, sum_one_step, lanes_per_output):
//   <c> <wide> <groups> <one_step> <lpo_opt>: <B> <R> <C> <bpr> <bpc> <part_len> | <steps> | <10 words of rows> <10 words of cols> <lpo> | ...
// with one "| jobs lpo" section per step, the SumJob words in the order of its members.  Stand-alone host program, no HIP:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined reduce_plan_check.cpp && ./a.out
#include <cstdio>
#include "../../zksnake_amd/csrc/msm_reduce_plan.h"

using namespace zkmi;

static void print_job(const SumJob& j) {
    printf(" %u %u %u %u %u %u %u %u %u %u", j.n_out, j.per_group, j.group_stride, j.outer, j.inner, j.count, j.out_offset, j.split, j.outer2, j.in_offset);
}

int main() {
    const int cs[] = {2, 3, 4, 9, 15, 16, 17, 20};
    const unsigned groups[] = {1, 2, 8, 16}, lpos[] = {0, 2, 64};
    for (int c : cs)
        for (unsigned g : groups)
            for (int one_step = 0; one_step < 2; ++one_step)
                for (unsigned lpo : lpos) {
                    const bool wide = c > 16;
                    ReduceShape s;
                    if (!reduce_shape(c, wide, &s)) {
                        printf("%d %d %u %d %u: refused\n", c, (int)wide, g, one_step, lpo);
                        continue;
                    }
                    printf("%d %d %u %d %u: %u %u %u %u %u %u", c, (int)wide, g, one_step, lpo, s.B, s.R, s.C, s.bpr, s.bpc, sum_part_len(s));
                    const ReducePlan p = reduce_plan(s, g, one_step != 0, lpo);
                    printf(" | %d", p.steps);
                    for (int k = 0; k < p.steps; ++k) {
                        printf(" |");
                        print_job(p.step[k].rows);
                        print_job(p.step[k].cols);
                        printf(" %u", p.step[k].lpo);
                    }
                    printf("\n");
                }
    return 0;
}
