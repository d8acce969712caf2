// ntt_plan.h -- the pass plan of a 2^log_n transform (ntt.hip): how many passes, and for each the stages m it performs and the
// run length exponent q of its global accesses.  Plain C++, no HIP include: tests/native/ntt_plan_check.cpp prints it for every
// size and tests/test_host_lib.py compares that with the integer model of the tests (tests/qap_model.py::plan).
#pragma once
#include <algorithm>

namespace zkmi {

constexpr int NTT_TILE_LOG = 11;   // 2048 elements = 72 KiB of LDS per workgroup (limb-major), two workgroups per CU
constexpr int NTT_MAX_DIGIT = 8;   // stages per pass: 2^8 x 2^3 runs of 256 B at least

struct NttPass {
    int m, q;   // a workgroup owns all 2^m values of the pass's digit for a run of 2^q consecutive values of the rest of the index
};

// Pass plan: ceil(log_n / 8) passes, the stages split as evenly as possible with the larger digits LAST (the later
// passes share one twiddle among the 2^q elements of a run and read small table rows; the first pass streams one twiddle
// per butterfly).  Every global access is a run of 256 or 512 bytes; a single pass (log_n <= NTT_TILE_LOG) has q = 0: one
// workgroup holds the whole vector.  Returns the number of passes (0 for log_n = 0, at most 4 for log_n <= 30).
inline int ntt_plan(int log_n, NttPass out[8]) {
    if (log_n <= 0) return 0;
    const int passes = log_n <= NTT_TILE_LOG ? 1 : (log_n + NTT_MAX_DIGIT - 1) / NTT_MAX_DIGIT;
    // Stages per pass.  An odd count costs a radix-2 step (616 instructions for one stage of four elements against 1054 for the two
    // stages of a radix-4 step), so odd digits are paired up into even ones where the sum allows it, and the smallest digit goes in
    // the middle (2^22: 8 + 6 + 8 runs 0.557 ms, 8 + 8 + 6 0.564, 6 + 8 + 8 0.571, the balanced 7 + 7 + 8 0.580-0.592)
    int digits[8] = {0};
    for (int i = 0, r = log_n; i < passes; ++i) { digits[i] = r / (passes - i); r -= digits[i]; }
    for (;;) {
        int a = -1, b = -1;
        for (int i = 0; i < passes; ++i) if (digits[i] & 1) { if (a < 0) a = i; else if (b < 0) b = i; }
        if (b < 0) break;
        if (digits[a] < NTT_MAX_DIGIT) { ++digits[a]; --digits[b]; }
        else if (digits[b] < NTT_MAX_DIGIT) { ++digits[b]; --digits[a]; }
        else break;
    }
    std::sort(digits, digits + passes, [](int x, int y) { return x > y; });
    if (passes >= 3) {   // smallest to the middle: rotate it in from the end
        const int small = digits[passes - 1], mid = passes / 2;
        for (int i = passes - 1; i > mid; --i) digits[i] = digits[i - 1];
        digits[mid] = small;
    }
    for (int i = 0; i < passes; ++i) out[i] = {digits[i], passes == 1 ? 0 : std::min(NTT_TILE_LOG - digits[i], log_n - digits[i])};
    return passes;
}

}  // namespace zkmi
