// rb_covwalk.hpp — the threshold walks of correctErrorsSE / correctErrorsPE / getCoverageStats over a 129-bin histogram of count codes instead of
// a sorted array: what rb_coverage.hip (rb_graph_read_coverage) and rb_pair_correct.hip (rb_graph_correct_pairs) both run.  Device code only.
#pragma once
#include "rb_device.hpp"

// Java float arithmetic: every product below is one float32 operation, rounded once.  (The products feed comparisons only, never a sum, so there
// is nothing to contract today; the pragma keeps it so, here and in the files that include this one, which set it for themselves as well.)
#pragma clang fp contract(off)

namespace rb {

constexpr int COV_BINS = 129;            // a bin per count code (count_code_of, rb_device.hpp): every count getCount can return

// the bin holding sorted position r (cum[b] = elements in bins < b, cum[COV_BINS] = n)
__device__ __forceinline__ int bin_of_rank(const uint32_t *cum, int64_t r) {
    int lo = 0, hi = COV_BINS - 1;                     // largest b with cum[b] <= r
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if ((int64_t)cum[mid] <= r) lo = mid; else hi = mid - 1; }
    return lo;
}
// The downward walk of the reference from sorted position s: pairs (covs[i], covs[i+1]) for i = s-1 .. 0, stop at the first with
// covs[i+1] * g > covs[i] (strict) or >= (PE); the threshold is then covs[i+1], else covs[0].  Over bins: the pairs inside one bin are
// all (v, v) and give the same answer, so a bin is tested once inside (when the walk sees two of its elements) and once against the
// next lower non-empty bin — the step-by-step loop's answer, multiplicities included.
__device__ inline float cov_walk(const uint32_t *cum, int64_t s, float g, bool strict, bool &found) {
    int b = bin_of_rank(cum, s);
    float v = count_code_value((uint32_t)b);
    int64_t seen = s - (int64_t)cum[b] + 1;            // elements of bin b at or below the walk's start
    for (;;) {
        const float t = v * g;
        if (seen >= 2 && (strict ? t > v : t >= v)) { found = true; return v; }
        int pb = b - 1;
        while (pb >= 0 && cum[pb + 1] == cum[pb]) --pb;
        if (pb < 0) { found = false; return v; }
        const float pv = count_code_value((uint32_t)pb);
        if (strict ? t > pv : t >= pv) { found = true; return v; }
        b = pb; v = pv; seen = (int64_t)cum[b + 1] - cum[b];
    }
}

}  // namespace rb
