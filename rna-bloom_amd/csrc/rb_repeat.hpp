// rb_repeat.hpp — SeqUtils.isRepeat of one k-mer by one lane, from the packed 2-bit codes of a batch: what the coverage statistics' isRepeat
// screen (rb_coverage.hip) and the repeat scan of the fragment-paired branch extension (rb_extend.hip) both ask.  The thresholds are the
// caller's: rb_coverage.hip passes Math.round of 0.9 * k, k / 2 and k / 3 as they are; rb_extend.hip passes "never" for one the reference's
// signed-byte counters cannot reach (DESIGN.md §5 "Fragment-paired branch extension").
// Reference citations: R/ = src/rnabloom/ of bcgsc/RNA-Bloom v2.0.1.
#pragma once
#include "rb_device.hpp"

namespace rb {

__device__ __forceinline__ uint32_t base_at(const uint32_t *cw32, uint32_t b) { return (cw32[b >> 4] >> (2u * (b & 15u))) & 3u; }

// SeqUtils.isRepeat (:458-497) of the k bases at b0: a base count >= t1, a dinucleotide count of one phase >= t2 or a trinucleotide count of
// one phase >= t3.  Each threshold is more than half of its phase's elements whenever it is above 1, so only a phase's majority element
// can reach it: one pass finds each phase's majority candidate (Boyer-Moore vote), a second pass counts it.  A phase holds the pairs /
// triples starting at offsets of one residue mod 2 / 3 (U is T: the batch's code of U is T's).
__device__ __forceinline__ void vote(uint32_t &cand, uint32_t &cnt, uint32_t d) {
    if (cnt == 0u) { cand = d; cnt = 1u; } else if (cand == d) ++cnt; else --cnt;
}
// base(j): the 2-bit code of the window's letter j — a batch's packed codes (window_is_repeat below) or a walk's row of a code a byte
template <class BASE> __device__ __forceinline__ bool window_is_repeat_of(BASE base, int k, int t1, int t2, int t3) {
    uint32_t cnt_ac = 0, cnt_gt = 0;                                 // base counts, 16 bits each
    uint32_t d0 = 0, d1 = 0, dn0 = 0, dn1 = 0;                       // dinucleotide candidates / votes, phases 0 1
    uint32_t e0 = 0, e1 = 0, e2 = 0, en0 = 0, en1 = 0, en2 = 0;      // trinucleotide candidates / votes, phases 0 1 2
    uint32_t p1 = 0, p2 = 0;                                         // the previous two bases
    uint32_t ph3 = 0;                                                // (j - 2) mod 3
    for (int j = 0; j < k; ++j) {
        const uint32_t c = base(j);
        if (c & 2u) cnt_gt += 1u << (16u * (c & 1u)); else cnt_ac += 1u << (16u * (c & 1u));
        if (j >= 1) {
            const uint32_t d = (p1 << 2) | c;
            if ((uint32_t)(j - 1) & 1u) vote(d1, dn1, d); else vote(d0, dn0, d);
        }
        if (j >= 2) {
            const uint32_t d = (p2 << 4) | (p1 << 2) | c;
            if (ph3 == 0u) vote(e0, en0, d); else if (ph3 == 1u) vote(e1, en1, d); else vote(e2, en2, d);
            ph3 = ph3 == 2u ? 0u : ph3 + 1u;
        }
        p2 = p1; p1 = c;
    }
    const int m1 = (int)max(max(cnt_ac & 0xffffu, cnt_ac >> 16), max(cnt_gt & 0xffffu, cnt_gt >> 16));
    if (m1 >= t1) return true;
    uint32_t n20 = 0, n21 = 0, n30 = 0, n31 = 0, n32 = 0;
    p1 = p2 = 0; ph3 = 0;
    for (int j = 0; j < k; ++j) {
        const uint32_t c = base(j);
        if (j >= 1) {
            const uint32_t d = (p1 << 2) | c;
            if ((uint32_t)(j - 1) & 1u) n21 += d == d1 ? 1u : 0u; else n20 += d == d0 ? 1u : 0u;
        }
        if (j >= 2) {
            const uint32_t d = (p2 << 4) | (p1 << 2) | c;
            if (ph3 == 0u) n30 += d == e0 ? 1u : 0u; else if (ph3 == 1u) n31 += d == e1 ? 1u : 0u; else n32 += d == e2 ? 1u : 0u;
            ph3 = ph3 == 2u ? 0u : ph3 + 1u;
        }
        p2 = p1; p1 = c;
    }
    // a phase with no element never returns (the reference's loop does not run); with elements, its majority's count decides
    return (k > 1 && (int)n20 >= t2) || (k > 2 && (int)n21 >= t2) ||
           (k > 2 && (int)n30 >= t3) || (k > 3 && (int)n31 >= t3) || (k > 4 && (int)n32 >= t3);
}
__device__ bool window_is_repeat(const uint32_t *cw32, uint32_t b0, int k, int t1, int t2, int t3) {
    return window_is_repeat_of([&](int j) { return base_at(cw32, b0 + (uint32_t)j); }, k, t1, t2, t3);
}

}  // namespace rb
