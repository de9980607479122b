// rb_align.hpp — SeqUtils.getDistance and getPercentIdentity (R/util/SeqUtils.java:164-229) by one wavefront: what error correction
// (rb_correct.hip: a repaired gap against the letters it replaces) and the represented screen (rb_screen.hip: an assembled walk or path
// against the sequence's own letters) both ask; and SeqUtils.isLowComplexityShort, which getMaxCoveragePath's meeting rule asks
// (rb_correct.hip, rb_long.hip).  getDistance is not a true Levenshtein distance (below), so it is neither symmetric nor
// reversal-invariant: callers pass the reference's operands in its order and orientation.
// Reference citations: R/ = src/rnabloom/ of bcgsc/RNA-Bloom v2.0.1.
#pragma once
#include "rb_device.hpp"

namespace rb {

constexpr int LEV_LDS = 1024;                 // columns of a Levenshtein row a wavefront keeps in LDS; longer rows live in device scratch

// a base as the walk kernels write it: upper case, U as T (the letters of a good k-mer are all of ACGTU)
__device__ __forceinline__ uint8_t ce_norm(uint32_t ch) { const uint32_t c = letter_code(ch); return c < 4u ? code_letter(c) : (uint8_t)ch; }

// SeqUtils.getDistance(String, String) (R/util/SeqUtils.java:190-229) by the whole wavefront.  The reference's System.arraycopy(v1, 0, v0, 0, tLen)
// copies tLen of the tLen + 1 entries, so v0[tLen] keeps its first value tLen: every column but the last is the Levenshtein matrix D, and the
// result is min(D[sLen][tLen-1] + 1, tLen + 1, D[sLen-1][tLen-1] + (s[sLen-1] != t[tLen-1])) — reproduced.  Columns 0 .. tLen-1 of a row are held
// 64 to a step, lane by lane (LDS, or device scratch for tLen > LEV_LDS): new[j] = min(new[j-1] + 1, old[j] + 1, old[j-1] + cost) is
// tmp[j] = min(old[j] + 1, old[j-1] + cost) followed by new[j] - j = the running minimum of tmp[j'] - j' — a prefix minimum across the lanes.
// A lane reads back only what it wrote itself; its left neighbour's old value comes by a shuffle.  sLen, tLen >= 1.
template <class S, class T> __device__ int ce_distance(S s, int slen, T t, int tlen, int *row, uint32_t lane) {
    bool diff = slen != tlen;
    if (!diff) {
        for (int x0 = 0; x0 < slen && !diff; x0 += 64) { const int x = x0 + (int)lane; diff = __ballot(x < slen && s(x) != t(x)) != 0ull; }
        if (!diff) return 0;                                                    // s.equals(t)
    }
    const int ncol = tlen;                                                      // columns 0 .. tLen - 1
    for (int j = (int)lane; j < ncol; j += 64) row[j] = j;
    int d_prev_last = ncol - 1, d_last = ncol - 1;                              // D[i][tLen-1] of the previous / this row
    for (int i = 1; i <= slen; ++i) {
        const uint32_t sc = s(i - 1);
        int carry = 0x3fffffff, carry_old = 0;
        for (int j0 = 0; j0 < ncol; j0 += 64) {
            const int j = j0 + (int)lane;
            const bool on = j < ncol;
            const int o = on ? row[j] : 0x3fffffff;
            int oprev = __shfl_up(o, 1, 64);
            if (lane == 0) oprev = carry_old;
            carry_old = __shfl(o, 63, 64);
            int v;
            if (!on) v = 0x3fffffff;
            else if (j == 0) v = i;
            else v = min(o + 1, oprev + (sc == (uint32_t)t(j - 1) ? 0 : 1)) - j;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int u = __shfl_up(v, d, 64); if ((int)lane >= d) v = min(v, u); }
            v = min(v, carry);
            carry = __shfl(v, 63, 64);
            if (on) row[j] = v + j;
            if (j0 + 64 >= ncol) { d_prev_last = d_last; d_last = __shfl(v + j, (ncol - 1) - j0, 64); }
        }
    }
    const int cost = s(slen - 1) == (uint32_t)t(tlen - 1) ? 0 : 1;
    return min(min(d_last + 1, tlen + 1), d_prev_last + cost);
}
// SeqUtils.getPercentIdentity(String, String) :164-175; the quotient is one float32 division (the including file sets contraction off)
__device__ __forceinline__ float ce_identity(int d, int alen, int blen) {
    if (alen <= blen) return ((float)(blen - d)) / (float)blen;
    return ((float)(alen - d)) / (float)alen;
}

// SeqUtils.isLowComplexityShort (R/util/SeqUtils.java:499-543) of the k letters get(0 .. k-1) (all of ACGT): lane l counts trinucleotide l, lanes
// 0..15 the dinucleotides, lanes 0..3 the letters; the thresholds are tested on the increments of letter 3 onwards, as the reference tests them
template <class GET> __device__ bool ce_low_complexity(GET get, int k, uint32_t lane) {
#pragma clang fp contract(off)                                           // Math.round(k * 0.95f): a float32 product, then the sum
    if (k < 3) return false;
    const int t1 = min(32767, (int)floorf((float)k * 0.95f + 0.5f)), t2 = min(32767, (int)floorf((float)(k / 2) * 0.95f + 0.5f)),
              t3 = min(32767, (int)floorf((float)(k / 3) * 0.95f + 0.5f));
    uint32_t c3 = letter_code(get(0)) & 3u, c2 = letter_code(get(1)) & 3u, c1 = letter_code(get(2)) & 3u;
    int n1 = (lane == c3) + (lane == c2) + (lane == c1), n2 = (lane == c3 * 4u + c2) + (lane == c2 * 4u + c1), n3 = lane == c3 * 16u + c2 * 4u + c1;
    for (int q = 3; q < k; ++q) {
        c3 = c2; c2 = c1; c1 = letter_code(get(q)) & 3u;
        bool hit = false;
        if (lane == c1) hit = ++n1 >= t1;
        if (lane == c2 * 4u + c1) hit = hit || ++n2 >= t2;
        if (lane == c3 * 16u + c2 * 4u + c1) hit = hit || ++n3 >= t3;
        if (__ballot(hit)) return true;
    }
    const int a0 = __shfl(n1, 0, 64), a1 = __shfl(n1, 1, 64), a2 = __shfl(n1, 2, 64), a3 = __shfl(n1, 3, 64);
    return a0 + a1 >= t1 || a0 + a2 >= t1 || a0 + a3 >= t1 || a1 + a2 >= t1 || a1 + a3 >= t1 || a2 + a3 >= t1;
}

}  // namespace rb
