// rb_wave.hpp — what ONE wavefront does for the sequence, pair or window it works on, once: the direction of a walk (both strands' hashes in
// walking order), the 64-bit shuffle, the wavefront-scope fence, the scans of a range with a lane per index (first / last index where a predicate
// holds, a minimum, "all equal"), the check of a sequence's letters and the membership test of a walk's row — HashSet.contains / indexOf as a
// sweep of forward hashes that is confirmed on the bases.  The kernels of rb_extend, rb_join, rb_screen, rb_trim and rb_long are built from
// these; their walks differ and stay where they are.  Everything is in an unnamed namespace: a unit that includes this gets its own
// copy, inlined into its kernels.  Compiled before a unit's `#pragma clang fp contract(off)`: no function below has a product feeding a sum.
#pragma once
#include <math.h>

#include "rb_pipeline.hpp"
#include "rb_lookup.hpp"

namespace rb {
namespace {

// scratch layouts keep every array at a multiple of 16 bytes
__host__ __device__ constexpr size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// Math.round(float): floor(x + 1/2), exact in double for every float
__host__ __device__ __forceinline__ int64_t java_round(float x) { return (int64_t)floor((double)x + 0.5); }

// what one lane wrote to the wavefront's rows (LDS or device scratch) is what the others read behind this
__device__ __forceinline__ void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

__device__ __forceinline__ uint64_t wave_shfl64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}

// Both strands of a k-mer, in walking order: A rolls like a forward hash along the walk, B like a reverse-strand hash.  A right-hand walk
// has (f, r) = (A, B) with A over the bases' seeds and B over their complements'; a left-hand walk adds bases at the k-mer's front, so its
// A is the k-mer's reverse-strand hash and its B the forward one: xm / ym turn a base into the code whose seed A / B take.
// FUNNEL: the two rotations by k and k - 1 come out of 32-bit funnel shifts (rotl_var) where a kernel's registers ask for it, else out of
// 64-bit shifts (rotl); the value is the same.  Both kernels that are sensitive sit at a step of their occupancy: with the shifts k_screen takes 280
// registers for 245 (one wavefront per SIMD for two), with the funnel shifts the fragment-paired k_extend on device scratch 169 for 168 (two for three).
template <bool FUNNEL = false> struct WaveDir {
    int stranded, left;
    uint32_t uk, xm, ym;
    __device__ __forceinline__ uint64_t fwd(uint64_t A, uint64_t B) const { return left ? B : A; }
    __device__ __forceinline__ uint64_t hash(uint64_t A, uint64_t B) const { return stranded ? fwd(A, B) : smin(A, B); }
    __device__ __forceinline__ static uint64_t rot(uint64_t v, uint32_t s) { if constexpr (FUNNEL) return rotl_var(v, s); else return rotl(v, s); }
    // the neighbour that drops base `out` and takes base `in` (Successors / PredecessorsNTHashIterator)
    __device__ __forceinline__ void step(uint64_t A, uint64_t B, uint32_t out, uint32_t in, uint64_t &nA, uint64_t &nB) const {
        nA = rotl(A, 1) ^ rot(seed_of(out ^ xm), uk) ^ seed_of(in ^ xm);
        nB = rotr(B, 1) ^ rotr(seed_of(out ^ ym), 1) ^ rot(seed_of(in ^ ym), uk - 1u);
    }
};
template <bool FUNNEL = false> __device__ __forceinline__ WaveDir<FUNNEL> wave_dir(int stranded, int k, int left) {
    return WaveDir<FUNNEL>{stranded, left, (uint32_t)k, left ? 3u : 0u, left ? 0u : 3u};
}

// a letter outside ACGTU among the first `letters` of a sequence whose usable-letter bits start at valid_words (lane l looks at 32 letters at a time)
__device__ __forceinline__ bool wave_bad_letter(const uint32_t *valid_words, int letters, uint32_t lane) {
    bool bad = false;
    for (int w = (int)lane; 32 * w < letters; w += 64) {
        const int left = letters - 32 * w;
        const uint32_t want = left >= 32 ? 0xFFFFFFFFu : (1u << left) - 1u;
        bad = bad || (valid_words[w] & want) != want;
    }
    return __ballot(bad) != 0ull;
}

// ---- scans of [lo, hi) with a lane per index.  All 64 lanes call; all get the result. ----
// the first index where pred holds, else hi
template <class PRED> __device__ __forceinline__ int wave_first(int lo, int hi, PRED pred, uint32_t lane) {
    for (int p0 = lo; p0 < hi; p0 += 64) {
        const int p = p0 + (int)lane;
        const unsigned long long m = __ballot(p < hi && pred(p));
        if (m) return p0 + (int)__builtin_ctzll(m);
    }
    return hi;
}
// the last one, else lo - 1 (lane l looks at top - 1 - l, so the lowest set bit is the highest index)
template <class PRED> __device__ __forceinline__ int wave_last(int lo, int hi, PRED pred, uint32_t lane) {
    for (int top = hi; top > lo; top -= 64) {
        const int p = top - 1 - (int)lane;
        const unsigned long long m = __ballot(p >= lo && pred(p));
        if (m) return top - 1 - (int)__builtin_ctzll(m);
    }
    return lo - 1;
}
// the smallest value(p), +infinity for an empty range (getMinimumKmerCoverage over counts; over count codes: min_code, rb_lookup.hpp)
template <class VALUE> __device__ __forceinline__ float wave_min(int lo, int hi, VALUE value, uint32_t lane) {
    float mn = INFINITY;
    for (int p = lo + (int)lane; p < hi; p += 64) mn = fminf(mn, value(p));
    for (int s = 32; s > 0; s >>= 1) mn = fminf(mn, __shfl_xor(mn, s, 64));
    return mn;
}
// are the n bytes at x one value?  (SeqUtils.isHomopolymer(byte[]) :354-368)
__device__ __forceinline__ bool wave_all_equal(const uint8_t *x, int n, uint32_t lane) {
    bool same = true;
    for (int q = (int)lane; q < n; q += 64) same = same && x[q] == x[0];
    return __ballot(!same) == 0ull;
}

// HashSet.contains / indexOf over the k-mers a walk keeps: the first (last: the last) entry j in [lo, hi) that equals the candidate, else
// WAVE_NOWHERE.  A lane per entry compares the forward hashes — hash(j) against the candidate's, want — and a lane whose hash is equal confirms
// on the k bases by itself (Kmer.equals): entry_base(j, q) against cand_base(q), q = 0 .. k - 1.  How an entry's bases are found in the walk's
// text (by its start, or entry + 1 in walking order; reversed where the candidate walks the other way) is the callables' business.
constexpr int WAVE_NOWHERE = INT32_MIN;
template <class HASH, class EBASE, class CBASE>
__device__ __forceinline__ int wave_find(int lo, int hi, int k, HASH hash, uint64_t want, EBASE entry_base, CBASE cand_base, bool last, uint32_t lane) {
    int res = WAVE_NOWHERE;
    for (int base = lo; base < hi; base += 64) {
        const int j = base + (int)lane;
        bool hit = j < hi && hash(j) == want;
        if (hit) for (int q = 0; q < k && hit; ++q) hit = entry_base(j, q) == cand_base(q);
        const unsigned long long m = __ballot(hit);
        if (m) {
            if (!last) return base + (int)__builtin_ctzll(m);
            res = base + 63 - (int)__builtin_clzll(m);
        }
    }
    return res;
}

}  // namespace
}  // namespace rb
