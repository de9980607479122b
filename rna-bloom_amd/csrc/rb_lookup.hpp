// rb_lookup.hpp — the read-only lookups of the graph's filters on the device, once each: graph.getCount of one hash and of four at a time, the
// read-pair filter's probe, and the wavefront's order statistic over count codes.  What every kernel that only READS the graph calls (rb_query,
// rb_mismatch, rb_correct, rb_overlap, rb_extend); the letter helpers and the run-time rotation that go with them need no FilterView and live in
// rb_device.hpp.  The insert path (rb_graph.hip) reads counters that are being written and keeps its own volatile loads.
//   Three forms of getCount, by how a kernel asks.  graph_count: probe after probe with the reference's early exits, where a lane has one count
// to ask and nothing else to wait for.  count_lookup (count_code / count_value): with two hash functions per filter all four probes first, for
// the wavefront-per-sequence kernels whose few asking lanes would else pay four dependent round trips.  probe4_h2 / count_lookup4: four hashes of
// one lane together.  The first is also the generic loop for any other number of hash functions; the other two have their own behind the fast path
// (tests/test_gpu_hash_counts.py runs those: every other world of these calls has two functions per filter).
//   Everything here is compiled before a unit's `#pragma clang fp contract(off)`: no function below has a product feeding a sum.
// Reference citations: R/ = src/rnabloom/ of bcgsc/RNA-Bloom v2.0.1.
#pragma once
#include "rb_pipeline.hpp"

namespace rb {

// CountingBloomFilter.getCount(long[]) :235-251 (zero check inside the h>=1 loop)
__device__ __forceinline__ float cbf_get_count(const uint8_t *cbf, const Mod &mod, int num_hash, uint64_t kmul, uint64_t h0) {
    uint32_t mn = cbf[index_of(h0, mod)];
    for (int j = 1; j < num_hash; ++j) {
        uint32_t c = cbf[index_of(multi_hash(h0, (uint32_t)j, kmul), mod)];
        if (c < mn) mn = c;
        if (mn == 0u) return 0.0f;
    }
    return minifloat_to_float(mn);
}
// BloomFilterDeBruijnGraph.getCount :562-570 as a float, one probe after the other with the reference's early exits: the form of the kernels
// whose every lane asks for one count in a dependent chain (k_graph_count, k_get_kmers, k_neighbors, the traversals; k_text_kmers and the
// edge gaps' variants in rb_correct.hip)
__device__ __forceinline__ float graph_count(const FilterView &fv, uint64_t h0) {
    if (!bits_lookup(fv.dbg, fv.dbg_mod, fv.dbg_h, fv.kmul, h0)) return 0.0f;
    return cbf_get_count(fv.cbf, fv.cbf_mod, fv.cbf_h, fv.kmul, h0) + 1.0f;
}

// graph.getCount of a k-mer hash for the wavefront-per-sequence kernels: `absent` where the hash is not in dbgbf, else present(the smallest counter
// byte).  With two hash functions per filter — every configuration the reference runs — the four probes are issued before any is consumed.
template <class T, class PRESENT> __device__ __forceinline__ T count_lookup(const FilterView &fv, uint64_t h, T absent, PRESENT present) {
    if (fv.dbg_h == 2 && fv.cbf_h == 2) {
        const uint64_t h1 = multi_hash(h, 1u, fv.kmul);
        const uint64_t b0 = index_of(h, fv.dbg_mod), b1 = index_of(h1, fv.dbg_mod), c0 = index_of(h, fv.cbf_mod), c1 = index_of(h1, fv.cbf_mod);
        const uint32_t w0 = fv.dbg[b0 >> 5], w1 = fv.dbg[b1 >> 5], n0 = fv.cbf[c0], n1 = fv.cbf[c1];
        if (!((w0 >> (uint32_t)(b0 & 31u)) & (w1 >> (uint32_t)(b1 & 31u)) & 1u)) return absent;
        return present(min(n0, n1));
    }
    if (!bits_lookup(fv.dbg, fv.dbg_mod, fv.dbg_h, fv.kmul, h)) return absent;
    uint32_t mn = fv.cbf[index_of(h, fv.cbf_mod)];                    // CountingBloomFilter.getCount(long[]) :235-251
    for (int j = 1; j < fv.cbf_h; ++j) mn = min(mn, (uint32_t)fv.cbf[index_of(multi_hash(h, (uint32_t)j, fv.kmul), fv.cbf_mod)]);
    return present(mn);
}
// ... as a count code (rb_device.hpp: 0 absent, else 1 + the MiniFloat byte), and as the float it stands for: count_code_value(count_code(fv, h)) ==
// count_value(fv, h) for every byte, without the test for code 0 that the compiler cannot drop
__device__ __forceinline__ uint32_t count_code(const FilterView &fv, uint64_t h) {
    return count_lookup(fv, h, 0u, [](uint32_t mn) { return 1u + mn; });
}
__device__ __forceinline__ float count_value(const FilterView &fv, uint64_t h) {
    return count_lookup(fv, h, 0.0f, [](uint32_t mn) { return minifloat_to_float(mn) + 1.0f; });
}

// Four hashes at once, two hash functions per filter (count_lookup4 below tests fv.dbg_h == 2 && fv.cbf_h == 2 and goes hash by hash otherwise;
// k_batch_counts collects its windows in fours and comes here directly): all filter indices, the 8 Bloom-bit loads, then the 8 counter loads, and
// only then the combination — one round trip where four count_code calls are four.  hash(a) is hash a = 0 .. 3; those from n on are padding,
// probed but not used (any resident line will do).  use(a, in, mn), a < n: hash a is in dbgbf (graph.contains); the minimum of its two counters,
// whatever `in` says.
template <class HASH, class USE> __device__ __forceinline__ void probe4_h2(const FilterView &fv, uint32_t n, HASH hash, USE use) {
    uint64_t bi[4][2], ci[4][2];
    uint32_t bw[4][2], cb[4][2];
#pragma unroll
    for (uint32_t a = 0; a < 4u; ++a) {
        const uint64_t h0 = hash(a), h1 = multi_hash(h0, 1u, fv.kmul);
        bi[a][0] = index_of(h0, fv.dbg_mod); bi[a][1] = index_of(h1, fv.dbg_mod);
        ci[a][0] = index_of(h0, fv.cbf_mod); ci[a][1] = index_of(h1, fv.cbf_mod);
    }
#pragma unroll
    for (uint32_t a = 0; a < 4u; ++a) { bw[a][0] = fv.dbg[bi[a][0] >> 5]; bw[a][1] = fv.dbg[bi[a][1] >> 5]; }
#pragma unroll
    for (uint32_t a = 0; a < 4u; ++a) { cb[a][0] = fv.cbf[ci[a][0]]; cb[a][1] = fv.cbf[ci[a][1]]; }
#pragma unroll
    for (uint32_t a = 0; a < 4u; ++a) {
        if (a >= n) break;
        const bool in = ((bw[a][0] >> (uint32_t)(bi[a][0] & 31u)) & (bw[a][1] >> (uint32_t)(bi[a][1] & 31u)) & 1u) != 0u;
        const uint32_t mn = cb[a][0] < cb[a][1] ? cb[a][0] : cb[a][1];
        use(a, in, mn);
    }
}
// graph.getCount of four hashes at once: use(a, in, mn) for a = 0 .. 3 — hash a is in dbgbf, and then mn is its smallest counter byte
template <class USE> __device__ __forceinline__ void count_lookup4(const FilterView &fv, const uint64_t (&h)[4], USE use) {
    if (fv.dbg_h == 2 && fv.cbf_h == 2) probe4_h2(fv, 4u, [&](uint32_t a) { return h[a]; }, use);
    else {
#pragma unroll
        for (uint32_t a = 0; a < 4u; ++a) { const uint32_t code = count_code(fv, h[a]); use(a, code != 0u, code - 1u); }
    }
}

// what a kernel needs of the read-pair filter, and PairedKeysBloomFilter.lookup of a pair key: with two hash functions both words are loaded
// before either is tested
struct PairView { const uint32_t *bits; Mod mod; int num_hash; uint64_t kmul; };
__device__ __forceinline__ bool pair_hit(const PairView &pf, uint64_t key) {
    if (pf.num_hash == 2) {
        const uint64_t i0 = index_of(key, pf.mod), i1 = index_of(multi_hash(key, 1u, pf.kmul), pf.mod);
        const uint32_t w0 = pf.bits[i0 >> 5], w1 = pf.bits[i1 >> 5];
        return ((w0 >> (uint32_t)(i0 & 31u)) & (w1 >> (uint32_t)(i1 & 31u)) & 1u) != 0u;
    }
    return bits_lookup(pf.bits, pf.mod, pf.num_hash, pf.kmul, key);
}
// ... and of two keys in two pair filters at once (a walked k-mer's read-paired and fragment-paired partner, rb_extend.hip): with two hash
// functions in both, the up to four words are loaded before any is tested.  key_a() / key_b() give the keys, each called only where it is
// asked (ask_a / ask_b); a key that is not asked loads nothing and misses.
template <class KA, class KB>
__device__ __forceinline__ void pair_hit2(const PairView &pa, KA key_a, bool ask_a, const PairView &pb, KB key_b, bool ask_b, bool &hit_a, bool &hit_b) {
    if (pa.num_hash == 2 && pb.num_hash == 2) {
        uint32_t wa0 = 0, wa1 = 0, wb0 = 0, wb1 = 0, sh = 0;                                  // a probe's word; its bit's place in it, a byte of sh each
        if (ask_a) {
            const uint64_t key = key_a(), i0 = index_of(key, pa.mod), i1 = index_of(multi_hash(key, 1u, pa.kmul), pa.mod);
            wa0 = pa.bits[i0 >> 5]; wa1 = pa.bits[i1 >> 5];
            sh = ((uint32_t)i0 & 31u) | (((uint32_t)i1 & 31u) << 8);
        }
        if (ask_b) {
            const uint64_t key = key_b(), i0 = index_of(key, pb.mod), i1 = index_of(multi_hash(key, 1u, pb.kmul), pb.mod);
            wb0 = pb.bits[i0 >> 5]; wb1 = pb.bits[i1 >> 5];
            sh |= (((uint32_t)i0 & 31u) << 16) | (((uint32_t)i1 & 31u) << 24);
        }
        hit_a = ((wa0 >> (sh & 31u)) & (wa1 >> ((sh >> 8) & 31u)) & 1u) != 0u;
        hit_b = ((wb0 >> ((sh >> 16) & 31u)) & (wb1 >> (sh >> 24)) & 1u) != 0u;
        return;
    }
    hit_a = ask_a && pair_hit(pa, key_a());
    hit_b = ask_b && pair_hit(pb, key_b());
}

// ---- order statistics of count codes by a whole wavefront ----
// Common.getMedian (R/util/Common.java:41-50) / getMedianKmerCoverage (R/util/GraphUtils.java:229-247): sorted[n / 2], or the float32 mean of
// sorted[n / 2 - 1] and sorted[n / 2].  code(p) is the count code of element p, 0 <= p < n, asked by lane p & 63.  An order statistic is found by
// bisection over the 129 code values with one ballot per 64 elements and step: no sort, no LDS.  All 64 lanes call; all get the result.
template <class CODE> __device__ __forceinline__ uint32_t kth_code(const CODE &code, int n, int rank, uint32_t lane) {
    uint32_t lo = 0, hi = 128;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        int cnt = 0;
        for (int p0 = 0; p0 < n; p0 += 64) {
            const int p = p0 + (int)lane;
            cnt += __popcll(__ballot(p < n && code(p) <= mid));
        }
        if (cnt >= rank + 1) hi = mid; else lo = mid + 1u;
    }
    return lo;
}
// the even / odd rule on top of any kth(rank) -> code (k_mismatch keeps its elements in registers and brings its own: rb_mismatch.hip mm_kth)
template <class KTH> __device__ __forceinline__ float median_of_kth(KTH kth, int n) {
    const float hi = count_code_value(kth(n / 2));
    if (n & 1) return hi;
    return (hi + count_code_value(kth(n / 2 - 1))) / 2.0f;
}
template <class CODE> __device__ __forceinline__ float median_code(const CODE &code, int n, uint32_t lane) {
    return median_of_kth([&](int rank) { return kth_code(code, n, rank, lane); }, n);
}
// the smallest code of elements [start, end) (getMinimumKmerCoverage(kmers, start, end), R/util/GraphUtils.java:133-145, as a code): code(p) is
// asked for start <= p < end; 255 for an empty range.  All 64 lanes call; all get the result.
template <class CODE> __device__ __forceinline__ uint32_t min_code(const CODE &code, int start, int end, uint32_t lane) {
    uint32_t mn = 255u;
    for (int p = start + (int)lane; p < end; p += 64) mn = min(mn, code(p));
    for (int s = 32; s > 0; s >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, s, 64));
    return mn;
}

}  // namespace rb
