// rb_trim.hip — rb_graph_trim_rc_artifacts: the three overloads of GraphUtils.trimReverseComplementArtifact for host sequences on the device —
// (kmers, graph, stranded) (R/util/GraphUtils.java:8588-8661, mode RB_TRIM_HASHES), (seqKmers, maxEdgeClip, maxIndelSize, minPercentIdentity,
// graph) (:7918-8057, RB_TRIM_EDGE) and the seven-argument one (:7762-7916, RB_TRIM_LONG).  Per piece the getKmers kernel leaves the sequences'
// hashes and counts in device scratch and k_trim_artifacts runs the mode, a wavefront per sequence.  The wavefront first builds an exact set of
// 64-bit hashes by open addressing — HASHES' HashSet of the left half's reverse-strand hashes; for the other two modes the getHash() of every
// k-mer, a prefilter: a seed whose getReverseComplementHash() is not in it matches no candidate, so its scan is skipped and nothing else
// changes.  The set lives in the wavefront's row of LDS for a list of up to TR_LDS_LIST k-mers and in a row of device scratch the wavefront
// owns beyond.  Scans take a lane per candidate: a ballot of the hash equality, hits in the reference's order, each confirmed on the bases by
// the whole wavefront (seed base q against candidate base k - 1 - q complemented); the inward runs of EDGE take a lane per step and confirm in
// the lane.  Minimum and median coverage are taken over count codes (rb_lookup.hpp).  Nothing is written to the graph (DESIGN.md §5 "Trimming
// reverse-complement artifacts").
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rb_pieces.hpp"
#include "rb_lookup.hpp"
#include "rb_repeat.hpp"
#include "rb_wave.hpp"

using namespace rb;

// Java float arithmetic: the median of an even number of counts is one float32 sum and one quotient; cov * maxCovGradient is one product
#pragma clang fp contract(off)

namespace {

constexpr int TR_TPB = 256;
constexpr int TR_WAVES = TR_TPB / 64;     // sequences a workgroup works on at a time: a wavefront each
constexpr int TR_MAX_SLOTS = 2048;        // wavefronts of a launch at the most (each takes sequences in turn)
constexpr int TR_LDS_LIST = 512;          // the longest k-mer list whose hash table stays in LDS (32 KB a workgroup)
constexpr int TR_LDS_SLOTS = 2 * TR_LDS_LIST;
constexpr int TR_MAX_CLIP = 1 << 20;      // the largest max_edge_clip taken
constexpr int TR_MAX_LIST = 1 << 24;      // the longest sequence taken, in k-mers
constexpr size_t TR_TAB_BUDGET = (size_t)512 << 20;   // device scratch all wavefronts' tables may take together (at least 4 wavefronts run whatever a table costs)

struct TrArgs {
    int stranded, k, mode, clip, tab_cap;    // tab_cap: slots of a wavefront's table in device scratch (0: every list fits LDS)
    float grad;
    int64_t pn;
    const int64_t *kof;                      // k-mer offsets of the piece's sequences
    const uint64_t *F;                       // their getKmers rows; in a stranded graph the row R holds 0 and the sequence's wavefront fills it
    uint64_t *R;
    const float *cnt;
    const uint64_t *codes;                   // the piece's batch: 2-bit codes and usable bits of its letters
    const uint32_t *valid, *woff;
    rb_trim_rec *recs;
};

#define TR_FENCE_TABLE() __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent")

// HashSet<Long>: open addressing over 64-bit keys, linear probing, at most half full.  An empty slot holds 0; the key 0 — a real hash — is not
// stored but kept as the mark `zero`.  Inserts are compare-and-swap (equal keys of several lanes meet in one slot); lookups load past the
// vector cache, which the atomics do not update.
struct TrSet {
    uint64_t *tab;
    uint32_t mask;
    bool zero;
    __device__ __forceinline__ uint32_t slot(uint64_t key) const { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask; }
    __device__ __forceinline__ bool has(uint64_t key) const {
        if (key == 0ull) return zero;
        for (uint32_t s = slot(key);; s = (s + 1u) & mask) {
            const uint64_t v = __hip_atomic_load(&tab[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v == key) return true;
            if (v == 0ull) return false;
        }
    }
};
// the set of key(0) .. key(n - 1) in the table `tab`, which holds the next power of two >= max(64, 2 n) slots
template <class KEY> __device__ TrSet tr_set_build(uint64_t *tab, int n, KEY key, uint32_t lane) {
    uint32_t slots = 64u;
    while (slots < 2u * (uint32_t)n) slots <<= 1;
    for (uint32_t s = lane; s < slots; s += 64u) tab[s] = 0ull;
    TR_FENCE_TABLE();
    TrSet st{tab, slots - 1u, false};
    bool z = false;
    for (int i = (int)lane; i < n; i += 64) {
        const uint64_t h = key(i);
        if (h == 0ull) { z = true; continue; }
        for (uint32_t s = st.slot(h);; s = (s + 1u) & st.mask) {
            const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long *>(&tab[s]), 0ull, (unsigned long long)h);
            if (old == 0ull || old == h) break;
        }
    }
    TR_FENCE_TABLE();
    st.zero = __ballot(z) != 0ull;
    return st;
}

// what the wavefront reads of its sequence
struct TrSeq {
    const uint32_t *cw32;
    const uint64_t *F, *R;
    const float *cnt;
    int nk, k, stranded;
    __device__ __forceinline__ uint32_t base(int p) const { return base_at(cw32, (uint32_t)p); }
    __device__ __forceinline__ uint32_t code(int i) const { return count_code_of(cnt[i]); }
    // Kmer.getHash() / getReverseComplementHash(): f and NTP64RC; CanonicalKmer's are both min(f, r)
    __device__ __forceinline__ uint64_t hv(int i) const { return stranded ? F[i] : smin(F[i], R[i]); }
    __device__ __forceinline__ uint64_t rc(int i) const { return stranded ? R[i] : smin(F[i], R[i]); }
    // SeqUtils.isReverseComplement (R/util/SeqUtils.java:1257-1271) of k-mers s and c: by the wavefront, and by one lane
    __device__ __forceinline__ bool is_rc(int s, int c, uint32_t lane) const {
        bool ne = false;
        for (int q = (int)lane; q < k; q += 64) ne = ne || 3u - base(s + q) != base(c + k - 1 - q);
        return __ballot(ne) == 0ull;
    }
    __device__ __forceinline__ bool is_rc_lane(int s, int c) const {
        for (int q = 0; q < k; ++q) if (3u - base(s + q) != base(c + k - 1 - q)) return false;
        return true;
    }
};
// the list a pass works on: k-mers [o, o + n) of the sequence, in the list's own numbering
struct TrList {
    const TrSeq &sq;
    int o, n;
    __device__ __forceinline__ uint64_t hv(int i) const { return sq.hv(o + i); }
    __device__ __forceinline__ uint64_t rc(int i) const { return sq.rc(o + i); }
    // getMinimumKmerCoverage(kmers, start, end) (:133-145): k-mer `start` counts whatever `end` is
    __device__ __forceinline__ uint32_t min_cov(int start, int end, uint32_t lane) const {
        const TrSeq &s = sq;
        return min_code([&](int p) { return s.code(p); }, o + start, o + max(end, start + 1), lane);
    }
    __device__ __forceinline__ float median(int start, int end, uint32_t lane) const {
        const TrSeq &s = sq;
        const int at = o + start;
        return median_code([&](int p) { return s.code(at + p); }, end - start, lane);
    }
};

// the first j of from, from + 1, .. to - 1 with candidate.getHash() == seed.getReverseComplementHash() && isReverseComplement(seed, candidate), else -1
__device__ int tr_scan_up(const TrList &L, int seed, int from, int to, uint32_t lane) {
    const uint64_t want = L.rc(seed);
    for (int j0 = from; j0 < to; j0 += 64) {
        const int j = j0 + (int)lane;
        unsigned long long m = __ballot(j < to && L.hv(j) == want);
        while (m) {
            const int hit = j0 + (int)__builtin_ctzll(m);
            m &= m - 1ull;
            if (L.sq.is_rc(L.o + seed, L.o + hit, lane)) return hit;
        }
    }
    return -1;
}
// ... of hi, hi - 1, .. lo (lane l looks at top - l, so the lowest set bit is the highest index)
__device__ int tr_scan_down(const TrList &L, int seed, int hi, int lo, uint32_t lane) {
    const uint64_t want = L.rc(seed);
    for (int top = hi; top >= lo; top -= 64) {
        const int j = top - (int)lane;
        unsigned long long m = __ballot(j >= lo && L.hv(j) == want);
        while (m) {
            const int hit = top - (int)__builtin_ctzll(m);
            m &= m - 1ull;
            if (L.sq.is_rc(L.o + seed, L.o + hit, lane)) return hit;
        }
    }
    return -1;
}
// how many of the steps t = 0, 1, .. steps - 1 match from the first on without a break: seed a0 + t da, candidate b0 + t db (a lane per step)
__device__ int tr_run(const TrList &L, int a0, int da, int b0, int db, int steps, uint32_t lane) {
    for (int t0 = 0; t0 < steps; t0 += 64) {
        const int t = t0 + (int)lane;
        bool bad = false;
        if (t < steps) {
            const int s = a0 + t * da, c = b0 + t * db;
            bad = !(L.hv(c) == L.rc(s) && L.sq.is_rc_lane(L.o + s, L.o + c));
        }
        const unsigned long long m = __ballot(bad);
        if (m) return t0 + (int)__builtin_ctzll(m);
    }
    return steps;
}

// The anchor scan from the left (:7928-7943, :7775-7792): seeds 0 .. stop - 1, each against the candidates behind it; the loop stops only at a
// seed index > 0, so a match of seed 0 stays unless a later seed has one.  ai, aj: the seed and its candidate, or -1.
__device__ void tr_anchor_l2r(const TrList &L, const TrSet &set, int stop, int &ai, int &aj, uint32_t lane) {
    ai = -1; aj = -1;
    for (int i0 = 0; i0 < stop && !(ai > 0); i0 += 64) {
        const int s = i0 + (int)lane;
        unsigned long long m = __ballot(s < stop && set.has(L.rc(s)));
        while (m) {
            const int i = i0 + (int)__builtin_ctzll(m);
            m &= m - 1ull;
            const int j = tr_scan_up(L, i, i + 1, L.n, lane);
            if (j >= 0) { ai = i; aj = j; }
            if (ai > 0) break;
        }
    }
}
// ... from the right (:7995-8010, :7848-7865): seeds n - 1 .. stop, each against the candidates before it
__device__ void tr_anchor_r2l(const TrList &L, const TrSet &set, int stop, int &ai, int &aj, uint32_t lane) {
    ai = -1; aj = -1;
    for (int top = L.n - 1; top >= stop && !(ai > 0); top -= 64) {
        const int s = top - (int)lane;
        unsigned long long m = __ballot(s >= stop && set.has(L.rc(s)));
        while (m) {
            const int i = top - (int)__builtin_ctzll(m);
            m &= m - 1ull;
            const int j = tr_scan_down(L, i, i - 1, 0, lane);
            if (j >= 0) { ai = i; aj = j; }
            if (ai > 0) break;
        }
    }
}

__device__ __forceinline__ rb_trim_pass tr_pass(int why, int i0, int i1, int i2, int i3) { return rb_trim_pass{why, i0, i1, i2, i3}; }

// (kmers, graph, stranded) (:8588-8661)
__device__ void tr_hashes(const TrArgs &a, const TrSeq &sq, uint64_t *tab, rb_trim_rec &rec, uint32_t lane) {
    const int n = sq.nk, half = n / 2;
    const TrSet set = tr_set_build(tab, half, [&](int i) { return sq.R[i]; }, lane);
    int start = -1, num = 0;
    for (int i0 = half; i0 < n; i0 += 64) {
        const int i = i0 + (int)lane;
        const unsigned long long m = __ballot(i < n && set.has(sq.F[i]));
        if (m && start < 0) start = i0 + (int)__builtin_ctzll(m);
        num += __popcll(m);
    }
    rec.pass[0] = tr_pass(0, start, num, -1, -1);
    if (num < a.k || start < half) return;                       // (start >= half wherever num > 0)
    if (start == half) {                                         // need to adjust start position (:8616-8621): the loop runs down to 0, its last hit is the lowest
        for (int i0 = 0; i0 <= half; i0 += 64) {
            const int i = i0 + (int)lane;
            const unsigned long long m = __ballot(i <= half && set.has(sq.F[i]));
            if (m) { start = i0 + (int)__builtin_ctzll(m); break; }
        }
        rec.pass[0].why = 2;
    } else rec.pass[0].why = 1;
    rec.pass[0].i2 = start;
    rec.flags |= RB_TRIM_FOUND;
    rec.begin = start;
}

// (seqKmers, maxEdgeClip, maxIndelSize, minPercentIdentity, graph) (:7918-8057)
__device__ void tr_edge(const TrArgs &a, const TrSeq &sq, const TrSet &set, rb_trim_rec &rec, uint32_t lane) {
    const int k = a.k, clip = a.clip;
    int o = 0, n = sq.nk;
    {   // search from left to right
        const TrList L{sq, o, n};
        int left, right;
        tr_anchor_l2r(L, set, min(clip, n), left, right, lane);
        rb_trim_pass ps = tr_pass(0, left, right, -1, -1);
        if (left > 0 && right - left >= k) {
            int cut = left + 1;
            int c = tr_run(L, left + k, k, right - k, -k, (right - left - 1) / k, lane);               // i = k, 2k, .. < right - left
            if (c > 0) cut = left + c * k;
            const int s0 = cut - left;
            c = tr_run(L, left + s0, 1, right - s0, -1, right - left - s0, lane);
            if (c > 0) cut = left + s0 + c - 1;
            cut = min(cut, (left + right) / 2);
            ps.i2 = cut;
            int nb, ne;
            if (right >= n - clip) {
                const int cl = cut - left;
                ps.i3 = cl;
                const uint32_t lmin = L.min_cov(cut, min(n, cut + k), lane), rmin = L.min_cov(max(0, n - cl - k), n - cl, lane);
                if (lmin > rmin) { ps.why = 1; nb = 0; ne = max(1, n - cl - k); }
                else { ps.why = 2; nb = cut; ne = n; }
            } else { ps.why = 3; nb = min(n - 1, cut + k); ne = n; }
            o += nb; n = ne - nb;
        }
        rec.pass[0] = ps;
    }
    {   // search from right to left, in the list the first pass left
        const TrList L{sq, o, n};
        int left, right;
        tr_anchor_r2l(L, set, max(0, n - 1 - clip), right, left, lane);
        rb_trim_pass ps = tr_pass(0, left, right, -1, -1);
        if (right > 0 && right - left >= k) {
            int cut = right - 1;
            int c = tr_run(L, right - k, -k, left + k, k, (right - left - 1) / k, lane);
            if (c > 0) cut = right - c * k;
            const int s0 = right - cut;
            c = tr_run(L, right - s0, -1, left + s0, 1, right - left - s0, lane);
            if (c > 0) cut = right - (s0 + c - 1);
            cut = max(cut, (right + left) / 2);
            ps.i2 = cut;
            int nb, ne;
            if (left < clip) {
                const int cl = right - cut;
                ps.i3 = cl;
                const uint32_t lmin = L.min_cov(cl, min(cl + k, n), lane), rmin = L.min_cov(max(0, cut - k), cut, lane);
                if (lmin > rmin) { ps.why = 1; nb = 0; ne = max(1, cut - k); }
                else { ps.why = 2; nb = min(cl + k, n - 1); ne = n; }
            } else { ps.why = 3; nb = 0; ne = max(1, cut - k); }
            o += nb; n = ne - nb;
        }
        rec.pass[1] = ps;
    }
    if (rec.pass[0].why || rec.pass[1].why) rec.flags |= RB_TRIM_FOUND;
    rec.begin = o; rec.end = o + n;
}

// the seven-argument overload (:7762-7916)
__device__ void tr_long(const TrArgs &a, const TrSeq &sq, const TrSet &set, rb_trim_rec &rec, uint32_t lane) {
    const int n = sq.nk, min_match = 2 * a.k, clip = a.clip;
    const float grad = a.grad;
    const TrList L{sq, 0, n};
    auto found = [&](int p, int why, int begin, int end) { rec.pass[p].why = why; rec.flags |= RB_TRIM_FOUND; rec.begin = begin; rec.end = end; };
    {   // scan from left to right
        int as, ps;
        tr_anchor_l2r(L, set, min(n, clip), as, ps, lane);
        int ae = as, pe = ps;
        if (as > 0) {
            const int mid = (as + ps) / 2;
            for (int i0 = as + 1; i0 < mid; i0 += 64) {
                const int s = i0 + (int)lane;
                unsigned long long m = __ballot(s < mid && set.has(L.rc(s)));
                while (m) {
                    const int i = i0 + (int)__builtin_ctzll(m);
                    m &= m - 1ull;
                    const int j = tr_scan_down(L, i, ps - 1, mid, lane);
                    if (j >= 0) { ae = i; ps = j; }
                }
            }
        }
        rec.pass[0] = tr_pass(0, as, ae, ps, pe);
        if (as > 0) {
            rec.pass[0].why = 1;
            if (ae - as >= min_match && pe - ps >= min_match) {
                ++ae; ++pe;
                if (a.stranded) {
                    const float anchor = L.median(as, ae, lane), middle = ae < ps ? L.median(ae, ps, lane) : 0.0f, partner = L.median(ps, pe, lane);
                    if (anchor < partner) {
                        if (middle >= anchor && middle >= partner * grad) found(0, 3, ae, n);
                        else found(0, 4, ps, n);
                    } else {
                        if (middle > partner && middle >= anchor * grad) found(0, 5, 0, ps);
                        else found(0, 6, 0, ae);
                    }
                } else found(0, 2, ae, ps);
                return;
            }
        }
    }
    {   // scan from right to left
        int as, ps;
        tr_anchor_r2l(L, set, max(0, n - clip), as, ps, lane);
        int ae = as, pe = ps;
        if (as > 0) {
            const int mid = (as + ps) / 2;
            for (int top = as - 1; top > mid; top -= 64) {
                const int s = top - (int)lane;
                unsigned long long m = __ballot(s > mid && set.has(L.rc(s)));
                while (m) {
                    const int i = top - (int)__builtin_ctzll(m);
                    m &= m - 1ull;
                    const int j = tr_scan_up(L, i, pe + 1, mid + 1, lane);
                    if (j >= 0) { as = i; pe = j; }
                }
            }
        }
        rec.pass[1] = tr_pass(0, as, ae, ps, pe);
        if (as > 0) {
            rec.pass[1].why = 1;
            if (ae - as >= min_match && pe - ps >= min_match) {
                ++ae; ++pe;
                if (a.stranded) {
                    const float partner = L.median(ps, pe, lane), middle = pe < as ? L.median(pe, as, lane) : 0.0f, anchor = L.median(as, ae, lane);
                    if (partner > anchor) {
                        if (middle > anchor && middle >= partner * grad) found(1, 3, 0, as);
                        else found(1, 4, 0, pe);
                    } else {
                        if (middle > partner && middle >= anchor * grad) found(1, 5, pe, n);
                        else found(1, 6, as, n);
                    }
                } else found(1, 2, pe, as);
            }
        }
    }
}

// NTP64RC of every k-mer of a sequence in a stranded graph, whose getKmers row R holds 0: a lane per stretch of windows, the first hashed
// base by base, the others rolled (R/bloom/hash/NTHash.java:133-166, as k_get_kmers rolls the reverse strand)
__device__ void tr_reverse_hashes(const TrArgs &a, const uint32_t *cw32, uint64_t *R, int nk, uint32_t lane) {
    const uint32_t uk = (uint32_t)a.k;
    const int per = (nk + 63) / 64, p0 = (int)lane * per, p1 = min(nk, p0 + per);
    if (p0 < nk) {
        uint64_t rv = 0;
        for (uint32_t q = 0; q < uk; ++q) rv ^= rotl_var(seed_of(3u - base_at(cw32, (uint32_t)p0 + q)), q);
        R[p0] = rv;
        for (int p = p0 + 1; p < p1; ++p) {
            const uint32_t out = base_at(cw32, (uint32_t)p - 1u), in = base_at(cw32, (uint32_t)p + uk - 1u);
            rv = rotr1(rv) ^ rotr1(seed_of(3u - out)) ^ rotl_var(seed_of(3u - in), uk - 1u);
            R[p] = rv;
        }
    }
    wave_fence();
}

__device__ __forceinline__ rb_trim_rec tr_blank(int flags, int nk, int mode) {
    rb_trim_rec rec;
    rec.flags = flags; rec.begin = 0; rec.end = nk; rec.mode = mode;
    rec.pass[0] = rb_trim_pass{-1, -1, -1, -1, -1}; rec.pass[1] = rec.pass[0];
    rec.reserved[0] = 0; rec.reserved[1] = 0;
    return rec;
}

// sequence r of the piece, by one wavefront; its table is its LDS row, or — a list longer than TR_LDS_LIST — its row of device scratch
__device__ void tr_one(const TrArgs &a, int64_t r, uint64_t *lds_tab, uint64_t *dev_tab, uint32_t lane) {
    const int64_t k0 = a.kof[r];
    const int nk = (int)(a.kof[r + 1] - k0);
    if (nk == 0 || wave_bad_letter(a.valid + a.woff[r], nk + a.k - 1, lane)) {    // not judged
        if (lane == 0) a.recs[r] = tr_blank(nk == 0 ? RB_SCREEN_NO_KMER : RB_SCREEN_BAD_LETTER, nk, a.mode);
        return;
    }
    const uint32_t *cw32 = reinterpret_cast<const uint32_t *>(a.codes + a.woff[r]);
    if (a.stranded) tr_reverse_hashes(a, cw32, a.R + k0, nk, lane);
    const TrSeq sq{cw32, a.F + k0, a.R + k0, a.cnt + k0, nk, a.k, a.stranded};
    uint64_t *tab = nk <= TR_LDS_LIST ? lds_tab : dev_tab;
    rb_trim_rec rec = tr_blank(0, nk, a.mode);
    if (a.mode == RB_TRIM_HASHES) tr_hashes(a, sq, tab, rec, lane);
    else {
        const TrSet set = tr_set_build(tab, nk, [&](int i) { return sq.hv(i); }, lane);
        if (a.mode == RB_TRIM_EDGE) tr_edge(a, sq, set, rec, lane);
        else tr_long(a, sq, set, rec, lane);
    }
    if (rec.begin > 0 || rec.end < nk) rec.flags |= RB_TRIM_TRIMMED;
    if (lane == 0) a.recs[r] = rec;
}

// A wavefront per sequence, taking sequences in turn
__global__ void __launch_bounds__(TR_TPB) k_trim_artifacts(TrArgs a, uint64_t *scratch) {
    __shared__ uint64_t s_tab[TR_WAVES][TR_LDS_SLOTS];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t slot = (int64_t)blockIdx.x * TR_WAVES + wv, n_slots = (int64_t)gridDim.x * TR_WAVES;
    uint64_t *dev_tab = scratch + (size_t)slot * (size_t)a.tab_cap;
    for (int64_t r = slot; r < a.pn; r += n_slots) {
        tr_one(a, r, s_tab[wv], dev_tab, lane);
        wave_fence();
    }
}

void trim_call(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, int mode, int max_edge_clip, float max_cov_gradient, rb_trim_rec *out) {
    const char *who = "rb_graph_trim_rc_artifacts";
    RB_REQUIRE(g, "%s: null handle", who);
    RB_REQUIRE(!g->shard, "%s: not available on a shard handle", who);
    RB_REQUIRE(g->dbg.bits && g->cbf, "%s: dbgbf or the counting filter has been destroyed", who);
    RB_REQUIRE(mode == RB_TRIM_HASHES || mode == RB_TRIM_EDGE || mode == RB_TRIM_LONG, "%s: mode = %d", who, mode);
    RB_REQUIRE(max_edge_clip >= 0 && max_edge_clip <= TR_MAX_CLIP, "%s: max_edge_clip out of range [0, %d]", who, TR_MAX_CLIP);
    RB_REQUIRE(std::isfinite(max_cov_gradient), "%s: max_cov_gradient is not finite", who);
    RB_REQUIRE(n >= 0, "%s: n = %lld", who, (long long)n);
    if (n == 0) return;
    RB_REQUIRE(offsets && out, "%s: null argument", who);
    const int k = g->k;
    std::vector<int64_t> ko((size_t)n + 1);
    kmer_offsets(offsets, n, k, ko.data(), who);
    RB_REQUIRE(offsets[n] == offsets[0] || seq, "%s: null sequence text", who);
    const int64_t longest = longest_list(ko, n);
    RB_REQUIRE(longest <= TR_MAX_LIST, "%s: a sequence of %lld k-mers (at most %d)", who, (long long)longest, TR_MAX_LIST);
    // what no kernel touches: the sequences of pieces without a k-mer
    for (int64_t i = 0; i < n; ++i) {
        rb_trim_rec &rc = out[i];
        rc.flags = RB_SCREEN_NO_KMER; rc.begin = 0; rc.end = 0; rc.mode = mode;
        rc.pass[0] = rb_trim_pass{-1, -1, -1, -1, -1}; rc.pass[1] = rc.pass[0];
        rc.reserved[0] = 0; rc.reserved[1] = 0;
    }
    if (ko[(size_t)n] == 0) return;
    RB_HIP(hipSetDevice(g->p.device));
    HostPin pin_r(out, (size_t)n * sizeof(rb_trim_rec));
    QueryLease q(g);
    RB_REQUIRE(g->dbg.bits && g->cbf, "%s: dbgbf or the counting filter has been destroyed", who);
    hipStream_t s = q.c->st;
    // a wavefront's table in device scratch, where the longest list does not fit the LDS row: twice its k-mers, rounded up to a power of two
    int64_t tab_cap = 0;
    if (longest > TR_LDS_LIST) { tab_cap = 64; while (tab_cap < 2 * longest) tab_cap <<= 1; }
    const int64_t max_slots = tab_cap ? std::max<int64_t>(4, std::min<int64_t>(TR_MAX_SLOTS, (int64_t)(TR_TAB_BUDGET / ((size_t)tab_cap * 8)))) : TR_MAX_SLOTS;
    TrArgs a{};
    a.stranded = (int)g->stranded; a.k = k; a.mode = mode; a.clip = max_edge_clip; a.tab_cap = (int)tab_cap; a.grad = max_cov_gradient;
    // piece by piece (rb_pieces.hpp): b0 the piece's k-mer offsets, b1 / b2 the getKmers hashes, b3 counts, records and the wavefronts'
    // tables; with profiling on the kernels of every piece are timed: entry "trim_artifacts"
    for_each_host_piece(g, s, seq, offsets, ko.data(), n, "trim_artifacts", [&](HostPiece &pc) {
        const int64_t ra = pc.ra, pn = pc.pn, pt = pc.pt;
        const int64_t slots = std::min<int64_t>(pn, max_slots);
        const unsigned blocks = blocks_for(slots, TR_WAVES);
        const size_t o_rec = up16((size_t)pt * 4), o_tab = up16(o_rec + (size_t)pn * sizeof(rb_trim_rec));
        q.c->b3.reserve(o_tab + (size_t)blocks * TR_WAVES * (size_t)tab_cap * 8 + 16);
        uint8_t *base3 = q.c->b3.as<uint8_t>();
        a.recs = reinterpret_cast<rb_trim_rec *>(base3 + o_rec);
        PieceRows(g, *q.c, pc).into(a);
        hipLaunchKernelGGL(k_trim_artifacts, dim3(blocks), dim3(TR_TPB), 0, s, a, reinterpret_cast<uint64_t *>(base3 + o_tab));
        RB_HIP(hipGetLastError());
        pc.kernels_end();
        RB_HIP(hipMemcpyAsync(out + ra, a.recs, (size_t)pn * sizeof(rb_trim_rec), hipMemcpyDeviceToHost, s));
    });
}

}  // namespace

extern "C" {
int rb_graph_trim_rc_artifacts(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, int mode, int max_edge_clip, float max_cov_gradient,
                               rb_trim_rec *out) {
    return guarded([&] { trim_call(g, seq, offsets, n, mode, max_edge_clip, max_cov_gradient, out); });
}
}  // extern "C"
