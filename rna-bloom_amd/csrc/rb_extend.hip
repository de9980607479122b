// rb_extend.hip — paired-k-mer branch extension of host sequences (rb_graph_extend_se): GraphUtils.extendRightSE / extendLeftSE
// (R/util/GraphUtils.java:6018-6204) over countKmerPairsSE / countKmerPairsReversedSE (:5718-5790) and naiveExtend{Right,Left}NoBackChecks
// (:6888-6933, :7067-7112), on the device.  Only the last min(n, d) k-mers of a sequence matter to the step, so the host hands the device
// the last (first, for the left-hand direction) d + k - 1 letters of every sequence; per piece the getKmers kernel leaves their hashes and
// counts in device scratch and k_extend_se runs the step, a wavefront per sequence: the up to 4 first-level and 16 second-level naive
// walks advance side by side, a lane per (walk, neighbour base), and the pair look-ups of a finished walk go a lane per walked k-mer.
// Nothing is written to the graph (DESIGN.md §5 "Branch extension").
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rb_pieces.hpp"
#include "rb_lookup.hpp"

using namespace rb;

// Java float arithmetic: the score is one float32 product and one float32 quotient, the median of an even number of counts one sum and one quotient
#pragma clang fp contract(off)

namespace {

constexpr int EX_TPB = 256;
constexpr int EX_WAVES = EX_TPB / 64;    // sequences a workgroup works on at a time: a wavefront each
constexpr int EX_LDS_D = 256;            // the largest read-paired k-mer distance whose walk rows live in LDS; a larger one keeps them in device scratch
constexpr int EX_SCRATCH_SLOTS = 4096;   // wavefronts of the scratch instantiation (each owns one row of device scratch and takes sequences in turn)
constexpr int EX_NO_GAP = 1 << 30;

// A wavefront's rows for distance capacity D: one count code (count_code_of) and one 2-bit base per walked k-mer — 4 first-level walks of
// at most D k-mers (candidate + d - 1), 16 second-level walks of at most D + 2 (next candidate + d - gap + 1, gap >= 1) — and the bases of
// the sequence's last k-mer, four a byte.
constexpr int ex_l1b_stride(int D) { return (D + 3) / 4; }
constexpr int ex_l2_cap(int D) { return D + 2; }
constexpr int ex_l2b_stride(int D) { return (D + 2 + 3) / 4; }
constexpr size_t ex_row_bytes(int D) {
    return ((size_t)4 * D + (size_t)16 * ex_l2_cap(D) + (size_t)4 * ex_l1b_stride(D) + (size_t)16 * ex_l2b_stride(D) + (RB_MAX_K + 3) / 4 + 15) & ~(size_t)15;
}
static_assert(ex_row_bytes(EX_LDS_D) * EX_WAVES * 4 <= 160 * 1024, "the rows of four workgroups must fit the CU's 160 KB of LDS (the kernel's registers, not LDS, set its occupancy: three wavefronts per SIMD)");

__device__ __forceinline__ uint32_t ex_get2(const uint8_t *row, int i) { return ((uint32_t)row[i >> 2] >> (2u * ((uint32_t)i & 3u))) & 3u; }
__device__ __forceinline__ void ex_put2(uint8_t *row, int i, uint32_t c) {
    const uint32_t s = 2u * ((uint32_t)i & 3u);
    row[i >> 2] = (uint8_t)(((uint32_t)row[i >> 2] & ~(3u << s)) | (c << s));
}
__device__ __forceinline__ uint64_t ex_shfl64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}

// The text a walk's k-mers are windows of, in walking order (for the left-hand direction the reverse of the sequence's orientation): the
// k bases of the sequence's last k-mer, then the bases of a first-level walk (its first `gap` k-mers; all of them when there is no second
// level), then those of a second-level walk.  K-mer j of the chain is bases [j + 1, j + k].
struct ExChain {
    const uint8_t *seed, *l1, *l2;
    int k, gap;
    __device__ __forceinline__ uint32_t base(int pos) const {
        if (pos < k) return ex_get2(seed, pos);
        pos -= k;
        return pos < gap ? ex_get2(l1, pos) : ex_get2(l2, pos - gap);
    }
    // is k-mer `a` of the chain followed by base nb the same k-mer as k-mer t?  (Kmer.equals: the bases)
    __device__ bool next_equals(int a, uint32_t nb, int t) const {
        bool eq = nb == base(t + k);
        for (int q = 0; q + 1 < k && eq; ++q) eq = base(a + 2 + q) == base(t + 1 + q);
        return eq;
    }
};

// Both strands of a k-mer, in walking order: A rolls like a forward hash along the walk, B like a reverse-strand hash.  A right-hand walk
// has (f, r) = (A, B) with A over the bases' seeds and B over their complements'; a left-hand walk adds bases at the k-mer's front, so its
// A is the k-mer's reverse-strand hash and its B the forward one: xm / ym turn a base into the code whose seed A / B take.
struct ExDir {
    int stranded, left;
    uint32_t uk, xm, ym;
    __device__ __forceinline__ uint64_t fwd(uint64_t A, uint64_t B) const { return left ? B : A; }
    __device__ __forceinline__ uint64_t hash(uint64_t A, uint64_t B) const { return stranded ? fwd(A, B) : smin(A, B); }
    // the neighbour that drops base `out` and takes base `in` (Successors / PredecessorsNTHashIterator)
    __device__ __forceinline__ void step(uint64_t A, uint64_t B, uint32_t out, uint32_t in, uint64_t &nA, uint64_t &nB) const {
        nA = rotl(A, 1) ^ rotl(seed_of(out ^ xm), uk) ^ seed_of(in ^ xm);
        nB = rotr(B, 1) ^ rotr(seed_of(out ^ ym), 1) ^ rotl(seed_of(in ^ ym), uk - 1u);
    }
};

// One naive walk (naiveExtend{Right,Left}NoBackChecks) as its four lanes hold it: lane (lane & 3) looks at neighbour base lane & 3.
struct ExWalk {
    uint64_t A, B, start_f;      // the k-mer the walk stands on; forward hash of the k-mer it started from
    int len, added, bound, cap;  // entries of its row (the start k-mer is entry 0), k-mers added, the reference's bound, room of the row
    int off;                     // chain index of row entry 0
    bool alive;
};

// Advances the wavefront's walks side by side until none is alive.  Per step and walk: the neighbours with count >= min_cov (hasDepth* is
// always true: rb_capi.h, rb_graph_naive_extend); none or several end it; the only one ends it, not added, when it equals the k-mer the
// walk started from or the one added last (:6919); else it is added and the walk ends once ++extensionLength > bound (:6925).
__device__ void ex_run_walks(const FilterView &fv, const ExDir &dr, float min_cov, const ExChain &ch, uint8_t *crow, uint8_t *brow, ExWalk &w, uint32_t lane) {
    const uint32_t in = lane & 3u;
    while (__ballot(w.alive)) {
        uint64_t nA = 0, nB = 0;
        uint32_t code = 0;
        bool pass = false;
        const int ci = w.off + w.len - 1;                        // chain index of the k-mer the walk stands on
        if (w.alive) {
            dr.step(w.A, w.B, ch.base(ci + 1), in, nA, nB);
            code = count_code(fv, dr.hash(nA, nB));
            pass = count_code_value(code) >= min_cov;
        }
        const uint32_t m4 = (uint32_t)(__ballot(pass) >> (lane & ~3u)) & 0xFu;
        const uint32_t bi = m4 ? (uint32_t)__builtin_ctz(m4) : 0u;
        const int src = (int)((lane & ~3u) | bi);
        const uint64_t bA = ex_shfl64(nA, src), bB = ex_shfl64(nB, src);
        const uint32_t bcode = (uint32_t)__shfl((int)code, src, 64);
        if (w.alive) {
            if (__popc(m4) != 1) w.alive = false;
            else {
                const uint64_t bf = dr.fwd(bA, bB);
                bool rep = bf == dr.fwd(w.A, w.B) && ch.next_equals(ci, bi, ci);
                rep = rep || (bf == w.start_f && ch.next_equals(ci, bi, w.off));
                // w.len >= w.cap never holds for a live walk: len = 1 + added and a walk dies once added = bound + 1, so len <= bound + 2 — d of
                // the first level's cap D >= d (bound d - 2), d - gap + 2 <= d + 1 of the second level's D + 2 (bound d - gap, gap >= 1).  The
                // comparison only keeps the stores below inside the row should that arithmetic ever be changed.
                if (rep || w.len >= w.cap) w.alive = false;
                else {
                    if (in == 0u) { crow[w.len] = (uint8_t)bcode; ex_put2(brow, w.len, bi); }
                    w.A = bA; w.B = bB;
                    ++w.len;
                    if (++w.added > w.bound) w.alive = false;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
}

// what the kernel reads of a sequence's last min(n, d) k-mers (the getKmers rows of the piece) — slot j counts from the oldest of them in
// the order of the reference's list (reversed for the left-hand direction), so the list's index numKmers - d + i is slot nt - d + i
struct ExTail {
    const uint64_t *F, *R;
    int nt, left;
    __device__ __forceinline__ int at(int j) const { return left ? nt - 1 - j : j; }
};

// countKmerPairsSE / countKmerPairsReversedSE with gap 0 over chain k-mers [i0, n): i runs to min(d - 1, n - 1), the partner is slot
// nt - d + i where that is not negative; k-mers below i0 are known to have no support (they were counted with the first level).  Each lane
// hashes its k-mer from the chain's bases (rotations by one only) and forms Kmer.getKmerPairHashValue (R/graph/Kmer.java:65-67,
// CanonicalKmer.java:61-72) with the partner on the side the direction puts it.
__device__ void ex_count_pairs(const PairView &pf, const ExDir &dr, const ExChain &ch, const ExTail &tl, int d, int n, int i0, uint32_t lane, int &pairs, int &last) {
    const int hi = min(d - 1, n - 1), k = (int)dr.uk;
    pairs = 0; last = -1;
    for (int base = i0; base <= hi; base += 64) {
        const int i = base + (int)lane, j = tl.nt - d + i;
        bool hit = false;
        if (i <= hi && j >= 0) {
            uint64_t A = 0, B = 0;
            for (int q = 0; q < k; ++q) {
                A = rotl(A, 1) ^ seed_of(ch.base(i + 1 + q) ^ dr.xm);
                B = rotl(B, 1) ^ seed_of(ch.base(i + k - q) ^ dr.ym);
            }
            const uint64_t f = dr.left ? B : A, r = dr.left ? A : B;
            const uint64_t pfw = tl.F[tl.at(j)], prv = dr.stranded ? 0ull : tl.R[tl.at(j)];
            uint64_t key;
            if (!dr.left) key = dr.stranded ? combine(pfw, f) : smin(combine(pfw, f), combine(r, prv));      // partner on the left
            else key = dr.stranded ? combine(f, pfw) : smin(combine(f, pfw), combine(prv, r));               // partner on the right
            hit = pair_hit(pf, key);
        }
        const unsigned long long m = __ballot(hit);
        if (m) { pairs += __popcll(m); last = base + 63 - (int)__builtin_clzll(m); }
    }
}

// count codes of a chain's k-mers: the first `gap` from a first-level row, the rest from a second-level row
struct ExCodes {
    const uint8_t *c1, *c2;
    int gap, n;
    __device__ __forceinline__ uint32_t at(int i) const { return i < gap ? c1[i] : c2[i - gap]; }
    __device__ __forceinline__ uint32_t operator()(int i) const { return at(i); }
};
// getMedianKmerCoverage(Collection) :229-247 of a chain's count codes
__device__ float ex_median(const ExCodes &cc, uint32_t lane) {
    return median_code(cc, cc.n, lane);
}

__device__ __forceinline__ void ex_put(rb_extend_rec *rec, int outcome, int why, int n_cand, int out_len, int pairs, int last, int winner, float score) {
    rb_extend_rec v;
    v.outcome = outcome; v.why = why; v.n_candidates = n_cand; v.out_len = out_len; v.pairs = pairs; v.last_partnered = last; v.winner = winner; v.score = score;
    *rec = v;
}

struct ExArgs {
    FilterView fv;
    PairView pf;
    int stranded, k, d, direction, D;        // D: the distance the rows are laid out for (EX_LDS_D in LDS, d in device scratch)
    int64_t pn;
    const int64_t *kof;                      // k-mer offsets of the piece's (cut) sequences
    const uint64_t *F, *R;                   // their getKmers rows
    const float *cnt;
    const uint64_t *codes;                   // the piece's batch: 2-bit codes and usable bits of its letters
    const uint32_t *valid, *woff;
    const float *floors;
    uint8_t *out_b;                          // [pn][d + 2]
    float *out_c;                            // [pn][d + 2] or nullptr
    rb_extend_rec *recs;
};

// the chain's first n k-mers as output: bases in walking order (upper-case A C G T) and, on request, counts
__device__ void ex_emit(const ExArgs &a, int64_t r, const ExChain &ch, const ExCodes &cc, int n, uint32_t lane) {
    const int64_t o = r * (int64_t)(a.d + 2);
    for (int i = (int)lane; i < n; i += 64) {
        const uint32_t b = ch.base(a.k + i);
        a.out_b[o + i] = code_letter(b);
        if (a.out_c) a.out_c[o + i] = count_code_value(cc.at(i));
    }
}

// extendRightSE / extendLeftSE of sequence r of the piece, by one wavefront with `row` for its walks
__device__ void ex_one(const ExArgs &a, int64_t r, uint8_t *row, uint32_t lane) {
    const int k = a.k, d = a.d, D = a.D;
    rb_extend_rec *rec = a.recs + r;
    const int64_t k0 = a.kof[r];
    const int nt = (int)(a.kof[r + 1] - k0);
    if (nt == 0) {                                            // shorter than k: the reference's callers never get here
        if (lane == 0) ex_put(rec, RB_EXT_NONE, RB_EXT_WHY_SHORT, 0, 0, 0, -1, -1, 0.0f);
        return;
    }
    const int S1 = ex_l1b_stride(D), S2 = ex_l2b_stride(D), C2 = ex_l2_cap(D);
    uint8_t *l1c = row, *l2c = l1c + 4 * D, *l1b = l2c + 16 * C2, *l2b = l1b + 4 * S1, *seed = l2b + 16 * S2;
    const ExDir dr{a.stranded, a.direction, (uint32_t)k, a.direction ? 3u : 0u, a.direction ? 0u : 3u};
    const ExTail tl{a.F + k0, a.R + k0, nt, a.direction};
    const uint32_t in = lane & 3u;

    // the last k-mer's bases in walking order, four a byte (lane l packs bases 4 l .. 4 l + 3); one outside ACGTU ends the sequence
    {
        const uint64_t *cw = a.codes + a.woff[r];
        const uint32_t *vw = a.valid + a.woff[r];
        uint32_t byte = 0;
        bool bad = false;
        for (int j = 0; j < 4; ++j) {
            const int q = 4 * (int)lane + j;
            if (q < k) {
                const uint32_t p = (uint32_t)(a.direction ? k - 1 - q : nt - 1 + q);
                bad = bad || !((vw[p >> 5] >> (p & 31u)) & 1u);
                byte |= ((uint32_t)(cw[p >> 5] >> (2u * (p & 31u))) & 3u) << (2 * j);
            }
        }
        if (4 * (int)lane < k) seed[lane] = (uint8_t)byte;
        if (__ballot(bad)) {
            if (lane == 0) ex_put(rec, RB_EXT_NONE, RB_EXT_WHY_INVALID_SEED, 0, 0, 0, -1, -1, 0.0f);
            return;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const float min_cov = a.floors[r];

    // candidates: neighbours of the last k-mer with count >= 1, whatever the floor (Kmer.getSuccessors(k, numHash, graph), R/graph/Kmer.java:228-230)
    const int sp = tl.at(nt - 1);
    const uint64_t sf = tl.F[sp], sr = a.stranded ? 0ull : tl.R[sp];
    const uint64_t A0 = a.direction ? sr : sf, B0 = a.direction ? sf : sr;
    const ExChain ch0{seed, l1b, l1b, k, EX_NO_GAP};
    uint64_t nA = 0, nB = 0;
    uint32_t code = 0;
    if (lane < 4u) {
        dr.step(A0, B0, ch0.base(0), in, nA, nB);
        code = count_code(a.fv, dr.hash(nA, nB));
    }
    const uint32_t mask0 = (uint32_t)__ballot(lane < 4u && code >= 1u) & 0xFu;
    const int n_cand = __popc(mask0);
    if (n_cand == 0) {
        if (lane == 0) ex_put(rec, RB_EXT_NONE, RB_EXT_WHY_NO_CANDIDATE, 0, 0, 0, -1, -1, 0.0f);
        return;
    }

    // first level: candidate c's walk is held by lanes 4 c .. 4 c + 3 and fills first-level row c, bound d - 2 (:6026)
    const uint32_t c1 = (lane >> 2) & 3u;
    ExWalk w1;
    w1.A = ex_shfl64(nA, (int)c1); w1.B = ex_shfl64(nB, (int)c1);
    const uint32_t code1 = (uint32_t)__shfl((int)code, (int)c1, 64);
    w1.alive = lane < 16u && ((mask0 >> c1) & 1u);
    w1.start_f = dr.fwd(w1.A, w1.B);
    w1.len = 1; w1.added = 0; w1.bound = d - 2; w1.cap = D; w1.off = 0;
    uint8_t *crow1 = l1c + c1 * D, *brow1 = l1b + c1 * S1;
    if (w1.alive && in == 0u) { crow1[0] = (uint8_t)code1; ex_put2(brow1, 0, c1); }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const ExChain ch1{seed, brow1, brow1, k, EX_NO_GAP};
    ex_run_walks(a.fv, dr, min_cov, ch1, crow1, brow1, w1, lane);
    int len1[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) len1[c] = __shfl(w1.len, 4 * c, 64);

    if (n_cand == 1) {                                        // :6030-6035: the only candidate and its walk, unscored and untrimmed
        const int c = __builtin_ctz(mask0), n = len1[c];
        ex_emit(a, r, ExChain{seed, l1b + c * S1, l1b + c * S1, k, EX_NO_GAP}, ExCodes{l1c + c * D, l1c + c * D, EX_NO_GAP, n}, n, lane);
        if (lane == 0) ex_put(rec, RB_EXT_SINGLE, RB_EXT_WHY_FOUND, 1, n, 0, -1, c, 0.0f);
        return;
    }

    // pathMinCov: the minimum count of the last min(n, d) k-mers (:6037)
    float path_min = INFINITY;
    for (int p = (int)lane; p < nt; p += 64) path_min = fminf(path_min, a.cnt[k0 + p]);
    for (int s = 32; s > 0; s >>= 1) path_min = fminf(path_min, __shfl_xor(path_min, s, 64));

    // the first stretches' pairs (:6047); an unsupported stretch shorter than d - 1 goes one branch further (:6067-6076)
    int pairs1[4], last1[4];
    uint32_t l2mask = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        pairs1[c] = 0; last1[c] = -1;
        if ((mask0 >> c) & 1u) {
            ex_count_pairs(a.pf, dr, ExChain{seed, l1b + c * S1, l1b + c * S1, k, EX_NO_GAP}, tl, d, len1[c], 0, lane, pairs1[c], last1[c]);
            if (pairs1[c] == 0 && len1[c] < d - 1) l2mask |= 1u << c;
        }
    }

    // second level: the successors (count >= 1) of a first stretch's last k-mer — lane 4 c + c2 of the first-level lanes finds candidate
    // (c, c2), which is second-level walk 4 c + c2, held by lanes 16 c + 4 c2 .. + 3, bound d - gap (:6079)
    uint32_t mask2 = 0;
    ExWalk w2;
    w2.alive = false; w2.len = 0;
    const uint32_t wid = lane >> 2, c2p = lane >> 4;          // this lane's second-level walk and its first-level parent
    const int gap = __shfl(w1.len, (int)(4u * c2p), 64);
    uint8_t *crow2 = l2c + wid * C2, *brow2 = l2b + wid * S2;
    const ExChain ch2{seed, l1b + c2p * S1, brow2, k, gap};
    if (l2mask) {
        const bool probe = lane < 16u && ((l2mask >> c1) & 1u);
        code = 0;
        if (probe) {
            dr.step(w1.A, w1.B, ch1.base(w1.len), in, nA, nB);
            code = count_code(a.fv, dr.hash(nA, nB));
        }
        mask2 = (uint32_t)__ballot(probe && code >= 1u) & 0xFFFFu;
        w2.A = ex_shfl64(nA, (int)wid); w2.B = ex_shfl64(nB, (int)wid);
        const uint32_t code2 = (uint32_t)__shfl((int)code, (int)wid, 64);
        w2.alive = (mask2 >> wid) & 1u;
        w2.start_f = dr.fwd(w2.A, w2.B);
        w2.len = 1; w2.added = 0; w2.bound = d - gap; w2.cap = C2; w2.off = gap;
        if (w2.alive && in == 0u) { crow2[0] = (uint8_t)code2; ex_put2(brow2, 0, wid & 3u); }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        ex_run_walks(a.fv, dr, min_cov, ch2, crow2, brow2, w2, lane);
    }

    // scores in the reference's order: candidate c's first stretch where it is supported, else its second-level extensions (:6051-6105)
    float best = 0.0f, best_cov = 0.0f;
    int b_level = 0, b_win = -1, b_len = 0, b_pairs = 0, b_last = -1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (!((mask0 >> c) & 1u)) continue;
        if (pairs1[c] > 0) {
            const float cov = ex_median(ExCodes{l1c + c * D, l1c + c * D, EX_NO_GAP, len1[c]}, lane);
            const float score = fminf(path_min, cov) * (float)pairs1[c] / (float)(last1[c] + 1);
            if (score > best || (score == best && cov > best_cov)) {
                best = score; best_cov = cov; b_level = 1; b_win = c; b_len = last1[c] + 1; b_pairs = pairs1[c]; b_last = last1[c];
            }
        } else if ((l2mask >> c) & 1u) {
            for (int c2 = 0; c2 < 4; ++c2) {
                const int w = 4 * c + c2;
                if (!((mask2 >> w) & 1u)) continue;
                const int n = len1[c] + __shfl(w2.len, 4 * w, 64);
                int pairs, last;
                ex_count_pairs(a.pf, dr, ExChain{seed, l1b + c * S1, l2b + w * S2, k, len1[c]}, tl, d, n, len1[c], lane, pairs, last);
                if (pairs == 0) continue;
                const float cov = ex_median(ExCodes{l1c + c * D, l2c + w * C2, len1[c], n}, lane);
                const float score = fminf(path_min, cov) * (float)pairs / (float)(last + 1);
                if (score > best || (score == best && cov > best_cov)) {
                    best = score; best_cov = cov; b_level = 2; b_win = c | (c2 << 4); b_len = last + 1; b_pairs = pairs; b_last = last;
                }
            }
        }
    }
    if (b_level == 0) {
        if (lane == 0) ex_put(rec, RB_EXT_NONE, RB_EXT_WHY_NO_SUPPORT, n_cand, 0, 0, -1, -1, 0.0f);
        return;
    }
    // the winner, trimmed to its last supported k-mer (:6060-6064)
    const int c = b_win & 3, w = 4 * c + (b_win >> 4);
    if (b_level == 1) ex_emit(a, r, ExChain{seed, l1b + c * S1, l1b + c * S1, k, EX_NO_GAP}, ExCodes{l1c + c * D, l1c + c * D, EX_NO_GAP, b_len}, b_len, lane);
    else ex_emit(a, r, ExChain{seed, l1b + c * S1, l2b + w * S2, k, len1[c]}, ExCodes{l1c + c * D, l2c + w * C2, len1[c], b_len}, b_len, lane);
    if (lane == 0) ex_put(rec, b_level == 1 ? RB_EXT_FIRST : RB_EXT_SECOND, RB_EXT_WHY_FOUND, n_cand, b_len, b_pairs, b_last, b_win, best);
}

// A wavefront per sequence, taking sequences in turn.  LDS_ROW: the wavefront's rows are in LDS (d <= EX_LDS_D); else in its slot of `scratch`.
template <bool LDS_ROW>
__global__ void __launch_bounds__(EX_TPB) k_extend_se(ExArgs a, uint8_t *scratch, size_t row_bytes) {
    __shared__ __attribute__((aligned(16))) uint8_t s_row[EX_WAVES][LDS_ROW ? ex_row_bytes(EX_LDS_D) : 16];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t slot = (int64_t)blockIdx.x * EX_WAVES + wv, n_slots = (int64_t)gridDim.x * EX_WAVES;
    uint8_t *row;
    if constexpr (LDS_ROW) row = s_row[wv]; else row = scratch + (size_t)slot * row_bytes;
    for (int64_t r = slot; r < a.pn; r += n_slots) {
        ex_one(a, r, row, lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
}

inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

}  // namespace

extern "C" {
int rb_graph_extend_se(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, int direction, const float *min_kmer_cov, char *out_bases,
                       float *out_count, rb_extend_rec *recs) {
    return guarded([&] {
        RB_REQUIRE(g, "rb_graph_extend_se: null handle");
        RB_REQUIRE(!g->shard, "rb_graph_extend_se: not available on a shard handle");
        RB_REQUIRE(g->dbg.bits && g->cbf, "rb_graph_extend_se: dbgbf or the counting filter has been destroyed");
        RB_REQUIRE(g->rpk.bits, "rb_graph_extend_se: the graph has no read-paired k-mer filter (created without useReadPairedKmers, or destroyed)");
        const int d = g->read_d, k = g->k;
        RB_REQUIRE(d >= 2, "rb_graph_extend_se: the read-paired k-mer distance is %d (the step needs d >= 2)", d);
        RB_REQUIRE(direction == 0 || direction == 1, "rb_graph_extend_se: direction must be 0 (right) or 1 (left), not %d", direction);
        RB_REQUIRE(n >= 0, "rb_graph_extend_se: n = %lld", (long long)n);
        if (n == 0) return;
        RB_REQUIRE(offsets && min_kmer_cov && out_bases && recs, "rb_graph_extend_se: null argument");
        std::vector<int64_t> ko((size_t)n + 1), to((size_t)n + 1, 0);
        kmer_offsets(offsets, n, k, ko.data(), "rb_graph_extend_se");
        RB_REQUIRE(offsets[n] == offsets[0] || seq, "rb_graph_extend_se: null sequence text");
        for (int64_t i = 0; i < n; ++i)
            RB_REQUIRE(std::isfinite(min_kmer_cov[i]) && min_kmer_cov[i] >= 0.0f, "rb_graph_extend_se: min_kmer_cov[%lld] must be finite and not negative", (long long)i);
        // the step reads the last min(nk, d) k-mers of a sequence only: the device gets the d + k - 1 letters at the end it extends
        const int64_t keep = (int64_t)d + k - 1, stride = (int64_t)d + 2;
        for (int64_t i = 0; i < n; ++i) to[(size_t)i + 1] = to[(size_t)i] + std::min(offsets[i + 1] - offsets[i], keep);
        std::vector<char> text((size_t)to[(size_t)n]);
        for (int64_t i = 0; i < n; ++i) {
            const int64_t len = offsets[i + 1] - offsets[i], take = to[(size_t)i + 1] - to[(size_t)i];
            if (take) memcpy(text.data() + to[(size_t)i], seq + (direction ? offsets[i] : offsets[i] + len - take), (size_t)take);
        }
        kmer_offsets(to.data(), n, k, ko.data(), nullptr);
        // what no kernel touches: sequences of pieces without a k-mer, rows past a result's length
        for (int64_t i = 0; i < n; ++i) {
            rb_extend_rec &v = recs[i];
            v.outcome = RB_EXT_NONE; v.why = RB_EXT_WHY_SHORT; v.n_candidates = 0; v.out_len = 0; v.pairs = 0; v.last_partnered = -1; v.winner = -1; v.score = 0.0f;
        }
        memset(out_bases, 0, (size_t)(n * stride));
        if (out_count) memset(out_count, 0, (size_t)(n * stride) * 4);
        if (ko[(size_t)n] == 0) return;
        RB_HIP(hipSetDevice(g->p.device));
        HostPin pin_b(out_bases, (size_t)(n * stride)), pin_c(out_count, out_count ? (size_t)(n * stride) * 4 : 0), pin_r(recs, (size_t)n * sizeof(rb_extend_rec));
        QueryLease q(g);
        hipStream_t s = q.c->st;
        const bool lds = d <= EX_LDS_D;
        const size_t row_bytes = ex_row_bytes(lds ? EX_LDS_D : d);
        // piece by piece (rb_pieces.hpp): b0 the piece's k-mer offsets, b1 / b2 the getKmers hashes, b3 counts, floors, records, results and — for a
        // distance past the LDS row — the wavefronts' walk rows; with profiling on the kernels of every piece are timed: entry "extend_se"
        std::vector<int64_t> tab;
        for_each_host_piece(g, s, text.data(), to.data(), ko.data(), n, "extend_se", [&](HostPiece &pc) {
            const int64_t ra = pc.ra, pn = pc.pn, pt = pc.pt;
            tab.assign((size_t)pn + 1, 0);
            for (int64_t i = 0; i <= pn; ++i) tab[(size_t)i] = ko[(size_t)(ra + i)] - ko[(size_t)ra];
            const rb_batch *b = pc.batch();
            const int64_t slots = lds ? pn : std::min<int64_t>(pn, EX_SCRATCH_SLOTS);
            const unsigned blocks = blocks_for(slots, EX_WAVES);
            const size_t o_fl = up16((size_t)pt * 4), o_rec = up16(o_fl + (size_t)pn * 4), o_b = o_rec + (size_t)pn * sizeof(rb_extend_rec),
                         o_c = up16(o_b + (size_t)(pn * stride)), o_row = up16(o_c + (out_count ? (size_t)(pn * stride) * 4 : 0));
            q.c->b0.reserve(tab.size() * 8);
            q.c->b1.reserve((size_t)pt * 8);
            q.c->b2.reserve((size_t)pt * 8);
            q.c->b3.reserve(o_row + (lds ? 0 : (size_t)blocks * EX_WAVES * row_bytes) + 16);
            uint8_t *base3 = q.c->b3.as<uint8_t>();
            ExArgs a;
            a.fv = g->view(0, 0);
            a.pf = PairView{g->rpk.bits, g->rpk.mod, g->rpk.num_hash, kmul_of(k)};
            a.stranded = (int)g->stranded; a.k = k; a.d = d; a.direction = direction; a.D = lds ? EX_LDS_D : d;
            a.pn = pn;
            a.kof = q.c->b0.as<int64_t>();
            a.F = q.c->b1.as<uint64_t>(); a.R = q.c->b2.as<uint64_t>();
            a.cnt = reinterpret_cast<float *>(base3);
            a.codes = b->codes; a.valid = b->valid; a.woff = b->woff;
            a.floors = reinterpret_cast<float *>(base3 + o_fl);
            a.recs = reinterpret_cast<rb_extend_rec *>(base3 + o_rec);
            a.out_b = base3 + o_b;
            a.out_c = out_count ? reinterpret_cast<float *>(base3 + o_c) : nullptr;
            RB_HIP(hipMemcpyAsync(q.c->b0.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
            RB_HIP(hipMemcpyAsync(base3 + o_fl, min_kmer_cov + ra, (size_t)pn * 4, hipMemcpyHostToDevice, s));
            RB_HIP(hipMemsetAsync(base3 + o_b, 0, o_row - o_b, s));        // (what no wavefront writes comes back as zeros, whatever the cuts)
            pc.kernels_begin();
            rb::launch_get_kmers(g, b, a.kof, q.c->b1.as<uint64_t>(), q.c->b2.as<uint64_t>(), reinterpret_cast<float *>(base3), s);
            if (lds) hipLaunchKernelGGL((k_extend_se<true>), dim3(blocks), dim3(EX_TPB), 0, s, a, (uint8_t *)nullptr, row_bytes);
            else hipLaunchKernelGGL((k_extend_se<false>), dim3(blocks), dim3(EX_TPB), 0, s, a, base3 + o_row, row_bytes);
            RB_HIP(hipGetLastError());
            pc.kernels_end();
            RB_HIP(hipMemcpyAsync(recs + ra, a.recs, (size_t)pn * sizeof(rb_extend_rec), hipMemcpyDeviceToHost, s));
            RB_HIP(hipMemcpyAsync(out_bases + ra * stride, a.out_b, (size_t)(pn * stride), hipMemcpyDeviceToHost, s));
            if (out_count) RB_HIP(hipMemcpyAsync(out_count + ra * stride, a.out_c, (size_t)(pn * stride) * 4, hipMemcpyDeviceToHost, s));
        });
    });
}
}  // extern "C"
