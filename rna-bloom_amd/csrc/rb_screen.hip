// rb_screen.hip — the fragment screens of the transcript assembler's worker on the device: rb_graph_screen_fragments = GraphUtils.isBranchFree
// (R/util/GraphUtils.java:7651-7672), isChimera (:7674-7760) and isBluntEndArtifact (:8535-8586) of host sequences, with what they call: the
// gated getMaxCoveragePath (:1677-1776), the gated greedyExtendRight / Left (:1978-1997, :1940-1959) over greedyExtend{Right,Left}Once
// (:535-562, :598-625) and getMaxMedianCoverage{Right,Left} (:312-373, :438-499), and the four static hasDepthRight / hasDepthLeft
// (:6680-6778).  Per piece the getKmers kernel leaves the sequences' hashes and counts in device scratch and k_screen runs the screens, a
// wavefront per sequence: lanes first take the sequence's k-mers side by side (gate bit, variants), the reference's sequential scans then
// run over ballots of the gate bits, and every walk advances with a lane per neighbour base and — where several neighbours pass — a lane
// per candidate for the lookahead's depth-first search.  Nothing is written to the graph or the gate (DESIGN.md §5 "Fragment screens").
//   rb_graph_represented = GraphUtils.represented (:711-824), the worker's screen between isBranchFree and isChimera, is k_represented: the same
// prologue, rows, walks, paths and depth searches, and SeqUtils.getPercentIdentity (rb_align.hpp) of every edge walk and gap path that has the
// expected length (DESIGN.md §5 "Represented").
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rb_pieces.hpp"
#include "rb_lookup.hpp"
#include "rb_repeat.hpp"
#include "rb_align.hpp"
#include "rb_wave.hpp"

using namespace rb;

// Java float arithmetic: the median of an even number of counts is one float32 sum and one quotient
#pragma clang fp contract(off)

namespace {

constexpr int SC_TPB = 256;
constexpr int SC_WAVES = SC_TPB / 64;     // sequences a workgroup works on at a time: a wavefront each
constexpr int SC_MAX_SLOTS = 2048;        // wavefronts of a launch at the most (each owns one set of walk rows in device scratch and takes sequences in turn)
constexpr int SC_GREEDY_BOUND = 1000;     // isChimera's greedyExtendRight / Left bound (:7746-7748)
constexpr int SC_MAX_LOOKAHEAD = 16;      // rb_graph_greedy_extend's cap
constexpr int SC_MAX_DEPTH = 1 << 20;     // the largest max_depth taken (rb_graph_greedy_extend's largest bound)
constexpr int SC_MAX_ROW = 1 << 24;       // represented's walk rows grow with the longest sequence: entries of one at the most
constexpr int SC_MAX_INDEL = 4096;        // the largest max_indel taken by represented (rb_graph_correct_errors' cap; the reference's default is 1)
constexpr size_t SC_ROW_BUDGET = (size_t)512 << 20;   // device scratch all wavefronts' rows may take together (at least 16 wavefronts run whatever a row costs)

// One level of a candidate's depth-first search (getMaxMedianCoverage*): the path's k-mer at this level (both strands' hashes in walking order,
// count code, the base it added) and — the reference's `frontier` — the siblings behind it that have not been tried: their bases as a mask
// and their count codes a byte each.  A lane's search keeps its levels in LDS.
struct ScLevel { uint64_t A, B; uint8_t code, base, fmask, pad; uint32_t fcodes; };
static_assert(sizeof(ScLevel) == 24, "ScLevel is 24 bytes");
constexpr int SC_LEVELS = SC_MAX_LOOKAHEAD + 1;

using Dir = WaveDir<true>;               // a walk's direction, its rotations by k out of funnel shifts (rb_wave.hpp: k_screen's registers)

struct ScGate { const uint32_t *bits; Mod mod; int num_hash; };       // the gate's dbgbf: BloomFilter assembledKmers

struct ScArgs {
    FilterView fv;
    ScGate gate;
    uint64_t kmul;
    int stranded, k, what, lookahead, max_depth, read_d, cap, max_visits;   // cap: entries of a walk row
    int max_indel;                           // represented: maxIndelSize, percentIdentity (max_depth is its maxEdgeClipLength)
    float percent_identity;
    int64_t pn;
    const int64_t *kof;                      // k-mer offsets of the piece's sequences
    const uint64_t *F, *R;                   // their getKmers rows
    const float *cnt;
    uint8_t *gbit;                           // [pt] a k-mer's gate bit, filled by the sequence's wavefront
    const uint64_t *codes;                   // the piece's batch: 2-bit codes and usable bits of its letters
    const uint32_t *valid, *woff;
    rb_screen_rec *recs;
    rb_repr_rec *reprs;                      // represented's records instead
};

// A wavefront's rows in device scratch, `cap` entries each: two rows of hashes (the forward hashes of the k-mers a walk added — Kmer.equals
// candidates; a depth search keeps its stack's two strands there), two rows of text (a walk's k-mers are windows of it, in walking order:
// the k bases of its first k-mer, then a base per added k-mer; a byte a base) and the depth search's untried siblings, a mask per level.
constexpr size_t sc_row_bytes(int cap, int k) { return ((size_t)16 * cap + (size_t)2 * (cap + k) + (size_t)cap + 15) & ~(size_t)15; }
struct ScRows {
    uint64_t *h[2];
    uint8_t *tx[2], *mk;
    __device__ ScRows(uint8_t *row, int cap, int k) {
        h[0] = reinterpret_cast<uint64_t *>(row); h[1] = h[0] + cap;
        tx[0] = reinterpret_cast<uint8_t *>(h[1] + cap); tx[1] = tx[0] + cap + k; mk = tx[1] + cap + k;
    }
};

// One neighbour of the k-mer (A, B): its hashes and its count code, 0 where it does not count — the gated getSuccessors / getPredecessors
// (R/graph/Kmer.java:257-299: bf.lookup first, then graph.getCount > 0) or the plain one (:199-255 with minKmerCov 1: getCount >= 1; a
// present k-mer counts at least 1, so both are "the count code is not 0")
__device__ __forceinline__ uint32_t sc_neighbor(const ScArgs &a, const Dir &dr, bool gated, uint64_t A, uint64_t B, uint32_t out, uint32_t in, uint64_t &nA,
                                                uint64_t &nB) {
    dr.step(A, B, out, in, nA, nB);
    const uint64_t h = dr.hash(nA, nB);
    if (gated && !bits_lookup(a.gate.bits, a.gate.mod, a.gate.num_hash, a.kmul, h)) return 0u;
    return count_code(a.fv, h);
}
// ... all four by lanes 0 .. 3 (lane l keeps neighbour base l): the mask of those that count, for every lane
struct ScNb { uint64_t A, B; uint32_t code; };
__device__ __forceinline__ uint32_t sc_neighbors(const ScArgs &a, const Dir &dr, bool gated, uint64_t A, uint64_t B, uint32_t out, uint32_t lane, ScNb &nb) {
    nb.A = 0; nb.B = 0; nb.code = 0;
    if (lane < 4u) nb.code = sc_neighbor(a, dr, gated, A, B, out, lane, nb.A, nb.B);
    return (uint32_t)__ballot(lane < 4u && nb.code != 0u) & 0xFu;
}

// getMaxMedianCoverageRight / Left(graph, source, lookahead, bf) (:312-373, :438-499) of the candidate (cA, cB) by ONE lane, as a count code
// (codes order as their counts do, 0 is the count 0): the best minimum over the depth-first paths of exactly `lookahead` k-mers from the
// candidate.  The candidate is the k-mer behind chain k-mer `at` of the text tx (ntext bases); st[0 .. SC_LEVELS) is the lane's stack.
// With psize = path.size() and depth = frontier.size(), psize == depth + 1 at the head of the reference's outer loop and level j of the
// path is chain k-mer at + 1 + j, whose leaving base is text position at + 1 + j — a base of tx, or one the path itself added.
__device__ uint32_t sc_lookahead_score(const ScArgs &a, const Dir &dr, const uint8_t *tx, int at, int ntext, ScLevel *st, uint64_t cA, uint64_t cB,
                                       uint32_t ccode, uint32_t cbase) {
    auto base = [&](int pos) -> uint32_t { return pos < ntext ? (uint32_t)tx[pos] : (uint32_t)st[pos - ntext].base; };
    auto nbrs = [&](uint64_t A, uint64_t B, uint32_t out, uint32_t &codes4) -> uint32_t {
        uint32_t m = 0;
        codes4 = 0;
        for (uint32_t in = 0; in < 4u; ++in) {
            uint64_t nA, nB;
            const uint32_t c = sc_neighbor(a, dr, true, A, B, out, in, nA, nB);
            if (c) { m |= 1u << in; codes4 |= c << (8u * in); }
        }
        return m;
    };
    // path[j + 1] = the first untried child of path[j]; the rest of them stays at level j
    auto descend = [&](int j, uint32_t m, uint32_t codes4) {
        const uint32_t b = (uint32_t)__builtin_ctz(m);
        uint64_t nA, nB;
        dr.step(st[j].A, st[j].B, base(at + 1 + j), b, nA, nB);
        st[j].fmask = (uint8_t)(m & (m - 1u)); st[j].fcodes = codes4;
        st[j + 1].A = nA; st[j + 1].B = nB; st[j + 1].code = (uint8_t)((codes4 >> (8u * b)) & 0xFFu); st[j + 1].base = (uint8_t)b; st[j + 1].fmask = 0;
    };
    st[0].A = cA; st[0].B = cB; st[0].code = (uint8_t)ccode; st[0].base = (uint8_t)cbase; st[0].fmask = 0; st[0].fcodes = 0;
    uint32_t codes4;
    uint32_t m = nbrs(cA, cB, base(at + 1), codes4);
    if (!m) return a.lookahead > 0 ? 0u : ccode;
    descend(0, m, codes4);
    uint32_t best = 0;
    int depth = 1;
    while (depth > 0) {
        if (depth + 1 < a.lookahead) {
            m = nbrs(st[depth].A, st[depth].B, base(at + 1 + depth), codes4);
            if (m) { descend(depth, m, codes4); ++depth; continue; }
        }
        if (depth + 1 == a.lookahead) {                          // (we only calculate coverage if path is long enough)
            uint32_t mn = st[0].code;
            for (int j = 1; j <= depth; ++j) mn = min(mn, (uint32_t)st[j].code);
            best = max(best, mn);
        }
        while (depth > 0) {                                      // path.removeLast(), then the next sibling of the deepest level that has one
            const uint32_t fm = st[depth - 1].fmask;
            if (!fm) --depth;
            else { descend(depth - 1, fm, st[depth - 1].fcodes); break; }
        }
    }
    return best;
}

// One gated greedy step from chain k-mer `at` = (A, B) of the text tx — greedyExtend{Right,Left}Once(graph, source, lookahead, bf), which is
// also a step of the gated getMaxCoveragePath (:1696-1708: a single neighbour is taken as is, several go through greedyExtend*Once with the
// candidates at hand): no neighbour, the only one, or the candidate with the best lookahead score, a tie going to the strictly larger
// count (:547-559).  The text holds at + k bases.
struct ScPick { uint64_t A, B; uint32_t base; bool any; };
__device__ ScPick sc_greedy_step(const ScArgs &a, const Dir &dr, const uint8_t *tx, int at, uint64_t A, uint64_t B, ScLevel *dfs, uint32_t lane) {
    ScNb nb;
    const uint32_t mask = sc_neighbors(a, dr, true, A, B, tx[at], lane, nb);
    ScPick p{0, 0, 0, mask != 0u};
    if (!mask) return p;
    uint32_t bi = (uint32_t)__builtin_ctz(mask);
    if (mask & (mask - 1u)) {
        uint32_t score = 0;
        if (lane < 4u && ((mask >> lane) & 1u)) score = sc_lookahead_score(a, dr, tx, at, at + a.k, dfs + lane * SC_LEVELS, nb.A, nb.B, nb.code, lane);
        int best = -1;
        uint32_t best_code = 0;
        for (uint32_t c = 0; c < 4u; ++c) {
            const int s = __shfl((int)score, (int)c, 64);
            const uint32_t cc = (uint32_t)__shfl((int)nb.code, (int)c, 64);
            if (!((mask >> c) & 1u)) continue;
            if (s > best) { best = s; bi = c; best_code = cc; }
            else if (s == best && cc > best_code) { bi = c; best_code = cc; }
        }
    }
    p.A = wave_shfl64(nb.A, (int)bi); p.B = wave_shfl64(nb.B, (int)bi); p.base = bi;
    return p;
}

// what the wavefront reads of its sequence
struct ScSeq {
    const uint32_t *cw32;
    const uint64_t *F, *R;
    const float *cnt;
    const uint8_t *gbit;
    int nk, stranded;
    __device__ __forceinline__ uint32_t base(int p) const { return base_at(cw32, (uint32_t)p); }
    __device__ __forceinline__ uint32_t code(int i) const { return count_code_of(cnt[i]); }
};

// a walk from k-mer s of the sequence: its text's first k bases in walking order, its hashes
__device__ void sc_walk_begin(const ScArgs &a, const ScSeq &sq, const Dir &dr, int s, uint8_t *tx, uint64_t &A, uint64_t &B, uint32_t lane) {
    for (int q = (int)lane; q < a.k; q += 64) tx[q] = (uint8_t)sq.base(dr.left ? s + a.k - 1 - q : s + q);
    const uint64_t f = sq.F[s], r = a.stranded ? 0ull : sq.R[s];
    A = dr.left ? r : f; B = dr.left ? f : r;
    wave_fence();
}
// Kmer.equals of chain k-mer c of a walk's text and k-mer s of the sequence: the forward hashes first (unequal hashes: unequal bases), then the bases
__device__ bool sc_equals_seq(const ScArgs &a, const ScSeq &sq, const Dir &dr, const uint8_t *tx, int c, uint64_t f, int s, uint32_t lane) {
    if (f != sq.F[s]) return false;
    bool ne = false;
    for (int q = (int)lane; q < a.k; q += 64) ne = ne || (uint32_t)tx[c + q] != sq.base(dr.left ? s + a.k - 1 - q : s + q);
    return __ballot(ne) == 0ull;
}
// ... of chain k-mer c of text tc and chain k-mer e of text te; rev: the two texts walk in opposite directions
__device__ bool sc_equals_chain(int k, const uint8_t *tc, int c, const uint8_t *te, int e, bool rev, uint32_t lane) {
    bool ne = false;
    for (int q = (int)lane; q < k; q += 64) ne = ne || tc[c + q] != te[rev ? e + k - 1 - q : e + q];
    return __ballot(ne) == 0ull;
}
// HashSet.contains / indexOf: the entry of the n k-mers a walk added that equals chain k-mer c of text tc (forward hash f), else WAVE_NOWHERE — entry e is
// chain k-mer e + 1 of text te with forward hash hrow[e] (a walk's entries differ).  rev: the two texts walk in opposite directions.
__device__ int sc_find(int k, const uint64_t *hrow, const uint8_t *te, int n, const uint8_t *tc, int c, uint64_t f, bool rev, uint32_t lane) {
    return wave_find(0, n, k, [&](int e) { return hrow[e]; }, f, [&](int e, int q) { return te[e + 1 + (rev ? k - 1 - q : q)]; },
                     [&](int q) { return tc[c + q]; }, false, lane);
}

// getMaxCoveragePath(graph, left, right, bound, lookahead, bf) (:1677-1776) for left = k-mer li and right = k-mer ri of the sequence.  form 0:
// null; 1: the left walk arrived, the path is its n0 k-mers (chain k-mers 1 .. n0 of text 0); 2: the right walk arrived, the path is its n1
// k-mers (chain k-mers n1 .. 1 of text 1, which runs right to left); 3: the right walk met entry idx of the left walk (:1748-1763), the path
// is the left walk's entries 0 .. idx (the last of them is the k-mer met) and then the right walk's n1 k-mers.
struct ScPath {
    int form, n0, n1, idx;
    __device__ __forceinline__ int size() const { return form == 1 ? n0 : form == 2 ? n1 : form == 3 ? idx + 1 + n1 : -1; }
};
__device__ ScPath sc_max_cov_path(const ScArgs &a, const ScSeq &sq, const ScRows &rw, ScLevel *dfs, int li, int ri, int bound, uint32_t lane) {
    const int k = a.k;
    const Dir dr0 = wave_dir<true>(a.stranded, a.k, 0), dr1 = wave_dir<true>(a.stranded, a.k, 1);
    uint64_t A, B;
    int n0 = 0, n1 = 0;                                          // leftPath.size(), rightPath.size() less the spliced-in k-mers
    sc_walk_begin(a, sq, dr0, li, rw.tx[0], A, B, lane);
    for (int depth = 0; depth < bound; ++depth) {
        const ScPick p = sc_greedy_step(a, dr0, rw.tx[0], n0, A, B, dfs, lane);
        if (!p.any) break;
        const uint64_t f = dr0.fwd(p.A, p.B);
        if (lane == 0) { rw.tx[0][k + n0] = (uint8_t)p.base; rw.h[0][n0] = f; }      // entry n0, kept only if the k-mer is added
        wave_fence();
        if (sc_equals_seq(a, sq, dr0, rw.tx[0], n0 + 1, f, ri, lane)) return ScPath{1, n0, 0, 0};
        if (sc_find(k, rw.h[0], rw.tx[0], n0, rw.tx[0], n0 + 1, f, false, lane) != WAVE_NOWHERE) break;
        A = p.A; B = p.B; ++n0;
    }
    /* not connected, search from right */
    sc_walk_begin(a, sq, dr1, ri, rw.tx[1], A, B, lane);
    for (int depth = 0; depth < bound; ++depth) {
        const ScPick p = sc_greedy_step(a, dr1, rw.tx[1], n1, A, B, dfs, lane);
        if (!p.any) break;
        const uint64_t f = dr1.fwd(p.A, p.B);
        if (lane == 0) { rw.tx[1][k + n1] = (uint8_t)p.base; rw.h[1][n1] = f; }
        wave_fence();
        if (sc_equals_seq(a, sq, dr1, rw.tx[1], n1 + 1, f, li, lane)) return ScPath{2, n0, n1, 0};
        const int idx = sc_find(k, rw.h[0], rw.tx[0], n0, rw.tx[1], n1 + 1, f, true, lane);
        if (idx != WAVE_NOWHERE) return ScPath{3, n0, n1, idx};     // right path intersects the left path (:1748-1763)
        if (sc_find(k, rw.h[1], rw.tx[1], n1, rw.tx[1], n1 + 1, f, false, lane) != WAVE_NOWHERE) break;          // :1769-1771
        A = p.A; B = p.B; ++n1;
    }
    return ScPath{0, n0, n1, 0};
}

// greedyExtendRight / Left(graph, source, lookahead, bound, bf) from k-mer s of the sequence into rows `side`: the number of k-mers added
__device__ int sc_greedy_walk(const ScArgs &a, const ScSeq &sq, const ScRows &rw, ScLevel *dfs, int side, int s, int bound, uint32_t lane) {
    const Dir dr = wave_dir<true>(a.stranded, a.k, side);
    uint64_t A, B;
    int n = 0;
    sc_walk_begin(a, sq, dr, s, rw.tx[side], A, B, lane);
    while (n < bound) {
        const ScPick p = sc_greedy_step(a, dr, rw.tx[side], n, A, B, dfs, lane);
        if (!p.any) break;
        if (lane == 0) { rw.tx[side][a.k + n] = (uint8_t)p.base; rw.h[side][n] = dr.fwd(p.A, p.B); }
        wave_fence();
        A = p.A; B = p.B; ++n;
    }
    return n;
}
// kmers1.retainAll(...) leaves something (:7748-7750): a k-mer of the right-hand walk (n0 entries of rows 0) equals one of the left-hand walk
// (n1 entries of rows 1).  Every lane keeps up to 16 of the first walk's forward hashes; the second walk's go by one at a time.
__device__ bool sc_walks_meet(const ScArgs &a, const ScRows &rw, int n0, int n1, uint32_t lane) {
    static_assert(SC_GREEDY_BOUND <= 16 * 64, "a lane keeps 16 hashes of the first walk");
    uint64_t mine[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) { const int e = 64 * j + (int)lane; mine[j] = e < n0 ? rw.h[0][e] : 0ull; }
    for (int e1 = 0; e1 < n1; ++e1) {
        const uint64_t f = rw.h[1][e1];
        uint32_t hit = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) hit |= (uint32_t)(mine[j] == f && 64 * j + (int)lane < n0) << j;
        if (!__ballot(hit != 0u)) continue;
        for (int j = 0; j < 16; ++j) {
            unsigned long long m = __ballot((hit >> j) & 1u);
            while (m) {
                const int e0 = 64 * j + (int)__builtin_ctzll(m);
                m &= m - 1ull;
                if (sc_equals_chain(a.k, rw.tx[1], e1 + 1, rw.tx[0], e0 + 1, true, lane)) return true;
            }
        }
    }
    return false;
}

// the first index in [from, to) whose gate bit is `want`, else `to`; the last one in [lo, hi), else lo - 1
__device__ int sc_next(const ScSeq &sq, int from, int to, bool want, uint32_t lane) {
    return wave_first(from, to, [&](int p) { return (sq.gbit[p] != 0) == want; }, lane);
}
__device__ int sc_prev(const ScSeq &sq, int lo, int hi, bool want, uint32_t lane) {
    return wave_last(lo, hi, [&](int p) { return (sq.gbit[p] != 0) == want; }, lane);
}

// isChimera (:7674-7760) into the record's chimera fields; true: chimera
__device__ bool sc_chimera(const ScArgs &a, const ScSeq &sq, const ScRows &rw, ScLevel *dfs, rb_screen_rec &rec, uint32_t lane) {
    const int nk = sq.nk, max_gap = 2 * a.k;
    if (!(sq.gbit[0] && sq.gbit[nk - 1])) { rec.chim_why = RB_CHIM_WHY_ENDS; return false; }
    int i = 1;
    while (i < nk - 1) {
        i = sc_next(sq, i, nk - 1, false, lane);
        if (i >= nk - 1) break;
        const int t = sc_next(sq, i + 1, nk - 1, true, lane);   // check to see if this is a small gap
        if (t < nk - 1 && t - i <= max_gap && sc_max_cov_path(a, sq, rw, dfs, i - 1, t, t - i, lane).form) { i = t + 1; continue; }
        break;
    }
    if (i == nk - 1) { rec.chim_why = RB_CHIM_WHY_ASSEMBLED; return false; }
    --i;
    int j = nk - 2;
    while (j > i) {
        j = sc_prev(sq, i + 1, j + 1, false, lane);              // (i where every k-mer down to i + 1 is in the gate: the loop's own end)
        if (j <= i) break;
        const int t = sc_prev(sq, i + 1, j, true, lane);
        if (t > i && j - t <= max_gap && sc_max_cov_path(a, sq, rw, dfs, t, j + 1, j - t, lane).form) { j = t - 1; continue; }
        break;
    }
    ++j;
    rec.break_i = i; rec.break_j = j;
    if (j - i > max_gap) { rec.chim_why = RB_CHIM_WHY_WIDE_GAP; return false; }
    const int n0 = sc_greedy_walk(a, sq, rw, dfs, 0, i, SC_GREEDY_BOUND, lane), n1 = sc_greedy_walk(a, sq, rw, dfs, 1, j, SC_GREEDY_BOUND, lane);
    rec.right_len = n0; rec.left_len = n1;
    const bool meet = sc_walks_meet(a, rw, n0, n1, lane);
    rec.chim_why = meet ? RB_CHIM_WHY_PATHS_MEET : RB_CHIM_WHY_DISJOINT;
    return !meet;
}

// The static GraphUtils.hasDepthRight / hasDepthLeft(source, graph, depth[, bf]) (:6680-6778) from k-mer s of the sequence: 1 true, 0 false,
// -1 where the search would make more than max_visits getSuccessors / getPredecessors calls.  The reference's frontier is a stack of neighbour
// deques; level l here is the k-mer whose neighbours that deque holds (chain k-mer l of the text, hashes in the two hash rows) and the mask
// of those not yet popped.  `frontier.size() >= depth` is tested after every push and after every removal of an empty level, never before
// the first of them.  A level is pushed only while size < depth <= cap, so the rows hold the stack.
__device__ int sc_has_depth(const ScArgs &a, const ScSeq &sq, const ScRows &rw, int left, bool gated, int s, int depth, uint32_t lane) {
    const Dir dr = wave_dir<true>(a.stranded, a.k, left);
    uint8_t *tx = rw.tx[0];
    uint64_t tA, tB;
    sc_walk_begin(a, sq, dr, s, tx, tA, tB, lane);
    ScNb nb;
    int visits = 1, size = 1;
    uint32_t tm = sc_neighbors(a, dr, gated, tA, tB, tx[0], lane, nb);
    if (lane == 0) { rw.h[0][0] = tA; rw.h[1][0] = tB; rw.mk[0] = (uint8_t)tm; }
    wave_fence();
    while (size > 0) {
        if (!tm) {                                               // alts.isEmpty(): frontier.removeLast()
            --size;
            if (size > 0) { tA = rw.h[0][size - 1]; tB = rw.h[1][size - 1]; tm = rw.mk[size - 1]; }
        } else {                                                 // frontier.add(alts.pop().getSuccessors(...))
            const uint32_t b = (uint32_t)__builtin_ctz(tm);
            tm &= tm - 1u;
            uint64_t cA, cB;
            dr.step(tA, tB, tx[size - 1], b, cA, cB);
            if (visits >= a.max_visits) return -1;
            if (lane == 0) { rw.mk[size - 1] = (uint8_t)tm; tx[a.k + size - 1] = (uint8_t)b; }
            wave_fence();
            ++visits;
            tm = sc_neighbors(a, dr, gated, cA, cB, tx[size], lane, nb);
            tA = cA; tB = cB;
            if (size < a.cap && lane == 0) { rw.h[0][size] = tA; rw.h[1][size] = tB; rw.mk[size] = (uint8_t)tm; }
            wave_fence();
            ++size;
        }
        if (size >= depth) return 1;
    }
    return 0;
}

// getMinimumKmerCoverage(kmers, start, end) (:133-145) as a count code; getMedianKmerCoverage(kmers, start, end) (:208-217)
__device__ uint32_t sc_min_code(const ScSeq &sq, int start, int end, uint32_t lane) {
    return min_code([&](int p) { return sq.code(p); }, start, end, lane);
}
__device__ float sc_median(const ScSeq &sq, int start, int end, uint32_t lane) {
    return median_code([&](int p) { return sq.code(start + p); }, end - start, lane);
}

// isBluntEndArtifact (:8535-8586) into the record's blunt-end fields: 1 artifact, 0 not, -1 a depth search ran out of its budget
__device__ int sc_blunt_end(const ScArgs &a, const ScSeq &sq, const ScRows &rw, rb_screen_rec &rec, uint32_t lane) {
    if (a.max_depth <= 0) return 0;
    const int nk = sq.nk, d = a.read_d;
    const uint32_t left_edge = sc_min_code(sq, 0, min(a.max_depth, nk), lane), right_edge = sc_min_code(sq, max(0, nk - a.max_depth), nk, lane);
    const bool g0 = sq.gbit[0] != 0, gl = sq.gbit[nk - 1] != 0;
    int v;
    if (g0 && (!gl || left_edge > right_edge)) {
        const int i = sc_next(sq, 1, nk, false, lane);
        rec.boundary = i;
        if (i == nk || i < nk - d) { rec.blunt_why = RB_BLUNT_WHY_LEFT_RANGE; return 0; }
        rec.blunt_why = RB_BLUNT_WHY_LEFT_FAILED;
        if ((v = sc_has_depth(a, sq, rw, 0, false, nk - 1, a.max_depth, lane)) != 0) return v < 0 ? -1 : 0;
        if (!(sc_median(sq, 0, i, lane) > sc_median(sq, i, nk, lane))) return 0;
        if ((v = sc_has_depth(a, sq, rw, 0, true, i - 1, nk - i, lane)) != 1) return v;
        rec.blunt_why = RB_BLUNT_WHY_LEFT_ARTIFACT;
        return 1;
    }
    if (gl && (!g0 || left_edge < right_edge)) {
        const int j = sc_prev(sq, 0, nk - 1, false, lane);
        rec.boundary = j + 1;
        if (j == -1 || j > d) { rec.blunt_why = RB_BLUNT_WHY_RIGHT_RANGE; return 0; }
        rec.blunt_why = RB_BLUNT_WHY_RIGHT_FAILED;
        if ((v = sc_has_depth(a, sq, rw, 1, false, 0, a.max_depth, lane)) != 0) return v < 0 ? -1 : 0;
        if (!(sc_median(sq, j + 1, nk, lane) > sc_median(sq, 0, j + 1, lane))) return 0;
        if ((v = sc_has_depth(a, sq, rw, 1, true, j + 1, j + 1, lane)) != 1) return v;
        rec.blunt_why = RB_BLUNT_WHY_RIGHT_ARTIFACT;
        return 1;
    }
    return 0;
}

// Kmer.getRightVariants / getLeftVariants(k, numHash, graph) (R/graph/Kmer.java:357-405, CanonicalKmer.java:382-436) of k-mer i: does any of
// the three other last bases, or of the three other first bases, give a k-mer with graph.getCount >= 1?  (isBranchFree asks the member
// hasDepthRight / Left of each, which is always true.)  One lane, six counts; the hashes are rb_graph_neighbors' (direction 3 / 2).
__device__ bool sc_has_variant(const ScArgs &a, const ScSeq &sq, int i) {
    const uint32_t uk = (uint32_t)a.k, c0 = sq.base(i), c1 = sq.base(i + a.k - 1);
    const uint64_t f = sq.F[i], r = a.stranded ? 0ull : sq.R[i];
    bool any = false;
    for (uint32_t b = 0; b < 4u; ++b) {
        if (b != c1) {
            const uint64_t nf = f ^ seed_of(c1) ^ seed_of(b), nr = r ^ rotl_var(seed_of(3u - c1) ^ seed_of(3u - b), uk - 1u);
            any = any || count_code(a.fv, a.stranded ? nf : smin(nf, nr)) != 0u;
        }
        if (b != c0) {
            const uint64_t nf = f ^ rotl_var(seed_of(c0) ^ seed_of(b), uk - 1u), nr = r ^ seed_of(3u - c0) ^ seed_of(3u - b);
            any = any || count_code(a.fv, a.stranded ? nf : smin(nf, nr)) != 0u;
        }
    }
    return any;
}

// the screens of sequence r of the piece, by one wavefront
__device__ void sc_one(const ScArgs &a, int64_t r, const ScRows &rw, ScLevel *dfs, uint32_t lane) {
    const int64_t k0 = a.kof[r];
    const int nk = (int)(a.kof[r + 1] - k0);
    rb_screen_rec rec;
    rec.flags = 0; rec.chim_why = 0; rec.break_i = -1; rec.break_j = -1; rec.right_len = 0; rec.left_len = 0; rec.blunt_why = 0; rec.boundary = -1;
    if (nk == 0) {
        rec.flags = RB_SCREEN_NO_KMER;
        if (lane == 0) a.recs[r] = rec;
        return;
    }
    if (wave_bad_letter(a.valid + a.woff[r], nk + a.k - 1, lane)) {    // not judged
        rec.flags = RB_SCREEN_BAD_LETTER;
        if (lane == 0) a.recs[r] = rec;
        return;
    }
    const ScSeq sq{reinterpret_cast<const uint32_t *>(a.codes + a.woff[r]), a.F + k0, a.R + k0, a.cnt + k0, a.gbit + k0, nk, a.stranded};
    // the k-mers side by side: the gate bit of each, and whether it has a variant
    const bool gated = (a.what & (RB_SCREEN_CHIMERA | RB_SCREEN_BLUNT_END)) != 0;
    bool branch = false;
    for (int i = (int)lane; i < nk; i += 64) {
        if (gated) {
            const uint64_t f = sq.F[i];
            a.gbit[k0 + i] = (uint8_t)bits_lookup(a.gate.bits, a.gate.mod, a.gate.num_hash, a.kmul, a.stranded ? f : smin(f, sq.R[i]));
        }
        if (a.what & RB_SCREEN_BRANCH_FREE) branch = branch || sc_has_variant(a, sq, i);
    }
    wave_fence();
    if ((a.what & RB_SCREEN_BRANCH_FREE) && !__ballot(branch)) rec.flags |= RB_SCREEN_BRANCH_FREE;
    if ((a.what & RB_SCREEN_CHIMERA) && sc_chimera(a, sq, rw, dfs, rec, lane)) rec.flags |= RB_SCREEN_CHIMERA;
    if (a.what & RB_SCREEN_BLUNT_END) {
        const int v = sc_blunt_end(a, sq, rw, rec, lane);
        if (v > 0) rec.flags |= RB_SCREEN_BLUNT_END;
        if (v < 0) { rec.flags |= RB_SCREEN_OVER_BUDGET; rec.blunt_why = 0; }
    }
    if (lane == 0) a.recs[r] = rec;
}

// A wavefront per sequence, taking sequences in turn; its walk rows are its slot of `scratch`, its lookahead stacks in LDS
__global__ void __launch_bounds__(SC_TPB) k_screen(ScArgs a, uint8_t *scratch, size_t row_bytes) {
    __shared__ ScLevel s_dfs[SC_WAVES][4 * SC_LEVELS];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t slot = (int64_t)blockIdx.x * SC_WAVES + wv, n_slots = (int64_t)gridDim.x * SC_WAVES;
    const ScRows rw(scratch + (size_t)slot * row_bytes, a.cap, a.k);
    for (int64_t r = slot; r < a.pn; r += n_slots) {
        sc_one(a, r, rw, s_dfs[wv], lane);
        wave_fence();
    }
}

// ---- represented (:711-824) ----
__host__ __device__ inline rb_repr_rec repr_blank(int flags) { return rb_repr_rec{flags, -1, -1, -1, -1, -1, -1, 0, 0, 0, 0, 0}; }

// getPercentIdentity(s, t) >= percentIdentity for s = the slen letters s(0 ..) of an assembled walk or path and t = the sequence's tlen >= 1
// letters from t0 on; d: getDistance(s, t).  An empty path assembles to "": d = tLen (:196).  The row is in LDS up to LEV_LDS columns.
template <class S>
__device__ bool sc_identity_ok(const ScArgs &a, const ScSeq &sq, S s, int slen, int t0, int tlen, int *lds_row, int *dev_row, int &d, uint32_t lane) {
    if (slen == 0) d = tlen;
    else d = ce_distance(s, slen, [&](int x) -> uint32_t { return sq.base(t0 + x); }, tlen, tlen > LEV_LDS ? dev_row : lds_row, lane);
    wave_fence();
    return !(ce_identity(d, slen, tlen) < a.percent_identity);
}

// represented of sequence r of the piece, by one wavefront: the record's flags.  FILLED: the sequence's gate bits stand in a.gbit already
// (k_represented_walk fills them with its whole workgroup), else the wavefront fills them first.
template <bool FILLED = false>
__device__ int sc_repr_one(const ScArgs &a, int64_t r, const ScRows &rw, ScLevel *dfs, int *lds_row, int *dev_row, uint32_t lane) {
    const int64_t k0 = a.kof[r];
    const int nk = (int)(a.kof[r + 1] - k0), k = a.k, clip = a.max_depth, max_indel = a.max_indel;
    if (nk == 0 || wave_bad_letter(a.valid + a.woff[r], nk + a.k - 1, lane)) {
        const int flags = nk == 0 ? RB_SCREEN_NO_KMER : RB_SCREEN_BAD_LETTER;
        if (lane == 0) a.reprs[r] = repr_blank(flags);
        return flags;
    }
    const ScSeq sq{reinterpret_cast<const uint32_t *>(a.codes + a.woff[r]), a.F + k0, a.R + k0, a.cnt + k0, a.gbit + k0, nk, a.stranded};
    if constexpr (!FILLED) {
        for (int i = (int)lane; i < nk; i += 64) {
            const uint64_t f = sq.F[i];
            a.gbit[k0 + i] = (uint8_t)bits_lookup(a.gate.bits, a.gate.mod, a.gate.num_hash, a.kmul, a.stranded ? f : smin(f, sq.R[i]));
        }
        wave_fence();
    }
    rb_repr_rec rec = repr_blank(0);
    rec.why = RB_REPR_WHY_TRUE;
    auto decide = [&](int why, int left, int right, int expected, int found, int d) {
        rec.why = why; rec.left = left; rec.right = right; rec.expected_len = expected; rec.found_len = found; rec.distance = d;
    };
    int last = -1, i = 0;                                        // lastRepresentedKmerFoundIndex
    bool open = true;                                            // no line has returned yet
    while (open) {
        const int start = sc_next(sq, i, nk, true, lane);
        if (start >= nk) break;
        const int end = sc_next(sq, start + 1, nk, false, lane) - 1;
        i = end + 1;
        if (end - start + 1 < a.lookahead) continue;
        if (start > 0 && last < 0) {                             // check left edge kmers (:745-753)
            int v = 1, d = -1;
            if (start < clip) v = sc_has_depth(a, sq, rw, 1, false, 0, clip - start, lane);
            if (v < 0) { if (lane == 0) a.reprs[r] = repr_blank(RB_SCREEN_OVER_BUDGET); return RB_SCREEN_OVER_BUDGET; }
            if (v == 0) ++rec.tips_skipped;
            else {
                const int n = sc_greedy_walk(a, sq, rw, dfs, 1, start, start, lane);
                const uint8_t *tx = rw.tx[1];                    // the walk's letters run right to left
                if (n != start) { decide(RB_REPR_WHY_LEFT_LENGTH, 0, start, start, n, -1); open = false; }
                else if (!sc_identity_ok(a, sq, [&](int x) -> uint32_t { return tx[n + k - 1 - x]; }, n + k - 1, 0, start + k - 1, lds_row, dev_row, d, lane)) {
                    decide(RB_REPR_WHY_LEFT_IDENTITY, 0, start, start, n, d); open = false;
                } else { ++rec.tests_passed; rec.distance_sum += d; }
            }
        } else if (start > 0) {                                  // check gap kmers (:756-796)
            int expected = start - last - 1, left = last, right = start, d = -1;
            if (expected > a.read_d + k) { rec.why = RB_REPR_WHY_WIDE_GAP; open = false; continue; }
            const int missing = k - expected;
            if (missing > 0) {                                   // --left / ++right come before the lookup: a widening stops ON a k-mer outside the gate
                const int lo = max(0, left - missing), hi = min(nk - 1, right + missing);
                const int pl = sc_prev(sq, lo, left, false, lane), pr = sc_next(sq, right + 1, hi + 1, false, lane);
                left = pl >= lo ? pl : lo; right = pr <= hi ? pr : hi;
                expected = right - left - 1;
            }
            const ScPath p = sc_max_cov_path(a, sq, rw, dfs, left, right, expected + max_indel, lane);
            const int plen = p.size();
            rec.path_form = p.form;
            if (!p.form) { decide(RB_REPR_WHY_NO_PATH, left, right, expected, -1, -1); open = false; continue; }
            if (plen < expected - max_indel || plen > expected + max_indel) { decide(RB_REPR_WHY_PATH_LENGTH, left, right, expected, plen, -1); open = false; continue; }
            const uint8_t *t0 = rw.tx[0], *t1 = rw.tx[1];
            const int slen = plen ? plen + k - 1 : 0, tlen = expected + k - 1, n1 = p.n1, cut = p.idx + k;
            bool ok;
            if (p.form == 1) ok = sc_identity_ok(a, sq, [&](int x) -> uint32_t { return t0[1 + x]; }, slen, left + 1, tlen, lds_row, dev_row, d, lane);
            else if (p.form == 2) ok = sc_identity_ok(a, sq, [&](int x) -> uint32_t { return t1[n1 + k - 1 - x]; }, slen, left + 1, tlen, lds_row, dev_row, d, lane);
            else ok = sc_identity_ok(a, sq, [&](int x) -> uint32_t { return x < cut ? t0[1 + x] : t1[n1 - (x - cut)]; }, slen, left + 1, tlen, lds_row, dev_row, d, lane);
            if (!ok) { decide(RB_REPR_WHY_PATH_IDENTITY, left, right, expected, plen, d); open = false; continue; }
            ++rec.tests_passed; rec.distance_sum += d;
        }
        if (open) last = end;
    }
    if (open && last < 0) { rec.why = RB_REPR_WHY_NO_RUN; open = false; }
    if (open && last < nk - 1) {                                 // check right edge kmers (:807-817)
        const int expected = nk - last - 1;
        int v = 1, d = -1;
        if (expected < clip) v = sc_has_depth(a, sq, rw, 0, false, nk - 1, clip - expected, lane);
        if (v < 0) { if (lane == 0) a.reprs[r] = repr_blank(RB_SCREEN_OVER_BUDGET); return RB_SCREEN_OVER_BUDGET; }
        if (v == 0) ++rec.tips_skipped;
        else {
            const int n = sc_greedy_walk(a, sq, rw, dfs, 0, last, expected, lane);
            const uint8_t *tx = rw.tx[0];
            if (n != expected) { decide(RB_REPR_WHY_RIGHT_LENGTH, last, nk - 1, expected, n, -1); open = false; }
            else if (!sc_identity_ok(a, sq, [&](int x) -> uint32_t { return tx[1 + x]; }, n + k - 1, last + 1, expected + k - 1, lds_row, dev_row, d, lane)) {
                decide(RB_REPR_WHY_RIGHT_IDENTITY, last, nk - 1, expected, n, d); open = false;
            } else { ++rec.tests_passed; rec.distance_sum += d; }
        }
    }
    if (open) rec.flags = RB_REPR_REPRESENTED;
    if (lane == 0) a.reprs[r] = rec;
    return rec.flags;
}

// as k_screen; the alignment's row is the wavefront's LDS row, or — longer than LEV_LDS columns — the ints at lev_off of its scratch slot
__global__ void __launch_bounds__(SC_TPB) k_represented(ScArgs a, uint8_t *scratch, size_t row_bytes, size_t lev_off) {
    __shared__ ScLevel s_dfs[SC_WAVES][4 * SC_LEVELS];
    __shared__ int s_row[SC_WAVES][LEV_LDS];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t slot = (int64_t)blockIdx.x * SC_WAVES + wv, n_slots = (int64_t)gridDim.x * SC_WAVES;
    uint8_t *mine = scratch + (size_t)slot * row_bytes;
    const ScRows rw(mine, a.cap, a.k);
    for (int64_t r = slot; r < a.pn; r += n_slots) {
        sc_repr_one(a, r, rw, s_dfs[wv], s_row[wv], reinterpret_cast<int *>(mine + lev_off), lane);
        wave_fence();
    }
}

// ---- represented, then add: TranscriptWriter.write (R/RNABloom.java:1639-1720), GraphUtils.reduceRedundancy (R/util/GraphUtils.java:652-699) ----
// The loop is sequential ACROSS sequences — a sequence is judged against the gate as every earlier kept sequence left it — and wide INSIDE
// one: nk gate look-ups before the verdict, nk x num_hash bit sets behind a verdict of "not represented".  So ONE workgroup walks the piece's
// sequences one after the other in ONE launch (DESIGN.md §5 "Represented, then add"):
//   the fill     a lane per k-mer, all wavefronts: a.gbit[i] = gate.lookup(getHash(k-mer i)); sc_repr_one<true> takes the bits as filled;
//   the verdict  wavefront 0 alone: the represented body as k_represented runs it, walk rows in the one scratch slot, DFS and alignment rows
//                in LDS; kept (flags == 0): getMedianKmerCoverage of the counts; keep, median and the record by lane 0;
//   the add      a lane per (k-mer, hash function), all wavefronts: an atomic OR of agent scope each (BloomFilter.add, R/bloom/BloomFilter.java:133-137).
// The walker reads gate bits it set a moment earlier, by plain loads (the body's, unchanged).  Visibility, the fence form: the ORs are done in
// L2; behind them EVERY wavefront executes __threadfence() — its acquire half drops the lines of the gate that this CU's vector L1 holds from
// before the ORs — and the workgroup meets at __syncthreads() before the next sequence's first gate load.  The gate reaches the kernel as a
// plain pointer: no __restrict__, no promise of invariance, so no gate load is hoisted over the fence or sent down the scalar path.  The
// other form (every gate load a relaxed atomic of agent scope, as rb_subsample.hip reads its counters) would put a load policy into every walk
// and search of the body for the sake of this one kernel; the fence costs a few microseconds per KEPT sequence and nothing per represented one.
// One workgroup waits on nobody: no flags, no spins.  The walk stops at the first sequence that is over its budget; *stop is its index in
// the piece, or pn.
constexpr int RW_TPB = 256;               // the fill and the add are short (a transcript's k-mers); the verdict is one wavefront's whatever the width

__global__ void __launch_bounds__(RW_TPB) k_represented_walk(ScArgs a, uint32_t *gate_bits, uint8_t *scratch, size_t lev_off, uint8_t *keep, float *median,
                                                             int64_t *stop) {
    __shared__ ScLevel s_dfs[4 * SC_LEVELS];
    __shared__ int s_row[LEV_LDS];
    __shared__ int s_flags;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const ScRows rw(scratch, a.cap, a.k);
    const uint32_t H = (uint32_t)a.gate.num_hash;
    int64_t r = 0;
    for (; r < a.pn; ++r) {
        const int64_t k0 = a.kof[r];
        const int nk = (int)(a.kof[r + 1] - k0);
        const uint64_t *F = a.F + k0, *R = a.R + k0;
        // ---- the fill ----
        for (int i = (int)tid; i < nk; i += RW_TPB) {
            const uint64_t f = F[i];
            a.gbit[k0 + i] = (uint8_t)bits_lookup(a.gate.bits, a.gate.mod, a.gate.num_hash, a.kmul, a.stranded ? f : smin(f, R[i]));
        }
        __syncthreads();
        // ---- the verdict ----
        if (tid < 64u) {
            const int flags = sc_repr_one<true>(a, r, rw, s_dfs, s_row, reinterpret_cast<int *>(scratch + lev_off), lane);
            float med = 0.0f;
            if (flags == 0) {
                const ScSeq sq{nullptr, F, R, a.cnt + k0, a.gbit + k0, nk, a.stranded};
                med = sc_median(sq, 0, nk, lane);
            }
            if (lane == 0u) { keep[r] = flags == 0 ? 1 : 0; median[r] = med; s_flags = flags; }
        }
        __syncthreads();
        const int flags = s_flags;
        if (flags & RB_SCREEN_OVER_BUDGET) break;                // the stop rule: every later answer would hang on this one
        // ---- the add ----
        if (flags == 0) {
            const uint32_t total = (uint32_t)nk * H;             // nk <= 2^24 (SC_MAX_ROW), H <= RB_MAX_HASH
            for (uint32_t e = tid; e < total; e += RW_TPB) {
                const uint32_t i = e / H, j = e - i * H;
                const uint64_t f = F[i];
                const uint64_t b = index_of(multi_hash(a.stranded ? f : smin(f, R[i]), j, a.kmul), a.gate.mod);
                __hip_atomic_fetch_or(gate_bits + (b >> 5), 1u << (uint32_t)(b & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __threadfence();
        }
        __syncthreads();
    }
    if (tid == 0u) *stop = r;
}

// What the two calls share once their arguments are checked: the pieces (rb_pieces.hpp), each with its getKmers rows, gate bits, records and the
// wavefronts' rows.  REC is the record, `blank` what a sequence no kernel touches gets, `cap` the entries of a walk row, lev_cols the ints of
// a wavefront's alignment row in device scratch (0: none), `launch` the kernel.
template <class REC, class LAUNCH>
void screen_run(rb_graph *g, const rb_graph *gate, const char *seq, const int64_t *offsets, int64_t n, const char *who, const char *entry, ScArgs a,
                const std::vector<int64_t> &ko, const REC &blank, size_t lev_cols, REC *out, LAUNCH launch) {
    for (int64_t i = 0; i < n; ++i) out[i] = blank;
    if (ko[(size_t)n] == 0) return;
    // the gate is read too: shared lock on it for the call, in address order with g's (rb_graph_greedy_extend)
    rb_graph *gm = const_cast<rb_graph *>(gate);
    std::shared_lock<std::shared_mutex> gate_lk;
    if (gm && gm != g && gm < g) gate_lk = std::shared_lock<std::shared_mutex>(gm->rw);
    RB_HIP(hipSetDevice(g->p.device));
    HostPin pin_r(out, (size_t)n * sizeof(REC));
    QueryLease q(g);
    if (gm && gm != g && gm > g) gate_lk = std::shared_lock<std::shared_mutex>(gm->rw);
    RB_REQUIRE(g->dbg.bits && g->cbf, "%s: dbgbf or the counting filter has been destroyed", who);
    if (gate) RB_REQUIRE(gate->dbg.bits, "%s: the gate's filter has been destroyed", who);
    hipStream_t s = q.c->st;
    const int k = g->k;
    const size_t lev_off = sc_row_bytes(a.cap, k), row_bytes = lev_off + up16(lev_cols * sizeof(int));
    const int64_t max_slots = std::max<int64_t>(16, std::min<int64_t>(SC_MAX_SLOTS, (int64_t)(SC_ROW_BUDGET / row_bytes)));
    // piece by piece (rb_pieces.hpp): b0 the piece's k-mer offsets, b1 / b2 the getKmers hashes, b3 counts, gate bits, records and the
    // wavefronts' rows; with profiling on the kernels of every piece are timed: entry `entry`
    for_each_host_piece(g, s, seq, offsets, ko.data(), n, entry, [&](HostPiece &pc) {
        const int64_t ra = pc.ra, pn = pc.pn, pt = pc.pt;
        const int64_t slots = std::min<int64_t>(pn, max_slots);
        const unsigned blocks = blocks_for(slots, SC_WAVES);
        const size_t o_g = up16((size_t)pt * 4), o_rec = up16(o_g + (size_t)pt), o_row = up16(o_rec + (size_t)pn * sizeof(REC));
        q.c->b3.reserve(o_row + (size_t)blocks * SC_WAVES * row_bytes + 16);
        uint8_t *base3 = q.c->b3.as<uint8_t>();
        a.fv = g->view(0, 0);
        a.gate = ScGate{gate ? gate->dbg.bits : nullptr, gate ? gate->dbg.mod : g->dbg.mod, gate ? gate->dbg.num_hash : 0};
        a.kmul = kmul_of(k);
        a.stranded = (int)g->stranded; a.k = k; a.read_d = g->read_d;
        a.gbit = base3 + o_g;
        REC *recs = reinterpret_cast<REC *>(base3 + o_rec);
        RB_HIP(hipMemsetAsync(base3 + o_g, 0, o_rec - o_g, s));
        PieceRows(g, *q.c, pc).into(a);
        launch(a, recs, blocks, s, base3 + o_row, row_bytes, lev_off);
        RB_HIP(hipGetLastError());
        pc.kernels_end();
        RB_HIP(hipMemcpyAsync(out + ra, recs, (size_t)pn * sizeof(REC), hipMemcpyDeviceToHost, s));
    });
}

void screen_call(rb_graph *g, const rb_graph *gate, const char *seq, const int64_t *offsets, int64_t n, int what, int lookahead, int max_depth,
                 int64_t max_visits, rb_screen_rec *out) {
    const char *who = "rb_graph_screen_fragments";
    RB_REQUIRE(g, "%s: null handle", who);
    RB_REQUIRE(!g->shard, "%s: not available on a shard handle", who);
    RB_REQUIRE(g->dbg.bits && g->cbf, "%s: dbgbf or the counting filter has been destroyed", who);
    RB_REQUIRE(what > 0 && what <= 7, "%s: what = %d is not a mask of the three screens", who, what);
    const bool gated = (what & (RB_SCREEN_CHIMERA | RB_SCREEN_BLUNT_END)) != 0;
    RB_REQUIRE(!gated || gate, "%s: the chimera and the blunt-end screen need a gate", who);
    if (gate)
        RB_REQUIRE(gate->dbg.bits && !gate->shard && gate->p.device == g->p.device && gate->k == g->k,
                   "%s: the gate must be a filter on the same device with the same k", who);
    RB_REQUIRE(lookahead >= 0 && lookahead <= SC_MAX_LOOKAHEAD, "%s: lookahead out of range [0, %d]", who, SC_MAX_LOOKAHEAD);
    RB_REQUIRE(max_depth <= SC_MAX_DEPTH, "%s: max_depth above %d", who, SC_MAX_DEPTH);
    RB_REQUIRE(max_visits >= 0, "%s: max_visits = %lld", who, (long long)max_visits);
    RB_REQUIRE(n >= 0, "%s: n = %lld", who, (long long)n);
    if (n == 0) return;
    RB_REQUIRE(offsets && out, "%s: null argument", who);
    std::vector<int64_t> ko((size_t)n + 1);
    kmer_offsets(offsets, n, g->k, ko.data(), who);
    RB_REQUIRE(offsets[n] == offsets[0] || seq, "%s: null sequence text", who);
    const int64_t visits = max_visits ? max_visits : RB_SCREEN_DEFAULT_VISITS;
    ScArgs a{};
    a.what = what; a.lookahead = lookahead; a.max_depth = max_depth; a.max_indel = 0; a.percent_identity = 0.0f;
    a.max_visits = (int)std::min<int64_t>(visits, INT32_MAX);
    // a walk row: the greedy walks' 1000 k-mers, a gap's 2k <= 512, and a depth search's stack — as deep as the depth asked for (max_depth, or a
    // stretch of the sequence) and never deeper than its budget, since every level costs a visit
    a.cap = (int)std::max<int64_t>(SC_GREEDY_BOUND, std::min<int64_t>(std::max<int64_t>(max_depth, longest_list(ko, n)), visits));
    a.reprs = nullptr;
    // what no kernel touches: the sequences of pieces without a k-mer
    const rb_screen_rec blank{RB_SCREEN_NO_KMER, 0, -1, -1, 0, 0, 0, -1};
    screen_run(g, gate, seq, offsets, n, who, "screen_fragments", a, ko, blank, 0, out,
               [](ScArgs &a, rb_screen_rec *recs, unsigned blocks, hipStream_t s, uint8_t *rows, size_t row_bytes, size_t) {
                   a.recs = recs;
                   hipLaunchKernelGGL(k_screen, dim3(blocks), dim3(SC_TPB), 0, s, a, rows, row_bytes);
               });
}

// what rb_graph_represented and rb_graph_represented_then_add refuse alike, before either looks at n ...
void repr_refuse(const char *who, const rb_graph *g, const rb_graph *gate, int lookahead, int max_indel, int max_edge_clip, float percent_identity,
                 int64_t max_visits, int64_t n) {
    RB_REQUIRE(g && gate, "%s: null handle", who);
    RB_REQUIRE(!g->shard, "%s: not available on a shard handle", who);
    RB_REQUIRE(g->dbg.bits && g->cbf, "%s: dbgbf or the counting filter has been destroyed", who);
    RB_REQUIRE(gate->dbg.bits && !gate->shard && gate->p.device == g->p.device && gate->k == g->k,
               "%s: the gate must be a filter on the same device with the same k", who);
    RB_REQUIRE(lookahead >= 0 && lookahead <= SC_MAX_LOOKAHEAD, "%s: lookahead out of range [0, %d]", who, SC_MAX_LOOKAHEAD);
    RB_REQUIRE(max_indel >= 0 && max_indel <= SC_MAX_INDEL, "%s: max_indel out of range [0, %d]", who, SC_MAX_INDEL);
    RB_REQUIRE(max_edge_clip >= 0 && max_edge_clip <= SC_MAX_DEPTH, "%s: max_edge_clip out of range [0, %d]", who, SC_MAX_DEPTH);
    RB_REQUIRE(std::isfinite(percent_identity), "%s: percent_identity is not finite", who);
    RB_REQUIRE(max_visits >= 0, "%s: max_visits = %lld", who, (long long)max_visits);
    RB_REQUIRE(n >= 0, "%s: n = %lld", who, (long long)n);
}
// ... and with n > 0: the sequences' k-mer offsets into ko, the kernel's arguments into a; returns the ints of a wavefront's alignment row in
// device scratch (0: the row stays in LDS)
size_t repr_args(const char *who, const rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, int lookahead, int max_indel, int max_edge_clip,
                 float percent_identity, int64_t max_visits, std::vector<int64_t> &ko, ScArgs &a) {
    const int k = g->k;
    ko.resize((size_t)n + 1);
    kmer_offsets(offsets, n, k, ko.data(), who);
    RB_REQUIRE(offsets[n] == offsets[0] || seq, "%s: null sequence text", who);
    const int64_t visits = max_visits ? max_visits : RB_SCREEN_DEFAULT_VISITS, longest = longest_list(ko, n);
    a.what = 0; a.lookahead = lookahead; a.max_depth = max_edge_clip; a.max_indel = max_indel; a.percent_identity = percent_identity;
    a.max_visits = (int)std::min<int64_t>(visits, INT32_MAX);
    // a walk row: an edge walk is bounded by a stretch of the sequence, a gap's path by max(2k - 1, d + k) + max_indel (a gap narrower than k
    // widens to 2k - 1 k-mers at the most), a depth search's stack by max_edge_clip and by its budget
    const int64_t cap = std::max<int64_t>(std::max<int64_t>(longest, std::max<int64_t>(2 * (int64_t)k, (int64_t)g->read_d + k) + max_indel),
                                          std::min<int64_t>(max_edge_clip, visits));
    RB_REQUIRE(cap <= SC_MAX_ROW, "%s: a walk row of %lld entries (at most %d: a sequence of that many k-mers)", who, (long long)cap, SC_MAX_ROW);
    a.cap = (int)cap;
    a.recs = nullptr;
    const size_t letters = (size_t)(longest ? longest + k - 1 : 0);
    return letters > (size_t)LEV_LDS ? letters : 0;
}

void represented_call(rb_graph *g, const rb_graph *gate, const char *seq, const int64_t *offsets, int64_t n, int lookahead, int max_indel,
                      int max_edge_clip, float percent_identity, int64_t max_visits, rb_repr_rec *out) {
    const char *who = "rb_graph_represented";
    repr_refuse(who, g, gate, lookahead, max_indel, max_edge_clip, percent_identity, max_visits, n);
    if (n == 0) return;
    RB_REQUIRE(offsets && out, "%s: null argument", who);
    std::vector<int64_t> ko;
    ScArgs a{};
    const size_t lev_cols = repr_args(who, g, seq, offsets, n, lookahead, max_indel, max_edge_clip, percent_identity, max_visits, ko, a);
    screen_run(g, gate, seq, offsets, n, who, "represented", a, ko, repr_blank(RB_SCREEN_NO_KMER), lev_cols, out,
               [](ScArgs &a, rb_repr_rec *recs, unsigned blocks, hipStream_t s, uint8_t *rows, size_t row_bytes, size_t lev_off) {
                   a.reprs = recs;
                   hipLaunchKernelGGL(k_represented, dim3(blocks), dim3(SC_TPB), 0, s, a, rows, row_bytes, lev_off);
               });
}

// rb_graph_represented_then_add: the pieces as screen_run cuts them, one k_represented_walk a piece, in order.  The gate is written: unique
// lock on it, shared lock on g (the lease), in address order.  The piece loop ends at a piece whose walker stopped; the records behind the
// stop are filled here.
void represented_then_add_call(rb_graph *g, rb_graph *gate, const char *seq, const int64_t *offsets, int64_t n, int lookahead, int max_indel,
                               int max_edge_clip, float percent_identity, int64_t max_visits, rb_repr_rec *out, uint8_t *keep, float *median,
                               int64_t *n_done) {
    const char *who = "rb_graph_represented_then_add";
    repr_refuse(who, g, gate, lookahead, max_indel, max_edge_clip, percent_identity, max_visits, n);
    RB_REQUIRE(gate != g, "%s: the gate is written and the graph is read: they must be two handles", who);
    if (n == 0) return;
    RB_REQUIRE(offsets && out && keep && n_done, "%s: null argument", who);
    std::vector<int64_t> ko;
    ScArgs a{};
    const size_t lev_cols = repr_args(who, g, seq, offsets, n, lookahead, max_indel, max_edge_clip, percent_identity, max_visits, ko, a);
    WriteLock gate_lk;
    if (gate < g) gate_lk = WriteLock(gate->rw);
    RB_HIP(hipSetDevice(g->p.device));
    HostPin pin_r(out, (size_t)n * sizeof(rb_repr_rec));
    QueryLease q(g);
    if (gate > g) gate_lk = WriteLock(gate->rw);
    RB_REQUIRE(g->dbg.bits && g->cbf, "%s: dbgbf or the counting filter has been destroyed", who);
    RB_REQUIRE(gate->dbg.bits, "%s: the gate's filter has been destroyed", who);
    RB_HIP(hipStreamSynchronize(gate->stream));                 // (whatever the gate's own calls left in flight)
    for (int64_t i = 0; i < n; ++i) { out[i] = repr_blank(RB_SCREEN_NO_KMER); keep[i] = 0; }
    if (median) std::fill(median, median + n, 0.0f);
    *n_done = n;
    if (ko[(size_t)n] == 0) return;
    hipStream_t s = q.c->st;
    const int k = g->k;
    const size_t lev_off = sc_row_bytes(a.cap, k), row_bytes = lev_off + up16(lev_cols * sizeof(int));
    int64_t stopped = -1;                                        // the call's index of the sequence the walk stopped at
    for_each_host_piece(g, s, seq, offsets, ko.data(), n, "represented_then_add", [&](HostPiece &pc) {
        if (stopped >= 0) return;
        const int64_t ra = pc.ra, pn = pc.pn, pt = pc.pt;
        // b3: counts, gate bits, records, keep flags, medians, the stop index, the one wavefront's rows
        const size_t o_g = up16((size_t)pt * 4), o_rec = up16(o_g + (size_t)pt), o_keep = up16(o_rec + (size_t)pn * sizeof(rb_repr_rec)),
                     o_med = up16(o_keep + (size_t)pn), o_stop = up16(o_med + (size_t)pn * 4), o_row = o_stop + 16;
        q.c->b3.reserve(o_row + row_bytes + 16);
        uint8_t *base3 = q.c->b3.as<uint8_t>();
        a.fv = g->view(0, 0);
        a.gate = ScGate{gate->dbg.bits, gate->dbg.mod, gate->dbg.num_hash};
        a.kmul = kmul_of(k);
        a.stranded = (int)g->stranded; a.k = k; a.read_d = g->read_d;
        a.gbit = base3 + o_g;
        a.reprs = reinterpret_cast<rb_repr_rec *>(base3 + o_rec);
        PieceRows(g, *q.c, pc).into(a);
        hipLaunchKernelGGL(k_represented_walk, dim3(1), dim3(RW_TPB), 0, s, a, gate->dbg.bits, base3 + o_row, lev_off, base3 + o_keep,
                           reinterpret_cast<float *>(base3 + o_med), reinterpret_cast<int64_t *>(base3 + o_stop));
        RB_HIP(hipGetLastError());
        pc.kernels_end();
        int64_t stop = pn;
        RB_HIP(hipMemcpyAsync(out + ra, a.reprs, (size_t)pn * sizeof(rb_repr_rec), hipMemcpyDeviceToHost, s));
        RB_HIP(hipMemcpyAsync(keep + ra, base3 + o_keep, (size_t)pn, hipMemcpyDeviceToHost, s));
        if (median) RB_HIP(hipMemcpyAsync(median + ra, base3 + o_med, (size_t)pn * 4, hipMemcpyDeviceToHost, s));
        RB_HIP(hipMemcpyAsync(&stop, base3 + o_stop, 8, hipMemcpyDeviceToHost, s));
        pc.finish();                                             // the next piece is walked only if this one came to its end
        if (stop < pn) stopped = ra + stop;
    });
    if (stopped >= 0) {
        *n_done = stopped;
        for (int64_t i = stopped + 1; i < n; ++i) { out[i] = repr_blank(RB_SCREEN_NOT_REACHED); keep[i] = 0; }
        if (median) std::fill(median + stopped + 1, median + n, 0.0f);
    }
}

}  // namespace

extern "C" {
int rb_graph_screen_fragments(rb_graph *g, const rb_graph *gate, const char *seq, const int64_t *offsets, int64_t n, int what, int lookahead,
                              int max_depth, int64_t max_visits, rb_screen_rec *out) {
    return guarded([&] { screen_call(g, gate, seq, offsets, n, what, lookahead, max_depth, max_visits, out); });
}
int rb_graph_represented(rb_graph *g, const rb_graph *gate, const char *seq, const int64_t *offsets, int64_t n, int lookahead, int max_indel,
                         int max_edge_clip, float percent_identity, int64_t max_visits, rb_repr_rec *out) {
    return guarded([&] { represented_call(g, gate, seq, offsets, n, lookahead, max_indel, max_edge_clip, percent_identity, max_visits, out); });
}
int rb_graph_represented_then_add(rb_graph *g, rb_graph *gate, const char *seq, const int64_t *offsets, int64_t n, int lookahead, int max_indel,
                                  int max_edge_clip, float percent_identity, int64_t max_visits, rb_repr_rec *out, uint8_t *keep, float *median,
                                  int64_t *n_done) {
    return guarded([&] {
        represented_then_add_call(g, gate, seq, offsets, n, lookahead, max_indel, max_edge_clip, percent_identity, max_visits, out, keep, median, n_done);
    });
}
}  // extern "C"
