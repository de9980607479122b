// rb_join.hip — joining of read pairs through the graph (rb_graph_join_pairs): GraphUtils.join (R/util/GraphUtils.java:892-1147), the second half of
// overlapAndConnect, on the device.  ONE kernel, a wavefront per pair: the pair's two paths — per k-mer both strands' hashes and the count, per
// letter a 2-bit code in a byte — live in a row of device scratch that the wavefront owns while it works on the pair.  On a single neighbour
// the wavefront walks: four lanes probe the four bases (rb_lookup.hpp), all lanes sweep the stored forward hashes 64 at a time for the
// reference's HashSet.contains / indexOf and confirm every hit on the bases (Kmer.equals).  At a fork it calls the branch step itself — ex_one of
// rb_extend_step.hpp, the body of rb_graph_extend_se — with the path's last min(size, d) k-mers where they lie in the row, and consumes the
// k-mers the step returns (:986-1023, :1112-1141) before it walks on.  Nothing is written to the graph (DESIGN.md §5 "Joining of read pairs").
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rb_pieces.hpp"
#include "rb_extend_step.hpp"

using namespace rb;

// Java float arithmetic: a threshold is one float32 product
#pragma clang fp contract(off)

namespace {

constexpr int JN_TPB = 256;
constexpr int JN_WAVES = JN_TPB / 64;            // pairs a workgroup works on at a time: a wavefront each
constexpr int64_t JN_MAX_ROWS = 4096;            // wavefronts of a launch (each owns one row of device scratch and takes pairs in turn) ...
constexpr int64_t JN_MIN_ROWS = 64;
constexpr size_t JN_ROWS_BYTES = (size_t)512 << 20;   // ... fewer when the rows are large: as many as fit this, JN_MIN_ROWS at the least

// A row, for K k-mers of paths (a pair's capacity: nkL + nkR + 2 A, A = bound + d + 2 the most one walk adds) — F[K], R[K], count[K], the
// letters' codes [K + 2 (k - 1)] — and what the branch step reads and writes for ONE sequence: its k-mer offsets {0, nt}, its record, the packed
// codes of the letters it asks for (the last k-mer's), its result's bases and counts, and for d > EX_LDS_D the rows of its walks.
struct JnLayout {
    size_t o_f, o_r, o_c, o_t, o_kof, o_rec, o_codes, o_ob, o_oc, o_walk, bytes;
    int words;                                   // 64-bit words of packed codes: d + k - 1 letters
    __host__ __device__ JnLayout(int64_t K, int k, int d, bool lds) {
        words = (d + k - 1 + 31) / 32 + 1;
        o_f = 0; o_r = o_f + (size_t)K * 8; o_c = o_r + (size_t)K * 8; o_t = up16(o_c + (size_t)K * 4);
        o_kof = up16(o_t + (size_t)K + 2 * (size_t)(k - 1));
        o_rec = o_kof + 16; o_codes = o_rec + up16(sizeof(rb_extend_rec)); o_ob = o_codes + (size_t)words * 8;
        o_oc = up16(o_ob + (size_t)d + 2); o_walk = up16(o_oc + ((size_t)d + 2) * 4);
        bytes = up16(o_walk + (lds ? 0 : ex_row_bytes(d)));
    }
};

struct JnArgs {
    FilterView fv;
    PairView pf;
    int stranded, k, d, bound, A;
    float grad, min_cov;
    int64_t pn, rowK;
    const int64_t *kof;                          // [2 pn + 1] k-mer offsets of the piece's reads: pair i's left read is sequence 2 i, its right read 2 i + 1
    const uint64_t *F, *R;                       // their getKmers rows
    const float *cnt;
    const uint64_t *codes;                       // the piece's batch
    const uint32_t *valid, *woff;
    const int64_t *oof;                          // [pn + 1] the pairs' places in out
    uint8_t *out;
    rb_join_rec *recs;
    uint8_t *rows;
    const uint32_t *ones, *zero;                 // all bits set (the step's `valid`: a path holds A C G T only); one 0 (its word offset)
    const float *floor1;                         // min_cov, as the step's floor
};

// a path as the wavefront holds it: per k-mer arrays and the letters' codes, both indexed by the k-mer's START in the text.  The left path's text
// grows at its end; the right path is the right read's list reversed, so entry i of rightPath is the k-mer at nk0 - 1 - i and the text grows at
// its front, into the A places in front of position 0.
struct JnPath {
    uint64_t *F, *R;
    float *C;
    uint8_t *T;
    int nk0, n, cap;                             // the read's k-mers, the path's size, the most it may hold
};

__device__ __forceinline__ bool jn_equal(const uint8_t *x, const uint8_t *y, int k) {
    bool eq = true;
    for (int q = 0; q < k && eq; ++q) eq = x[q] == y[q];
    return eq;
}
// the first (or last) position in [lo, hi) whose k-mer equals the k-mer at cand (forward hash bf), or WAVE_NOWHERE: a path's entries go by their start in its text
__device__ __forceinline__ int jn_find(const JnPath &p, int lo, int hi, uint64_t bf, const uint8_t *cand, int k, bool last, uint32_t lane) {
    return wave_find(lo, hi, k, [&](int j) { return p.F[j]; }, bf, [&](int j, int q) { return p.T[j + q]; }, [&](int q) { return cand[q]; }, last, lane);
}
// getMinimumKmerCoverage over positions [lo, hi), lo < hi
__device__ __forceinline__ float jn_min(const float *c, int lo, int hi, uint32_t lane) {
    return wave_min(lo, hi, [&](int j) { return c[j]; }, lane);
}

struct JnResult { int why, index, left_keep, right_from; };   // a returned list: leftPath[0, left_keep) + the right text's k-mers from position right_from

// One walk of join — the left walk (:912-1030, rw false: `own` is leftPath, `other` the right list) or the right walk (:1032-1144, rw true: `own` is
// rightPath, `other` leftPath as the left walk left it).  Returns 0 when the walk ended without a result (the caller goes on), 1 when it returned a
// list (res), 2 when it returned null.  end: how it ended; forks: the branch steps taken; thr: the walk's threshold.
__device__ __forceinline__ int jn_walk(const JnArgs &a, ExArgs &ea, uint8_t *xrow, const JnLayout &lay, uint8_t *row, bool rw, JnPath &own, const JnPath &other, int other_n,
                       const uint8_t *left_last, float &thr, int &end, int &forks, JnResult &res, uint32_t lane) {
    const int k = a.k, d = a.d;
    const float g = a.grad, m = a.min_cov;
    const WaveDir<> dr = wave_dir(a.stranded, k, rw ? 1 : 0);
    const int max_size = a.bound + own.n;
    auto pos_of = [&](int i) { return rw ? own.nk0 - 1 - i : i; };
    // One k-mer offered to the path — `best` (ext false) or a k-mer of a step's result (ext true): base in, count cf.  0: added; 1: the walk ends
    // (end set); 2: a list is returned (res set); 3: null is returned (end set).
    auto offer = [&](uint32_t in, float cf, bool ext) -> int {
        if (own.n >= own.cap) { end = RB_JOIN_END_BOUND; return 1; }     // (never: a walk adds at most bound - 1 + d + 1 k-mers, the row has room for bound + d + 2)
        const int lp = pos_of(own.n - 1), np = pos_of(own.n);
        const uint64_t lf = own.F[lp], lr = own.R[lp];
        uint64_t nA, nB;
        dr.step(rw ? lr : lf, rw ? lf : lr, own.T[rw ? lp + k - 1 : lp], in, nA, nB);
        const uint64_t bf = dr.fwd(nA, nB), br = rw ? nA : nB;
        if (lane == 0) own.T[rw ? np : np + k - 1] = (uint8_t)in;
        wave_fence();
        const uint8_t *cand = own.T + np;
        if (!rw) {
            const int j = jn_find(other, 0, other_n, bf, cand, k, false, lane);                                  // :946-967, :987-1008
            if (j == 0) { res = JnResult{RB_JOIN_WHY_REACHED_RIGHT, -1, own.n, 0}; return 2; }
            if (j > 0) {
                const float path_cov = jn_min(own.C, max(0, own.n - j), own.n, lane), dangling = jn_min(other.C, 0, j, lane);
                if (dangling < path_cov) { res = JnResult{RB_JOIN_WHY_INSIDE_RIGHT, j, own.n, j}; return 2; }
            }
            const bool homo = wave_all_equal(cand, k, lane);
            if (ext) { if (homo) { end = RB_JOIN_END_EXT_HOMOPOLYMER; return 1; } }                             // :1010
            else if (homo || jn_find(own, 0, own.n, bf, cand, k, false, lane) != WAVE_NOWHERE) { end = RB_JOIN_END_LOOP; return 1; }   // :969
        } else {
            const int i = jn_find(other, 0, other_n, bf, cand, k, true, lane);                                  // :1068-1094, :1113-1128
            if (i != WAVE_NOWHERE) {
                if (!ext && jn_equal(cand, left_last, k)) res = JnResult{RB_JOIN_WHY_REACHED_LEFT, -1, -1, pos_of(own.n - 1)};
                else res = JnResult{RB_JOIN_WHY_PATHS_MEET, i, i + 1, pos_of(own.n - 1)};
                return 2;
            }
            if (wave_all_equal(cand, k, lane)) { end = ext ? RB_JOIN_END_EXT_HOMOPOLYMER : RB_JOIN_END_LOOP; return 3; }   // :1096, :1129
            if (!ext && jn_find(own, pos_of(own.n - 1), own.nk0, bf, cand, k, false, lane) != WAVE_NOWHERE) { end = RB_JOIN_END_LOOP; return 3; }
        }
        if (lane == 0) { own.F[np] = bf; own.R[np] = br; own.C[np] = cf; }
        ++own.n;
        wave_fence();
        if (ext) {                                                                                              // :1018-1021, :1136-1139
            const float c = g * cf;
            if (c < thr) thr = fmaxf(c, m);
        }
        return 0;
    };
    while (own.n < max_size) {
        // the neighbours with count >= m in the order A C G T (Kmer.getSuccessors / getPredecessors(k, numHash, graph, minKmerCov)): lane b asks for base b
        const int lp = pos_of(own.n - 1);
        float cf = 0.0f;
        if (lane < 4u) {
            const uint64_t lf = own.F[lp], lr = own.R[lp];
            uint64_t nA, nB;
            dr.step(rw ? lr : lf, rw ? lf : lr, own.T[rw ? lp + k - 1 : lp], lane, nA, nB);
            cf = count_code_value(count_code(a.fv, dr.hash(nA, nB)));
        }
        uint32_t m4 = (uint32_t)__ballot(lane < 4u && cf >= m) & 0xFu;
        if (m4 == 0u) { end = RB_JOIN_END_NO_NEIGHBOR; return 0; }
        if (__popc(m4) > 1) m4 &= ~(uint32_t)__ballot(lane < 4u && cf < thr);                                  // :932-937
        if (__popc(m4) == 1) {
            const int b = __builtin_ctz(m4);
            const float bc = __shfl(cf, b, 64);
            thr = fmaxf(m, fminf(thr, bc * g));                                                                 // :929, :941
            const int st = offer((uint32_t)b, bc, false);
            if (st == 1) return 0;
            if (st >= 2) return st - 1;
            continue;
        }
        // a fork (none or several pass the threshold): extendRightSE(leftPath, ..., minKmerCov) / extendLeftSE(rightPath, ...) of the last min(size, d) k-mers
        ++forks;
        const int nt = min(own.n, d), tp = rw ? lp : lp - nt + 1;                                               // the tail's first position in the text
        ea.direction = rw ? 1 : 0;
        ea.F = own.F + tp; ea.R = own.R + tp; ea.cnt = own.C + tp;
        {   // the letters the step reads: the last k-mer's, at nt - 1 .. nt + k - 2 of the tail's text (left-hand direction: 0 .. k - 1)
            uint64_t *cw = reinterpret_cast<uint64_t *>(row + lay.o_codes);
            const int p_lo = rw ? 0 : nt - 1, p_hi = p_lo + k - 1;
            const int w = (p_lo >> 5) + (int)lane;
            if (w <= (p_hi >> 5)) {
                uint64_t word = 0;
                for (int bq = 0; bq < 32; ++bq) {
                    const int p = 32 * w + bq;
                    if (p >= p_lo && p <= p_hi) word |= (uint64_t)own.T[tp + p] << (2 * bq);
                }
                cw[w] = word;
            }
            if (lane == 0) reinterpret_cast<int64_t *>(row + lay.o_kof)[1] = nt;
        }
        wave_fence();
        ex_one<false>(ea, 0, xrow, lane);
        wave_fence();
        const rb_extend_rec *er = reinterpret_cast<const rb_extend_rec *>(row + lay.o_rec);
        const int ne = er->outcome == RB_EXT_NONE ? 0 : er->out_len;
        if (ne == 0) { end = RB_JOIN_END_STEP_NONE; return 0; }                                                 // :980, :1108
        const uint8_t *eb = row + lay.o_ob;
        const float *ec = reinterpret_cast<const float *>(row + lay.o_oc);
        for (int i = 0; i < ne; ++i) {
            const int st = offer(letter_code(eb[i]), ec[i], true);
            if (st == 1) return 0;
            if (st >= 2) return st - 1;
        }
    }
    end = RB_JOIN_END_BOUND;
    return 0;
}

// join of pair r of the piece by one wavefront with `row`
__device__ __forceinline__ void jn_one(const JnArgs &a, ExArgs &ea, uint8_t *xrow, const JnLayout &lay, uint8_t *row, int64_t r, uint32_t lane) {
    const int k = a.k;
    rb_join_rec v;
    v.outcome = RB_JOIN_NOT_JUDGED; v.why = RB_JOIN_WHY_SHORT; v.l_end = v.r_end = RB_JOIN_END_NOT_RUN;
    v.l_added = v.r_added = v.l_forks = v.r_forks = 0; v.index = -1; v.out_len = 0; v.l_threshold = v.r_threshold = 0.0f;
    const int64_t k0 = a.kof[2 * r], k1 = a.kof[2 * r + 1];
    const int nkL = (int)(k1 - k0), nkR = (int)(a.kof[2 * r + 2] - k1);
    if (nkL == 0 || nkR == 0) {                               // a read with fewer than k letters: the reference throws in get(0)
        if (lane == 0) a.recs[r] = v;
        return;
    }
    const int lenL = nkL + k - 1, lenR = nkR + k - 1;
    JnPath L, R;
    L.F = reinterpret_cast<uint64_t *>(row + lay.o_f); L.R = reinterpret_cast<uint64_t *>(row + lay.o_r); L.C = reinterpret_cast<float *>(row + lay.o_c);
    L.T = row + lay.o_t;
    L.nk0 = L.n = nkL; L.cap = nkL + a.A;
    R.F = L.F + L.cap + a.A; R.R = L.R + L.cap + a.A; R.C = L.C + L.cap + a.A; R.T = L.T + (L.cap + k - 1) + a.A;
    R.nk0 = R.n = nkR; R.cap = nkR + a.A;
    // a letter outside ACGTU in either read: the pair is not judged; else the reads' letters as codes, a byte each
    if (wave_bad_letter(a.valid + a.woff[2 * r], lenL, lane) || wave_bad_letter(a.valid + a.woff[2 * r + 1], lenR, lane)) {
        v.why = RB_JOIN_WHY_INVALID_LETTER;
        if (lane == 0) a.recs[r] = v;
        return;
    }
    for (int s = 0; s < 2; ++s) {
        const uint64_t *cw = a.codes + a.woff[2 * r + s];
        uint8_t *t = s ? R.T : L.T;
        for (int p = (int)lane; p < (s ? lenR : lenL); p += 64) t[p] = (uint8_t)((cw[p >> 5] >> (2 * (p & 31))) & 3u);
    }
    for (int j = (int)lane; j < nkL; j += 64) { L.F[j] = a.F[k0 + j]; L.R[j] = a.R[k0 + j]; L.C[j] = a.cnt[k0 + j]; }
    for (int j = (int)lane; j < nkR; j += 64) { R.F[j] = a.F[k1 + j]; R.R[j] = a.R[k1 + j]; R.C[j] = a.cnt[k1 + j]; }
    wave_fence();

    // the left walk, then — unless it returned — the right walk: one body, run twice
    JnResult res{RB_JOIN_WHY_EXHAUSTED, -1, 0, 0};
    int st = 0;
    for (int rw = 0; rw < 2 && st == 0; ++rw) {
        JnPath own = rw ? R : L;
        const JnPath other = rw ? L : R;
        float thr = fmaxf(a.min_cov, jn_min(own.C, 0, own.nk0, lane) * a.grad);                                 // :912, :1033
        int end = RB_JOIN_END_NOT_RUN, forks = 0;
        st = jn_walk(a, ea, xrow, lay, row, rw != 0, own, other, other.n, L.T + (nkL - 1), thr, end, forks, res, lane);
        if (st == 1) end = RB_JOIN_END_RETURNED;
        if (rw) { R.n = own.n; v.r_added = own.n - nkR; v.r_threshold = thr; v.r_end = end; v.r_forks = forks; }
        else { L.n = own.n; v.l_added = own.n - nkL; v.l_threshold = thr; v.l_end = end; v.l_forks = forks; }
    }
    if (st == 1 && res.left_keep < 0) res.left_keep = nkL;
    if (st == 2) res.why = RB_JOIN_WHY_RIGHT_LOOP;
    v.why = res.why;
    v.outcome = RB_JOIN_NONE;
    if (st == 1) {
        // the string the list spells: the kept left path's text, then the last letter of every right k-mer from right_from on
        const int nl = res.left_keep + k - 1, nr = nkR - res.right_from;
        uint8_t *o = a.out + a.oof[r];
        for (int p = (int)lane; p < nl; p += 64) o[p] = code_letter(L.T[p]);
        for (int q = (int)lane; q < nr; q += 64) o[nl + q] = code_letter(R.T[res.right_from + k - 1 + q]);
        v.outcome = RB_JOIN_JOINED; v.index = res.index; v.out_len = nl + nr;
    }
    if (lane == 0) a.recs[r] = v;
}

// A wavefront per pair, taking pairs in turn.  LDS_ROW: the rows of the branch step's walks are in LDS (d <= EX_LDS_D); else in the wavefront's row.
template <bool LDS_ROW>
__global__ void __launch_bounds__(JN_TPB) k_join(JnArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_row[JN_WAVES][LDS_ROW ? ex_row_bytes(EX_LDS_D) : 16];
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;     // (one value a wavefront: the row's addresses stay scalar)
    const int64_t slot = (int64_t)blockIdx.x * JN_WAVES + wv, n_slots = (int64_t)gridDim.x * JN_WAVES;
    const JnLayout lay(a.rowK, a.k, a.d, LDS_ROW);
    uint8_t *row = a.rows + (size_t)slot * lay.bytes;
    uint8_t *xrow;
    if constexpr (LDS_ROW) xrow = s_row[wv]; else xrow = row + lay.o_walk;
    // the step's view of ONE sequence, r = 0: its tail's rows are set at every fork, the rest here
    ExArgs ea;
    ea.fv = a.fv; ea.pf = a.pf;
    ea.stranded = a.stranded; ea.k = a.k; ea.d = a.d; ea.direction = 0; ea.D = LDS_ROW ? EX_LDS_D : a.d;
    ea.pn = 1;
    ea.kof = reinterpret_cast<const int64_t *>(row + lay.o_kof);
    ea.F = ea.R = nullptr; ea.cnt = nullptr;
    ea.codes = reinterpret_cast<const uint64_t *>(row + lay.o_codes); ea.valid = a.ones; ea.woff = a.zero;
    ea.floors = a.floor1;
    ea.out_b = row + lay.o_ob; ea.out_c = reinterpret_cast<float *>(row + lay.o_oc);
    ea.recs = reinterpret_cast<rb_extend_rec *>(row + lay.o_rec);
    if (lane == 0) reinterpret_cast<int64_t *>(row + lay.o_kof)[0] = 0;
    for (int64_t r = slot; r < a.pn; r += n_slots) {
        jn_one(a, ea, xrow, lay, row, r, lane);
        wave_fence();
    }
}

void join_call(rb_graph *g, const char *lseq, const int64_t *lo, const char *rseq, const int64_t *ro, int64_t n, int bound, float grad, int max_tip_len,
               float min_cov, int64_t *out_offsets, char *out_seq, rb_join_rec *recs) {
    const char *who = "rb_graph_join_pairs";
    (void)max_tip_len;                                        // (the branch step does not read it: rb_capi.h, rb_graph_naive_extend)
    RB_REQUIRE(g, "%s: null handle", who);
    RB_REQUIRE(!g->shard, "%s: not available on a shard handle", who);
    RB_REQUIRE(g->dbg.bits && g->cbf, "%s: dbgbf or the counting filter has been destroyed", who);
    RB_REQUIRE(g->rpk.bits, "%s: the graph has no read-paired k-mer filter (created without useReadPairedKmers, or destroyed)", who);
    const int d = g->read_d, k = g->k;
    RB_REQUIRE(d >= 2, "%s: the read-paired k-mer distance is %d (the branch step needs d >= 2)", who, d);
    RB_REQUIRE(bound >= 0 && bound <= RB_JOIN_MAX_BOUND, "%s: bound = %d (0 .. %d)", who, bound, RB_JOIN_MAX_BOUND);
    RB_REQUIRE(std::isfinite(grad) && grad >= 0.0f, "%s: max_cov_gradient must be finite and not negative", who);
    RB_REQUIRE(std::isfinite(min_cov) && min_cov >= 0.0f, "%s: min_kmer_cov must be finite and not negative", who);
    RB_REQUIRE(n >= 0, "%s: n = %lld", who, (long long)n);
    if (n == 0) return;
    RB_REQUIRE(lo && ro && out_offsets, "%s: null argument", who);
    RB_REQUIRE(recs || !out_seq, "%s: out_seq needs recs", who);
    // the reads as one list of sequences, pair i's left read at 2 i and its right read at 2 i + 1
    std::vector<int64_t> off((size_t)(2 * n + 1), 0), ko((size_t)(2 * n + 1), 0);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t ll = lo[i + 1] - lo[i], rl = ro[i + 1] - ro[i];
        RB_REQUIRE(ll >= 0 && rl >= 0, "%s: decreasing offsets at pair %lld", who, (long long)i);
        RB_REQUIRE(ll + rl <= INT32_MAX / 2, "%s: pair %lld has more letters than a row holds", who, (long long)i);
        off[(size_t)(2 * i + 1)] = off[(size_t)(2 * i)] + ll;
        off[(size_t)(2 * i + 2)] = off[(size_t)(2 * i + 1)] + rl;
    }
    RB_REQUIRE((lo[n] == lo[0] || lseq) && (ro[n] == ro[0] || rseq), "%s: null sequence text", who);
    kmer_offsets(off.data(), 2 * n, k, ko.data(), nullptr);
    // the capacity layout: the text of nkL + nkR + 2 (bound + d + 2) k-mers a pair
    const int A = bound + d + 2;
    auto cap_kmers = [&](int64_t i) { return ko[(size_t)(2 * i + 2)] - ko[(size_t)(2 * i)] + 2 * (int64_t)A; };
    out_offsets[0] = 0;
    for (int64_t i = 0; i < n; ++i) out_offsets[i + 1] = out_offsets[i] + cap_kmers(i) + k - 1;
    if (!out_seq) return;
    std::vector<char> text((size_t)off[(size_t)(2 * n)]);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t ll = lo[i + 1] - lo[i], rl = ro[i + 1] - ro[i];
        if (ll) memcpy(text.data() + off[(size_t)(2 * i)], lseq + lo[i], (size_t)ll);
        if (rl) memcpy(text.data() + off[(size_t)(2 * i + 1)], rseq + ro[i], (size_t)rl);
    }
    RB_HIP(hipSetDevice(g->p.device));
    HostPin pin_out(out_seq, (size_t)out_offsets[n]), pin_rec(recs, (size_t)n * sizeof(rb_join_rec));
    QueryLease q(g);
    hipStream_t s = q.c->st;
    const bool lds = d <= EX_LDS_D;
    // what no kernel touches: the pairs of pieces without a k-mer (a pair without one comes back like this from the kernel too)
    for (int64_t i = 0; i < n; ++i) {
        if (ko[(size_t)(2 * i + 2)] > ko[(size_t)(2 * i)]) continue;
        rb_join_rec v;
        memset(&v, 0, sizeof v);
        v.outcome = RB_JOIN_NOT_JUDGED; v.why = RB_JOIN_WHY_SHORT; v.index = -1;
        recs[i] = v;
        memset(out_seq + out_offsets[i], 0, (size_t)(out_offsets[i + 1] - out_offsets[i]));
    }
    // piece by piece (rb_pieces.hpp), a pair a record, cut by the k-mers of both reads: b0 the piece's tables, b1 / b2 the getKmers hashes, b3 counts,
    // records, the text out, the step's constants and the wavefronts' rows; with profiling on the kernels of every piece are timed: entry "join"
    std::vector<int64_t> oof;
    for_each_host_piece(g, s, text.data(), off.data(), ko.data(), n, "join", [&](HostPiece &pc) {
        const int64_t ra = pc.ra, rb_ = pc.rb, pn = pc.pn, pt = pc.pt;
        const int64_t ot = out_offsets[rb_] - out_offsets[ra];
        int64_t rowK = 0;
        oof.resize((size_t)pn + 1);
        for (int64_t i = 0; i <= pn; ++i) oof[(size_t)i] = out_offsets[ra + i] - out_offsets[ra];
        for (int64_t i = ra; i < rb_; ++i) rowK = std::max(rowK, cap_kmers(i));
        const JnLayout lay(rowK, k, d, lds);
        const int64_t rows = std::min(std::min(pn, JN_MAX_ROWS), std::max(JN_MIN_ROWS, (int64_t)(JN_ROWS_BYTES / lay.bytes)));
        const unsigned blocks = blocks_for(rows, JN_WAVES);
        const size_t n_ones = (size_t)lay.words * 2 + 2;
        const size_t o_rec = up16((size_t)pt * 4), o_txt = o_rec + (size_t)pn * sizeof(rb_join_rec), o_const = up16(o_txt + (size_t)ot),
                     o_rows = up16(o_const + 16 + n_ones * 4);
        q.c->b3.reserve(o_rows + (size_t)blocks * JN_WAVES * lay.bytes + 16);
        uint8_t *base3 = q.c->b3.as<uint8_t>();
        JnArgs a;
        a.fv = g->view(0, 0);
        a.pf = PairView{g->rpk.bits, g->rpk.mod, g->rpk.num_hash, kmul_of(k)};
        a.stranded = (int)g->stranded; a.k = k; a.d = d; a.bound = bound; a.A = A;
        a.grad = grad; a.min_cov = min_cov;
        a.rowK = rowK;
        a.out = base3 + o_txt;
        a.recs = reinterpret_cast<rb_join_rec *>(base3 + o_rec);
        a.rows = base3 + o_rows;
        a.floor1 = reinterpret_cast<float *>(base3 + o_const);
        a.zero = reinterpret_cast<uint32_t *>(base3 + o_const + 4);
        a.ones = reinterpret_cast<uint32_t *>(base3 + o_const + 16);
        RB_HIP(hipMemsetAsync(base3 + o_txt, 0, o_const + 16 - o_txt, s));          // (what no pair writes comes back as zeros, whatever the cuts)
        RB_HIP(hipMemsetAsync(base3 + o_const + 16, 0xFF, n_ones * 4, s));
        RB_HIP(hipMemcpyAsync(base3 + o_const, &min_cov, 4, hipMemcpyHostToDevice, s));
        PieceRows(g, *q.c, pc, oof.data(), oof.size()).into(a);
        a.oof = a.kof + 2 * pn + 1;
        if (lds) hipLaunchKernelGGL((k_join<true>), dim3(blocks), dim3(JN_TPB), 0, s, a);
        else hipLaunchKernelGGL((k_join<false>), dim3(blocks), dim3(JN_TPB), 0, s, a);
        RB_HIP(hipGetLastError());
        pc.kernels_end();
        RB_HIP(hipMemcpyAsync(recs + ra, a.recs, (size_t)pn * sizeof(rb_join_rec), hipMemcpyDeviceToHost, s));
        RB_HIP(hipMemcpyAsync(out_seq + out_offsets[ra], a.out, (size_t)ot, hipMemcpyDeviceToHost, s));
    }, 2);
}

}  // namespace

extern "C" {
int rb_graph_join_pairs(rb_graph *g, const char *lseq, const int64_t *loffsets, const char *rseq, const int64_t *roffsets, int64_t n, int bound,
                        float max_cov_gradient, int max_tip_len, float min_kmer_cov, int64_t *out_offsets, char *out_seq, rb_join_rec *recs) {
    return guarded([&] { join_call(g, lseq, loffsets, rseq, roffsets, n, bound, max_cov_gradient, max_tip_len, min_kmer_cov, out_offsets, out_seq, recs); });
}
}  // extern "C"
