// rb_extend_step.hpp — the paired-k-mer branch step on the device, once: GraphUtils.extendRightSE / extendLeftSE (R/util/GraphUtils.java:6018-6204) and,
// as a compile-time variant, extendRightPE / extendLeftPE (:6206-6414) of ONE sequence by ONE wavefront (ex_one), with the naive walks, the pair
// counts and the repeat scan it is made of.  rb_extend.hip runs it over host sequences (rb_graph_extend_se / rb_graph_extend_pe: k_extend); rb_join.hip
// calls it where a walk of GraphUtils.join stands at a fork, with the path's tail where it lies in device memory (k_join); rb_extend_loop.hip
// calls it round after round on a sequence that grows in a row of device memory (k_extloop), letters included (ExRowText).  Everything is in an
// unnamed namespace: a unit that includes this gets its own copy, inlined into its kernels.
#pragma once
#include <math.h>

#include <type_traits>

#include "rb_pipeline.hpp"
#include "rb_lookup.hpp"
#include "rb_repeat.hpp"
#include "rb_wave.hpp"

// Java float arithmetic: the score is one float32 product and one float32 quotient, the median of an even number of counts one sum and one quotient
#pragma clang fp contract(off)

namespace rb {
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
__device__ void ex_run_walks(const FilterView &fv, const WaveDir<> &dr, float min_cov, const ExChain &ch, uint8_t *crow, uint8_t *brow, ExWalk &w, uint32_t lane) {
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
        const uint64_t bA = wave_shfl64(nA, src), bB = wave_shfl64(nB, src);
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
        wave_fence();
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
//   PE — countKmerPairsPE / countKmerPairsReversedPE (:5792-5888): d is the fragment-paired distance, and walked k-mer i has two partners, slot
// nt - d_r + i in pf (the read-pair filter) and slot nt - d + i in ff (the fragment-pair filter), each looked up only where its slot lies
// in [0, nt); the reference's loop ends once both slots have run off the list, which is when neither test holds any more.  Neither distance
// is assumed the larger.  fpairs counts the fragment pairs, last is the largest i either filter supports.  Here k-mers below i0 are NOT
// known to be without support — a first stretch reaches the second level with support of one kind — so the caller adds what the first
// stretch's own count gave for them (the same i, the same slots: min(d - 1, n - 1) only grows with n).
struct ExPairs { int pairs, fpairs, last; };
template <bool PE>
__device__ ExPairs ex_count_pairs(const PairView &pf, const PairView &ff, int d_r, const WaveDir<> &dr, const ExChain &ch, const ExTail &tl, int d, int n, int i0, uint32_t lane) {
    const int hi = min(d - 1, n - 1), k = (int)dr.uk;
    ExPairs res{0, 0, -1};
    for (int base = i0; base <= hi; base += 64) {
        const int i = base + (int)lane, j = tl.nt - d + i, jr = PE ? tl.nt - d_r + i : j;
        const bool ask_f = i <= hi && j >= 0 && (!PE || j < tl.nt), ask_r = PE ? (i <= hi && jr >= 0 && jr < tl.nt) : ask_f;
        bool hit = false, fhit = false;
        if (ask_r || ask_f) {
            uint64_t A = 0, B = 0;
            for (int q = 0; q < k; ++q) {
                A = rotl(A, 1) ^ seed_of(ch.base(i + 1 + q) ^ dr.xm);
                B = rotl(B, 1) ^ seed_of(ch.base(i + k - q) ^ dr.ym);
            }
            const uint64_t f = dr.left ? B : A, r = dr.left ? A : B;
            auto key_of = [&](int slot) {
                const uint64_t pfw = tl.F[tl.at(slot)], prv = dr.stranded ? 0ull : tl.R[tl.at(slot)];
                if (!dr.left) return dr.stranded ? combine(pfw, f) : smin(combine(pfw, f), combine(r, prv));      // partner on the left
                return dr.stranded ? combine(f, pfw) : smin(combine(f, pfw), combine(prv, r));                    // partner on the right
            };
            if constexpr (PE) pair_hit2(pf, [&] { return key_of(jr); }, ask_r, ff, [&] { return key_of(j); }, ask_f, hit, fhit);   // both filters' words before either test
            else hit = pair_hit(pf, key_of(j));
        }
        const unsigned long long m = __ballot(hit);
        if (m) { res.pairs += __popcll(m); res.last = base + 63 - (int)__builtin_clzll(m); }
        if constexpr (PE) {
            const unsigned long long mf = __ballot(fhit);
            if (mf) { res.fpairs += __popcll(mf); res.last = max(res.last, base + 63 - (int)__builtin_clzll(mf)); }
        }
    }
    return res;
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
// The fragment-paired step's arguments: d above is then the FRAGMENT-paired distance (bounds, rows and the output stride follow it), pf the
// read-pair filter with its own distance d_r, ff the fragment-pair filter; t1 t2 t3 are isRepeat's thresholds for a k-mer (t1 "never" where
// the reference's signed-byte counter cannot reach it); recs stays null and the records go to recs_pe.
struct ExArgsPE : ExArgs {
    PairView ff;
    int d_r, t1, t2, t3;
    rb_extend_pe_rec *recs_pe;
};
template <bool PE> using ExArgsT = std::conditional_t<PE, ExArgsPE, ExArgs>;

// one record: fpairs and max_ext are the fragment-paired step's fields
template <bool PE>
__device__ __forceinline__ void ex_put(const ExArgsT<PE> &a, int64_t r, int outcome, int why, int n_cand, int out_len, int pairs, int fpairs, int last, int winner, float score, int max_ext) {
    if constexpr (PE) {
        rb_extend_pe_rec v;
        v.outcome = outcome; v.why = why; v.n_candidates = n_cand; v.out_len = out_len; v.read_pairs = pairs; v.frag_pairs = fpairs; v.last_partnered = last;
        v.winner = winner; v.score = score; v.max_ext = max_ext;
        a.recs_pe[r] = v;
    } else {
        rb_extend_rec v;
        v.outcome = outcome; v.why = why; v.n_candidates = n_cand; v.out_len = out_len; v.pairs = pairs; v.last_partnered = last; v.winner = winner; v.score = score;
        a.recs[r] = v;
    }
}

// the chain's first n k-mers as output: bases in walking order (upper-case A C G T) and, on request, counts
__device__ void ex_emit(const ExArgs &a, int64_t r, const ExChain &ch, const ExCodes &cc, int n, uint32_t lane) {
    const int64_t o = r * (int64_t)(a.d + 2);
    for (int i = (int)lane; i < n; i += 64) {
        const uint32_t b = ch.base(a.k + i);
        a.out_b[o + i] = code_letter(b);
        if (a.out_c) a.out_c[o + i] = count_code_value(cc.at(i));
    }
}

// Where the step reads a sequence's letters — the last k-mer's, and for PE those of the trailing k-mers — by their place p in the text the
// tail's k-mers are windows of.  Two sources: the piece's packed batch (k_extend, k_join: 2-bit codes 32 a word and a usable-letter bit
// each), and a walk's row in device memory that holds a code a byte and nothing but A C G T (k_extloop, whose sequences grow where they lie).
struct ExBatchText {
    const uint64_t *codes;
    const uint32_t *valid, *woff;                // woff: the sequence's own entry (looked up at every use: a pointer held across the walks costs k_extend registers)
    __device__ __forceinline__ const uint64_t *cw() const { return codes + *woff; }
    __device__ __forceinline__ bool usable(uint32_t p) const { return ((valid + *woff)[p >> 5] >> (p & 31u)) & 1u; }
    __device__ __forceinline__ uint32_t seed_code(uint32_t p) const { return (uint32_t)(cw()[p >> 5] >> (2u * (p & 31u))) & 3u; }
    __device__ __forceinline__ uint32_t code(uint32_t p) const { return base_at(reinterpret_cast<const uint32_t *>(cw()), p); }
    __device__ __forceinline__ bool window_is_repeat(uint32_t p, int k, int t1, int t2, int t3) const {
        return rb::window_is_repeat(reinterpret_cast<const uint32_t *>(cw()), p, k, t1, t2, t3);
    }
};
struct ExRowText {
    const uint8_t *t;
    __device__ __forceinline__ bool usable(uint32_t) const { return true; }
    __device__ __forceinline__ uint32_t seed_code(uint32_t p) const { return t[p]; }
    __device__ __forceinline__ uint32_t code(uint32_t p) const { return t[p]; }
    __device__ __forceinline__ bool window_is_repeat(uint32_t p, int k, int t1, int t2, int t3) const {
        return window_is_repeat_of([&](int j) { return (uint32_t)t[p + (uint32_t)j]; }, k, t1, t2, t3);
    }
};

// The repeat scan of extendRightPE / extendLeftPE (:6226-6233, :6333-6340): the number of trailing k-mers of the list, from the last one
// backwards, that graph.isRepeatKmer accepts (SeqUtils.isRepeat(byte[]) :458-497 of the k-mer in its natural orientation, also for the
// left-hand direction), each lowering the bound by one.  Every bound <= 0 acts alike — a walk adds one k-mer and ++extensionLength > bound
// ends it, and the second level's bound - gap (gap >= 1) is then <= 0 as well — so the scan stops once the bound would reach 0: at most
// `most` = d - 2 k-mers are tested, which the d + k - 1 letters on the device always hold when the list is that long.  A lane per k-mer
// (window_is_repeat on the batch's packed codes), a ballot, the run of leading ones.  A k-mer holding a letter outside ACGTU: the
// reference's first loop returns true if a base count reaches t1 before that letter and else indexes an array with -1 and throws; -1 is
// returned for the throw.  A bad letter further back than the scan reaches is not seen.
template <class TEXT>
__device__ int ex_trailing_repeats(const ExArgsPE &a, const TEXT &tx, int nt, int most, uint32_t lane) {
    const int k = a.k, S = min(nt, most);
    int count = 0;
    for (int base = 0; base < S; base += 64) {
        const int t = base + (int)lane;
        int verdict = 0;                                          // 0 not a repeat (or past the scan), 1 a repeat, 2 the reference throws
        if (t < S) {
            const uint32_t p = (uint32_t)(a.direction ? t : nt - 1 - t);           // the k-mer's place in the text
            int fb = 0;                                           // letters before the first one outside ACGTU
            while (fb < k && tx.usable(p + (uint32_t)fb)) ++fb;
            if (fb == k) verdict = tx.window_is_repeat(p, k, a.t1, a.t2, a.t3) ? 1 : 0;
            else {
                int c4[4] = {0, 0, 0, 0};
                for (int j = 0; j < fb; ++j) {
                    const uint32_t c = tx.code(p + (uint32_t)j);
                    c4[0] += c == 0u; c4[1] += c == 1u; c4[2] += c == 2u; c4[3] += c == 3u;
                }
                verdict = max(max(c4[0], c4[1]), max(c4[2], c4[3])) >= a.t1 ? 1 : 2;
            }
        }
        const unsigned long long not_rep = ~__ballot(verdict == 1);
        if (not_rep == 0ull) { count += 64; continue; }
        const int first = (int)__builtin_ctzll(not_rep);
        count += first;
        if ((__ballot(verdict == 2) >> first) & 1ull) return -1;
        break;
    }
    return count;
}

// extendRightSE / extendLeftSE (PE: extendRightPE / extendLeftPE, :6206-6414) of sequence r of the piece, by one wavefront with `row` for its
// walks.  What the PE step does differently is marked where it does: the bound M = d - 2 lowered by the repeat scan when there are two or
// more candidates, pathMinCov over the last min(n, d) k-mers of a list that may be longer (it holds max(d_r, d) k-mers), two pair filters,
// scoring only with support of both kinds, the two-sided skip test and the second level's bound M - gap.
//   Rows (the layout above, D >= d).  A walk adds at most max(bound, 0) + 1 k-mers.  First level: candidate + walk <= max(M, 0) + 2 <= d
// entries for every d >= 2 and every M <= d - 2, negative M included (2 <= d).  Second level: bound M - gap <= d - 3, so next candidate +
// walk <= max(d - 3, 0) + 2 = max(d - 1, 2) <= d + 2 entries.  The SE step's bounds are d - 2 and d - gap: d and d + 1 entries.
//   tx: the sequence's letters (ExBatchText, ExRowText); ex_one below is the step over the piece's batch.
template <bool PE, class TEXT>
__device__ void ex_one_on(const ExArgsT<PE> &a, int64_t r, uint8_t *row, uint32_t lane, const TEXT &tx) {
    const int k = a.k, d = a.d, D = a.D;
    const int64_t k0 = a.kof[r];
    const int nt = (int)(a.kof[r + 1] - k0);
    if (nt == 0) {                                            // shorter than k: the reference's callers never get here
        if (lane == 0) ex_put<PE>(a, r, RB_EXT_NONE, RB_EXT_WHY_SHORT, 0, 0, 0, 0, -1, -1, 0.0f, d - 2);
        return;
    }
    const int S1 = ex_l1b_stride(D), S2 = ex_l2b_stride(D), C2 = ex_l2_cap(D);
    uint8_t *l1c = row, *l2c = l1c + 4 * D, *l1b = l2c + 16 * C2, *l2b = l1b + 4 * S1, *seed = l2b + 16 * S2;
    const WaveDir<> dr = wave_dir(a.stranded, k, a.direction);
    const ExTail tl{a.F + k0, a.R + k0, nt, a.direction};
    const uint32_t in = lane & 3u;
    int d_r = d;
    if constexpr (PE) d_r = a.d_r;
    // (the fragment-pair filter's view takes the read-pair filter's kmul: both are kmul_of(k), and one copy less to hold keeps the scratch
    // instantiation at 168 registers)
    const PairView ff = [&]() -> PairView { if constexpr (PE) return PairView{a.ff.bits, a.ff.mod, a.ff.num_hash, a.pf.kmul}; else return a.pf; }();

    // the last k-mer's bases in walking order, four a byte (lane l packs bases 4 l .. 4 l + 3); one outside ACGTU ends the sequence
    {
        uint32_t byte = 0;
        bool bad = false;
        for (int j = 0; j < 4; ++j) {
            const int q = 4 * (int)lane + j;
            if (q < k) {
                const uint32_t p = (uint32_t)(a.direction ? k - 1 - q : nt - 1 + q);
                bad = bad || !tx.usable(p);
                byte |= tx.seed_code(p) << (2 * j);
            }
        }
        if (4 * (int)lane < k) seed[lane] = (uint8_t)byte;
        if (__ballot(bad)) {
            if (lane == 0) ex_put<PE>(a, r, RB_EXT_NONE, RB_EXT_WHY_INVALID_SEED, 0, 0, 0, 0, -1, -1, 0.0f, d - 2);
            return;
        }
    }
    wave_fence();
    // PE: the repeat scan, used below only where there are two or more candidates.  It runs here, for every sequence, because nothing of the
    // walks is held in registers yet (behind the candidates' probes it costs the kernel a dozen registers); one round of a lane per k-mer as a rule
    int rep = 0;
    if constexpr (PE) rep = ex_trailing_repeats(a, tx, nt, d - 2, lane);
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
        if (lane == 0) ex_put<PE>(a, r, RB_EXT_NONE, RB_EXT_WHY_NO_CANDIDATE, 0, 0, 0, 0, -1, -1, 0.0f, d - 2);
        return;
    }

    // the walks' bound (:6026, :6215); PE with two or more candidates: less the trailing repeat k-mers, not below 0 (ex_trailing_repeats)
    int M = d - 2;
    if constexpr (PE) {
        if (n_cand > 1) {
            if (rep < 0) {
                if (lane == 0) ex_put<PE>(a, r, RB_EXT_NONE, RB_EXT_WHY_REPEAT_THROWS, n_cand, 0, 0, 0, -1, -1, 0.0f, d - 2);
                return;
            }
            M -= rep;
        }
    }

    // first level: candidate c's walk is held by lanes 4 c .. 4 c + 3 and fills first-level row c, bound M
    const uint32_t c1 = (lane >> 2) & 3u;
    ExWalk w1;
    w1.A = wave_shfl64(nA, (int)c1); w1.B = wave_shfl64(nB, (int)c1);
    const uint32_t code1 = (uint32_t)__shfl((int)code, (int)c1, 64);
    w1.alive = lane < 16u && ((mask0 >> c1) & 1u);
    w1.start_f = dr.fwd(w1.A, w1.B);
    w1.len = 1; w1.added = 0; w1.bound = M; w1.cap = D; w1.off = 0;
    uint8_t *crow1 = l1c + c1 * D, *brow1 = l1b + c1 * S1;
    if (w1.alive && in == 0u) { crow1[0] = (uint8_t)code1; ex_put2(brow1, 0, c1); }
    wave_fence();
    const ExChain ch1{seed, brow1, brow1, k, EX_NO_GAP};
    ex_run_walks(a.fv, dr, min_cov, ch1, crow1, brow1, w1, lane);
    int len1[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) len1[c] = __shfl(w1.len, 4 * c, 64);

    if (n_cand == 1) {                                        // :6030-6035, :6219-6224: the only candidate and its walk, unscored and untrimmed
        const int c = __builtin_ctz(mask0), n = len1[c];
        ex_emit(a, r, ExChain{seed, l1b + c * S1, l1b + c * S1, k, EX_NO_GAP}, ExCodes{l1c + c * D, l1c + c * D, EX_NO_GAP, n}, n, lane);
        if (lane == 0) ex_put<PE>(a, r, RB_EXT_SINGLE, RB_EXT_WHY_FOUND, 1, n, 0, 0, -1, c, 0.0f, M);
        return;
    }

    // pathMinCov: the minimum count of the last min(n, d) k-mers (:6037, :6235) — all the device holds for SE, the list's last d slots for PE
    float path_min = INFINITY;
    if constexpr (PE) {
        for (int j = max(nt - d, 0) + (int)lane; j < nt; j += 64) path_min = fminf(path_min, a.cnt[k0 + tl.at(j)]);
    } else {
        for (int p = (int)lane; p < nt; p += 64) path_min = fminf(path_min, a.cnt[k0 + p]);
    }
    for (int s = 32; s > 0; s >>= 1) path_min = fminf(path_min, __shfl_xor(path_min, s, 64));

    // the first stretches' pairs (:6047); an unsupported stretch shorter than d - 1 goes one branch further (:6067-6076).  PE (:6249, :6268):
    // a stretch without support of BOTH kinds goes further unless it is d_r - 1 long without a read pair or d - 1 long without a fragment pair
    int pairs1[4], fpairs1[4], last1[4];
    uint32_t l2mask = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        pairs1[c] = 0; fpairs1[c] = 0; last1[c] = -1;
        if ((mask0 >> c) & 1u) {
            const ExPairs cp = ex_count_pairs<PE>(a.pf, ff, d_r, dr, ExChain{seed, l1b + c * S1, l1b + c * S1, k, EX_NO_GAP}, tl, d, len1[c], 0, lane);
            pairs1[c] = cp.pairs; fpairs1[c] = cp.fpairs; last1[c] = cp.last;
            if constexpr (PE) {
                if (!(cp.pairs > 0 && cp.fpairs > 0) && !((len1[c] >= d_r - 1 && cp.pairs == 0) || (len1[c] >= d - 1 && cp.fpairs == 0))) l2mask |= 1u << c;
            } else if (cp.pairs == 0 && len1[c] < d - 1) l2mask |= 1u << c;
        }
    }

    // second level: the successors (count >= 1) of a first stretch's last k-mer — lane 4 c + c2 of the first-level lanes finds candidate
    // (c, c2), which is second-level walk 4 c + c2, held by lanes 16 c + 4 c2 .. + 3, bound d - gap (:6079; PE: M - gap, :6278)
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
        w2.A = wave_shfl64(nA, (int)wid); w2.B = wave_shfl64(nB, (int)wid);
        const uint32_t code2 = (uint32_t)__shfl((int)code, (int)wid, 64);
        w2.alive = (mask2 >> wid) & 1u;
        w2.start_f = dr.fwd(w2.A, w2.B);
        w2.len = 1; w2.added = 0; w2.bound = (PE ? M : d) - gap; w2.cap = C2; w2.off = gap;
        if (w2.alive && in == 0u) { crow2[0] = (uint8_t)code2; ex_put2(brow2, 0, wid & 3u); }
        wave_fence();
        ex_run_walks(a.fv, dr, min_cov, ch2, crow2, brow2, w2, lane);
    }

    // scores in the reference's order: candidate c's first stretch where it is supported, else its second-level extensions (:6051-6105).  A
    // PE chain's counts are the first stretch's plus those of the k-mers behind it (ex_count_pairs), its score counts pairs of both kinds
    float best = 0.0f, best_cov = 0.0f;
    int b_level = 0, b_win = -1, b_len = 0, b_pairs = 0, b_fpairs = 0, b_last = -1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (!((mask0 >> c) & 1u)) continue;
        if (pairs1[c] > 0 && (!PE || fpairs1[c] > 0)) {
            const float cov = ex_median(ExCodes{l1c + c * D, l1c + c * D, EX_NO_GAP, len1[c]}, lane);
            const float score = fminf(path_min, cov) * (float)(PE ? pairs1[c] + fpairs1[c] : pairs1[c]) / (float)(last1[c] + 1);
            if (score > best || (score == best && cov > best_cov)) {
                best = score; best_cov = cov; b_level = 1; b_win = c; b_len = last1[c] + 1; b_pairs = pairs1[c]; b_fpairs = fpairs1[c]; b_last = last1[c];
            }
        } else if ((l2mask >> c) & 1u) {
            for (int c2 = 0; c2 < 4; ++c2) {
                const int w = 4 * c + c2;
                if (!((mask2 >> w) & 1u)) continue;
                const int n = len1[c] + __shfl(w2.len, 4 * w, 64);
                ExPairs cp = ex_count_pairs<PE>(a.pf, ff, d_r, dr, ExChain{seed, l1b + c * S1, l2b + w * S2, k, len1[c]}, tl, d, n, len1[c], lane);
                if constexpr (PE) {
                    cp.pairs += pairs1[c]; cp.fpairs += fpairs1[c]; cp.last = max(cp.last, last1[c]);
                    if (cp.pairs == 0 || cp.fpairs == 0) continue;
                } else if (cp.pairs == 0) continue;
                const float cov = ex_median(ExCodes{l1c + c * D, l2c + w * C2, len1[c], n}, lane);
                const float score = fminf(path_min, cov) * (float)(PE ? cp.pairs + cp.fpairs : cp.pairs) / (float)(cp.last + 1);
                if (score > best || (score == best && cov > best_cov)) {
                    best = score; best_cov = cov; b_level = 2; b_win = c | (c2 << 4); b_len = cp.last + 1; b_pairs = cp.pairs; b_fpairs = cp.fpairs; b_last = cp.last;
                }
            }
        }
    }
    if (b_level == 0) {
        if (lane == 0) ex_put<PE>(a, r, RB_EXT_NONE, RB_EXT_WHY_NO_SUPPORT, n_cand, 0, 0, 0, -1, -1, 0.0f, M);
        return;
    }
    // the winner, trimmed to its last supported k-mer (:6060-6064)
    const int c = b_win & 3, w = 4 * c + (b_win >> 4);
    if (b_level == 1) ex_emit(a, r, ExChain{seed, l1b + c * S1, l1b + c * S1, k, EX_NO_GAP}, ExCodes{l1c + c * D, l1c + c * D, EX_NO_GAP, b_len}, b_len, lane);
    else ex_emit(a, r, ExChain{seed, l1b + c * S1, l2b + w * S2, k, len1[c]}, ExCodes{l1c + c * D, l2c + w * C2, len1[c], b_len}, b_len, lane);
    if (lane == 0) ex_put<PE>(a, r, b_level == 1 ? RB_EXT_FIRST : RB_EXT_SECOND, RB_EXT_WHY_FOUND, n_cand, b_len, b_pairs, b_fpairs, b_last, b_win, best, M);
}
template <bool PE>
__device__ void ex_one(const ExArgsT<PE> &a, int64_t r, uint8_t *row, uint32_t lane) {
    ex_one_on<PE>(a, r, row, lane, ExBatchText{a.codes, a.valid, a.woff + r});
}

}  // namespace
}  // namespace rb
