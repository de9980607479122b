// rb_correct.hip — error correction of host sequences (rb_graph_correct_errors): GraphUtils.correctErrorHelper (R/util/GraphUtils.java:3711-3912),
// what correctErrorsSE (:3998-4049) and correctErrorsPE (:4051-4182) run on every read that passes the coverage screen.  The helper finds each
// run of k-mers whose count is below the threshold (a "gap") and repairs it — an SNV bubble is refilled (:3782-3818), an interior gap bridged by a
// maximum-coverage path (:3819-3845), an edge tip replaced by a greedy extension or trimmed (:3736-3781, :3857-3902) — and then runs correctMismatches
// (:3904) on the repaired list.
//   Gaps are independent: after every gap the helper appends the good k-mer behind it (:3850), so the left anchor kmers2.get(size - 1) of the next gap
// (:3820) is always an ORIGINAL k-mer, and kmers2.isEmpty() (:3736) is true exactly for a gap that starts at k-mer 0.  Every gap of every sequence of
// a piece is therefore resolved at once.  kmers2 is a chain of k-mers that overlap by k - 1 bases (the SNV branch's k + 2 k-mers for k included), so
// it is the string it spells, and correctMismatches on it is the mismatch unit's kernels on that string.
//   Per piece (rb_pieces.hpp): getKmers rows (rb_query.hip) -> k_gap_scan counts, then emits, one record a gap -> the walks of the edge and path
// gaps, a bound each, by the kernels of rb_graph_greedy_extend / rb_graph_walk -> k_resolve_* decide every gap and write its replacement bases ->
// k_stitch writes each sequence's new text -> k_text_kmers hashes and counts it -> the two scans of rb_mismatch.hip.  (DESIGN.md §5 "Error correction".)
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rb_pieces.hpp"
#include "rb_correct.hpp"
#include "rb_lookup.hpp"
#include "rb_align.hpp"
#include "rb_wave.hpp"

using namespace rb;

// Java float arithmetic: medians and the percent identity are single float32 operations
#pragma clang fp contract(off)

namespace {

constexpr int CE_TPB = 256;
constexpr int CE_WAVES = CE_TPB / 64;         // sequences / gaps per workgroup: a wavefront each
constexpr size_t WALK_CHUNK_BYTES = (size_t)256 << 20;      // device scratch of the walks that run together

static_assert(sizeof(rb_corr_gap) == 20, "rb_corr_gap is 20 bytes");

__device__ __forceinline__ bool ce_contains(const FilterView &fv, uint64_t h0) { return bits_lookup(fv.dbg, fv.dbg_mod, fv.dbg_h, fv.kmul, h0); }
// Kmer.getLeftVariants / getRightVariants(k, numHash, graph, minKmerCov) (R/graph/Kmer.java:361-405, CanonicalKmer.java:387-) of the k-mer with
// getKmers hashes (f, r): is any alternative of the base ch (side 2: the first base, 3: the last) a k-mer with count >= min_cov?  The hashes are
// rb_graph_neighbors' (direction 2 / 3); lanes 0..3 take a substitution each.
__device__ __forceinline__ bool ce_has_variants(const FilterView &fv, int stranded, uint32_t uk, int side, uint64_t f, uint64_t r, uint32_t ch,
                                                float min_cov, uint32_t lane) {
    const uint32_t a = lane & 3u, oc = letter_code(ch);
    const uint64_t s_out = oc < 4u ? seed_of(oc) : 0ull, sc_out = oc < 4u ? seed_of(3u - oc) : 0ull;
    uint64_t nf, nr;
    if (side == 2) { nf = f ^ rotl_var(s_out, uk - 1u) ^ rotl_var(seed_of(a), uk - 1u); nr = r ^ sc_out ^ seed_of(3u - a); }
    else { nf = f ^ s_out ^ seed_of(a); nr = r ^ rotl_var(sc_out, uk - 1u) ^ rotl_var(seed_of(3u - a), uk - 1u); }
    bool ok = false;
    if (lane < 4u && ((alt_mask(ch) >> a) & 1u)) ok = graph_count(fv, stranded ? nf : smin(nf, nr)) >= min_cov;
    return __ballot(ok) != 0ull;
}
// Kmer.hasSuccessors (direction 0, ch = the first base) / hasPredecessors (1, ch = the last base) (R/graph/Kmer.java:97-125): graph.contains of
// any of the four neighbours, hashed as rb_graph_neighbors hashes them
__device__ __forceinline__ bool ce_has_neighbors(const FilterView &fv, int stranded, uint32_t uk, int direction, uint64_t f, uint64_t r, uint32_t ch,
                                                 uint32_t lane) {
    const uint32_t a = lane & 3u, oc = letter_code(ch);
    const uint64_t s_out = oc < 4u ? seed_of(oc) : 0ull, sc_out = oc < 4u ? seed_of(3u - oc) : 0ull;
    uint64_t nf, nr;
    if (direction == 0) { nf = rotl1(f) ^ rotl_var(s_out, uk) ^ seed_of(a); nr = rotr1(r) ^ rotr1(sc_out) ^ rotl_var(seed_of(3u - a), uk - 1u); }
    else { nf = rotr1(f) ^ rotr1(s_out) ^ rotl_var(seed_of(a), uk - 1u); nr = rotl1(r) ^ rotl_var(sc_out, uk) ^ seed_of(3u - a); }
    bool ok = false;
    if (lane < 4u) ok = ce_contains(fv, stranded ? nf : smin(nf, nr));
    return __ballot(ok) != 0ull;
}

// Common.getMedian (R/util/Common.java:41-50) of the n counts get(0 .. n-1), by the whole wavefront
template <class GET> __device__ __forceinline__ float ce_median(GET get, int n, uint32_t lane) {
    return median_code([&](int p) { return count_code_of(get(p)); }, n, lane);
}

// ---- gap scan (:3730-3855, :3857): a wavefront per sequence ballots 64 counts at a time; a run of counts below T that ends at a good k-mer is a gap,
// a run still open at the end is the right edge if it is not the whole list.  EMIT false: the number of gaps per sequence; true: the records, at
// gof[r] (the host's prefix sums of those numbers).
template <bool EMIT>
__global__ void __launch_bounds__(CE_TPB) k_gap_scan(int k, int64_t pn, const int64_t *__restrict__ kof, const float *__restrict__ cnt,
                                                     const float *__restrict__ thr, const int64_t *__restrict__ gof, int32_t *__restrict__ ngap,
                                                     rb_corr_gap *__restrict__ recs) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t r = (int64_t)blockIdx.x * CE_WAVES + wv;
    if (r >= pn) return;
    const int64_t k0 = kof[r];
    const int32_t nk = (int32_t)(kof[r + 1] - k0);
    const float T = thr[r];
    int ng = 0;
    if (nk > 0 && T > 0.0f) {                                   // T <= 0: no count is below it
        const float *c_ = cnt + k0;
        rb_corr_gap *out = EMIT ? recs + gof[r] : nullptr;
        auto emit = [&](int32_t first, int32_t nb) {
            if (EMIT && lane == 0) {
                rb_corr_gap g;
                g.seq = (int32_t)r; g.first = first; g.run = nb; g.repl_len = nb;
                g.kind = (uint8_t)(first == 0 ? RB_GAP_LEFT_EDGE : first + nb == nk ? RB_GAP_RIGHT_EDGE : nb == k ? RB_GAP_SNV : RB_GAP_PATH);
                g.outcome = RB_GAP_KEPT; g.pad[0] = g.pad[1] = 0;
                out[ng] = g;
            }
            ++ng;
        };
        int32_t run_start = -1;
        for (int32_t base = 0; base < nk; base += 64) {
            const int32_t p = base + (int32_t)lane;
            const unsigned long long m = __ballot(p < nk && c_[p] < T);
            const int32_t nv = min(64, nk - base);
            const unsigned long long vmask = nv == 64 ? ~0ull : ((1ull << nv) - 1ull);
            const unsigned long long good = ~m & vmask;
            int32_t pos = 0;
            while (pos < nv) {
                if (run_start < 0) {
                    const unsigned long long mm = m >> pos;
                    if (!mm) break;
                    pos += (int32_t)__builtin_ctzll(mm);
                    run_start = base + pos;
                } else {
                    const unsigned long long gg = good >> pos;
                    if (!gg) break;
                    pos += (int32_t)__builtin_ctzll(gg);
                    emit(run_start, base + pos - run_start);
                    run_start = -1;
                }
            }
        }
        if (run_start > 0) emit(run_start, nk - run_start);     // numBadKmersSince < numKmers (:3857): a list that is bad throughout stays
    }
    if (!EMIT && lane == 0) ngap[r] = ng;
}

// seeds, targets and bounds of the walks of a list of gaps.  mode 0: greedyExtendLeft from the good k-mer behind a left tip (:3753), 1:
// greedyExtendRight from the good k-mer before a right tip (:3874), both bounded by the run; 2: getMaxCoveragePath's walk to the right from the good
// k-mer before the gap towards the one behind it (:3820), bound run + max_indel; 3: the bounds of its walk back — 0 where the first walk arrived
__global__ void k_walk_setup(int k, int mode, int max_indel, const int32_t *__restrict__ list, int64_t n, const rb_corr_gap *__restrict__ recs,
                             const int64_t *__restrict__ tof, const uint8_t *__restrict__ txt, const uint8_t *__restrict__ reason1,
                             uint8_t *__restrict__ seeds, uint8_t *__restrict__ targets, int32_t *__restrict__ bounds) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    const rb_corr_gap g = recs[list[w]];
    if (mode == 3) { bounds[w] = reason1[w] == 1 ? 0 : g.run + max_indel; return; }
    const uint8_t *tx = txt + tof[g.seq];
    const int32_t src = mode == 0 ? g.first + g.run : g.first - 1;
    for (int q = 0; q < k; ++q) seeds[w * k + q] = tx[src + q];
    if (mode == 2) for (int q = 0; q < k; ++q) targets[w * k + q] = tx[g.first + g.run + q];
    bounds[w] = mode == 2 ? g.run + max_indel : g.run;
}

struct CorrView {                       // the piece's arrays as the resolve kernels see them
    const int64_t *kof, *tof;           // k-mer / text offsets of the piece's sequences
    const uint8_t *txt;
    const uint64_t *F, *R;              // getKmers rows
    const float *cnt;
    rb_corr_gap *recs;
    const int64_t *rof;                 // replacement pool offsets per gap
    uint8_t *pool;
    const int64_t *lof;                 // Levenshtein row in device scratch per gap (ints), -1: the row fits LDS
    int *lev;
};

// ---- edge gaps (:3736-3781 left, :3857-3902 right): a wavefront per gap.  walk: the greedy extension of gap list[w] is walk w (out_b / out_c rows of
// `bound`), or nullptr for the tips shorter than lookahead, which are dropped as soon as the k-mer next to the good one has a variant.
__global__ void __launch_bounds__(CE_TPB) k_resolve_edge(FilterView fv, int stranded, int k, CorrView v, const int32_t *__restrict__ list, int64_t n,
                                                         int lookahead, float percent_identity, float min_cov, int bound,
                                                         const uint8_t *__restrict__ out_b, const float *__restrict__ out_c,
                                                         const int32_t *__restrict__ out_len) {
    __shared__ int s_row[CE_WAVES][LEV_LDS];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u, uk = (uint32_t)k;
    const int64_t w = (int64_t)blockIdx.x * CE_WAVES + wv;
    if (w >= n) return;
    const int32_t gi = list[w];
    const rb_corr_gap g = v.recs[gi];
    const bool left = g.kind == RB_GAP_LEFT_EDGE;
    const int32_t nb = g.run, first = g.first;
    const int64_t k0 = v.kof[g.seq];
    const int32_t nk = (int32_t)(v.kof[g.seq + 1] - k0);
    const uint8_t *tx = v.txt + v.tof[g.seq];
    // the bad k-mer next to the good one: the last of a left tip, the first of a right tip; its far base is the one the variants replace
    const int32_t j = left ? nb - 1 : first;
    const uint32_t ch = left ? tx[j] : tx[j + k - 1];
    uint8_t outcome = RB_GAP_KEPT;
    if (ce_has_variants(fv, stranded, uk, left ? 2 : 3, v.F[k0 + j], stranded ? 0ull : v.R[k0 + j], ch, min_cov, lane)) {
        if (nb < lookahead) outcome = RB_GAP_TRIMMED;
        else if (out_b) {
            const float *tc = v.cnt + k0 + first;
            const float tip_med = ce_median([&](int p) { return tc[p]; }, nb, lane);
            const float *ec = out_c + w * (int64_t)bound;
            const uint8_t *eb = out_b + w * (int64_t)bound;
            if (out_len[w] == nb && ce_median([&](int p) { return ec[p]; }, nb, lane) > tip_med) {
                // assemble(extension) against assemble(tip): both nb + k - 1 letters
                const int len = nb + k - 1;
                const int64_t lo = v.lof[gi];
                int *row = lo >= 0 ? v.lev + lo : s_row[wv];
                const uint8_t *t0 = tx + (left ? 0 : first);
                int d;
                if (left) d = ce_distance([&](int x) -> uint32_t { return x < nb ? eb[nb - 1 - x] : ce_norm(tx[x]); }, len,
                                          [&](int x) -> uint32_t { return t0[x]; }, len, row, lane);
                else d = ce_distance([&](int x) -> uint32_t { return x < k - 1 ? ce_norm(tx[first + x]) : eb[x - (k - 1)]; }, len,
                                     [&](int x) -> uint32_t { return t0[x]; }, len, row, lane);
                if (ce_identity(d, len, len) >= percent_identity) {
                    outcome = RB_GAP_REPLACED;
                    uint8_t *rp = v.pool + v.rof[gi];
                    for (int x = (int)lane; x < nb; x += 64) rp[x] = left ? eb[nb - 1 - x] : eb[x];
                } else {
                    const int32_t e = left ? 0 : nk - 1;            // the k-mer at the sequence's end: a blunt end in the graph?
                    const bool has = ce_has_neighbors(fv, stranded, uk, left ? 1 : 0, v.F[k0 + e], stranded ? 0ull : v.R[k0 + e],
                                                      left ? tx[e + k - 1] : tx[e], lane);
                    if (!has && nb < k) outcome = RB_GAP_TRIMMED;
                }
            }
        }
    }
    if (lane == 0) { v.recs[gi].outcome = outcome; v.recs[gi].repl_len = outcome == RB_GAP_TRIMMED ? 0 : nb; }
}

// ---- SNV bubbles (:3782-3818): a wavefront per gap of exactly k k-mers.  The candidates are the k + 2 windows of left + n + right, 2k + 1 letters:
// left = the first bad k-mer, right = the last one (the base they share stands twice).  Lane w hashes window w once without n (ntHash is XOR-linear,
// so n's seed is added afterwards), probes the four candidates together (count_lookup4) and parks the counts in LDS; minimum and median per candidate
// are wavefront reductions.  bestCov starts at Float.MIN_VALUE: medians are multiples of 0.5, so `median > bestCov` is `median > 0` at first.
__global__ void __launch_bounds__(CE_TPB) k_resolve_snv(FilterView fv, int stranded, int k, CorrView v, const int32_t *__restrict__ list, int64_t n,
                                                        float min_cov) {
    __shared__ float s_c[CE_WAVES][4][RB_MAX_K + 2];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t w = (int64_t)blockIdx.x * CE_WAVES + wv;
    if (w >= n) return;
    const int32_t gi = list[w];
    const rb_corr_gap g = v.recs[gi];
    const uint8_t *tx = v.txt + v.tof[g.seq] + g.first;             // left = tx[0 .. k), right = tx[k-1 .. 2k-1)
    auto S = [&](int x) -> uint32_t { return x < k ? tx[x] : tx[x - 2]; };      // the 2k + 1 letters, x != k
    const int nw = k + 2;
    for (int win = (int)lane; win < nw; win += 64) {
        uint64_t f = 0, r = 0;
        bool ok = true;
        for (int q = 0; q < k; ++q) {
            const int xf = win + q, xr = win + k - 1 - q;
            uint32_t cf = 4u, cr = 4u;
            if (xf != k) { cf = letter_code(S(xf)); ok = ok && cf < 4u; }
            if (xr != k) cr = letter_code(S(xr));
            f = rotl1(f) ^ (cf < 4u ? seed_of(cf) : 0ull);
            r = rotl1(r) ^ (cr < 4u ? seed_of(3u - cr) : 0ull);     // Horner from the last base: r = XOR rotl(seed(comp(b_q)), q)
        }
        const bool has_n = win >= 1 && win <= k;                    // n is letter q = k - win of the window
        uint64_t h[4];
        float c[4];
#pragma unroll
        for (uint32_t a = 0; a < 4u; ++a) {
            const uint64_t nf = has_n ? f ^ rotl_var(seed_of(a), (uint32_t)(win - 1)) : f;
            const uint64_t nr = has_n ? r ^ rotl_var(seed_of(3u - a), (uint32_t)(k - win)) : r;
            h[a] = stranded ? nf : canonical(nf, nr);
        }
        count_lookup4(fv, h, [&](uint32_t a, bool in, uint32_t mn) { c[a] = in ? minifloat_to_float(mn) + 1.0f : 0.0f; });
#pragma unroll
        for (int a = 0; a < 4; ++a) s_c[wv][a][win] = ok ? c[a] : 0.0f;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    float best = 0.0f;
    int besta = -1;
    for (int a = 0; a < 4; ++a) {
        const float *ca = s_c[wv][a];
        bool low = false;
        for (int win = (int)lane; win < nw; win += 64) low = low || ca[win] < min_cov;
        if (__ballot(low)) continue;                                // m3[0] >= minKmerCov
        const float med = ce_median([&](int p) { return ca[p]; }, nw, lane);
        if (med > best) { best = med; besta = a; }
    }
    if (besta >= 0 && best >= min_cov) {
        uint8_t *rp = v.pool + v.rof[gi];                           // the last letters of the k + 2 k-mers
        for (int x = (int)lane; x < nw; x += 64) rp[x] = x == 1 ? code_letter((uint32_t)besta) : x == 0 ? tx[k - 1] : tx[k - 1 + (x - 2)];
        if (lane == 0) { v.recs[gi].outcome = RB_GAP_REPLACED; v.recs[gi].repl_len = nw; }
    }
}

// ---- path gaps (:3819-3845): a wavefront per gap joins the two walks as getMaxCoveragePath does (:1591-1675).  Walk w of the L arrays went right from
// the good k-mer before gap list[w], walk w of the R arrays back from the good k-mer behind it (bound 0 where the first arrived).  k-mer j of a walk is
// seq[j+1 .. j+k] in walk orientation (a left walk's letters run right to left).  The path is the left walk if it arrived; else the right walk's
// first k-mer that the left walk appended decides: low complexity -> none, else the left walk up to that k-mer and the right walk from it; else the
// right walk if it arrived; else none.  Accepted by length and — longer than k + max_indel — by percent identity against the gap's own letters.
__global__ void __launch_bounds__(CE_TPB) k_resolve_path(int k, CorrView v, const int32_t *__restrict__ list, int64_t n, int max_indel,
                                                         float percent_identity, int bound, const uint8_t *__restrict__ seqL,
                                                         const uint64_t *__restrict__ fL, const int32_t *__restrict__ lenL,
                                                         const uint8_t *__restrict__ reasonL, const uint8_t *__restrict__ seqR,
                                                         const uint64_t *__restrict__ fR, const int32_t *__restrict__ lenR,
                                                         const uint8_t *__restrict__ reasonR) {
    __shared__ int s_row[CE_WAVES][LEV_LDS];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t w = (int64_t)blockIdx.x * CE_WAVES + wv;
    if (w >= n) return;
    const int32_t gi = list[w];
    const rb_corr_gap g = v.recs[gi];
    const int32_t nb = g.run, first = g.first;
    const uint8_t *tx = v.txt + v.tof[g.seq];
    const uint8_t *sl = seqL + w * ((int64_t)k + bound), *sr = seqR + w * ((int64_t)k + bound);
    const uint64_t *pl = fL + w * (int64_t)bound, *pr = fR + w * (int64_t)bound;
    const int32_t nl = lenL[w];
    // form 0: none; 1: the left walk (plen = nl); 2: joined at left k-mer idx / right k-mer m; 3: the right walk, m = its last k-mer
    int form = 0, idx = 0, m = 0, plen = 0;
    if (reasonL[w] == 1) { form = 1; plen = nl; }
    else {
        const int32_t nr = lenR[w];
        int hit = -1;
        for (int j = 0; j < nr && hit < 0; ++j) {
            const uint64_t fr = pr[j];
            for (int x0 = 0; x0 < nl && hit < 0; x0 += 64) {
                const int x = x0 + (int)lane;
                unsigned long long mm = __ballot(x < nl && pl[x] == fr);
                while (mm && hit < 0) {                              // Kmer.equals: the hashes, then the letters
                    const int xx = x0 + (int)__builtin_ctzll(mm);
                    mm &= mm - 1ull;
                    bool ne = false;
                    for (int q = (int)lane; q < k; q += 64) ne = ne || letter_code(sl[xx + 1 + q]) != letter_code(sr[j + k - q]);
                    if (!__ballot(ne)) { hit = j; idx = xx; }
                }
            }
        }
        if (hit >= 0) {
            if (!ce_low_complexity([&](int q) -> uint32_t { return sl[idx + 1 + q]; }, k, lane)) { form = 2; m = hit; plen = idx + m + 1; }
        } else if (reasonR[w] == 1) { form = 3; m = nr - 1; plen = nr; }
    }
    bool accept = form != 0 && nb - max_indel <= plen && plen <= nb + max_indel;
    if (accept && plen > k + max_indel) {
        const int slen = plen + k - 1, tlen = nb + k - 1;
        const int64_t lo = v.lof[gi];
        int *row = lo >= 0 ? v.lev + lo : s_row[wv];
        const uint8_t *t0 = tx + first;
        auto t = [&](int x) -> uint32_t { return t0[x]; };
        int d;
        if (form == 1) d = ce_distance([&](int x) -> uint32_t { return ce_norm(sl[1 + x]); }, slen, t, tlen, row, lane);
        else if (form == 2) d = ce_distance([&](int x) -> uint32_t { return ce_norm(x < idx + k ? sl[1 + x] : sr[m - (x - (idx + k))]); }, slen, t, tlen, row, lane);
        else d = ce_distance([&](int x) -> uint32_t { return ce_norm(sr[m + k - x]); }, slen, t, tlen, row, lane);
        accept = ce_identity(d, slen, tlen) >= percent_identity;
    }
    if (accept) {
        uint8_t *rp = v.pool + v.rof[gi];                           // the last letter of each k-mer of the path
        for (int x = (int)lane; x < plen; x += 64)
            rp[x] = ce_norm(form == 1 ? sl[x + k] : form == 2 ? (x <= idx ? sl[x + k] : sr[m + 1 + idx - x]) : sr[m + 1 - x]);
        if (lane == 0) { v.recs[gi].outcome = RB_GAP_REPLACED; v.recs[gi].repl_len = plen; }
    }
}

// ---- stitch: a wavefront per sequence writes the string kmers2 spells.  A left tip stands for letters [0, run); any other gap for the last letters
// of its k-mers, [first + k - 1, first + k - 1 + run); kept gaps are copied, replaced ones come from the pool, trimmed ones are left out.
__global__ void __launch_bounds__(CE_TPB) k_stitch(int k, int64_t pn, const int64_t *__restrict__ tof, const int64_t *__restrict__ ctof,
                                                   const uint8_t *__restrict__ txt, const int64_t *__restrict__ gof, const rb_corr_gap *__restrict__ recs,
                                                   const int64_t *__restrict__ rof, const uint8_t *__restrict__ pool, uint8_t *__restrict__ ctxt,
                                                   int32_t *__restrict__ clen, int32_t *__restrict__ cnk, uint32_t *__restrict__ flags,
                                                   uint32_t *__restrict__ over) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t r = (int64_t)blockIdx.x * CE_WAVES + wv;
    if (r >= pn) return;
    const uint8_t *tx = txt + tof[r];
    const int64_t L = tof[r + 1] - tof[r], cap = ctof[r + 1] - ctof[r];
    uint8_t *out = ctxt + ctof[r];
    int64_t cur = 0, o = 0;
    bool changed = false;
    auto copy = [&](const uint8_t *src, int64_t cnt) {
        for (int64_t x = lane; x < cnt; x += 64) if (o + x < cap) out[o + x] = src[x];
        o += cnt;
    };
    for (int64_t gi = gof[r]; gi < gof[r + 1]; ++gi) {
        const rb_corr_gap g = recs[gi];
        const int64_t a = g.kind == RB_GAP_LEFT_EDGE ? 0 : (int64_t)g.first + k - 1, b = a + g.run;
        copy(tx + cur, a - cur);
        if (g.outcome == RB_GAP_KEPT) copy(tx + a, g.run);
        else { changed = true; if (g.outcome == RB_GAP_REPLACED) copy(pool + rof[gi], g.repl_len); }
        cur = b;
    }
    copy(tx + cur, L - cur);
    if (lane == 0) {
        if (o > cap) { atomicAdd(over, 1u); o = cap; }
        clen[r] = (int32_t)o;
        cnk[r] = o >= k ? (int32_t)(o - k + 1) : 0;
        flags[r] = changed ? RB_CORR_GAP : 0u;
    }
}

// ---- getKmers of the stitched text: hashes, counts and the usable-letter bits of every sequence, rows at the capacity offsets.  A wavefront per
// sequence, a lane per 32 windows (hashes rolled as k_get_kmers rolls them) and per word of the bit row.
__global__ void __launch_bounds__(CE_TPB) k_text_kmers(FilterView fv, int stranded, int k, int64_t pn, const int64_t *__restrict__ ctof,
                                                       const int64_t *__restrict__ ckof, const uint32_t *__restrict__ cwoff,
                                                       const uint8_t *__restrict__ ctxt, const int32_t *__restrict__ clen, uint32_t *__restrict__ valid,
                                                       uint64_t *__restrict__ F, uint64_t *__restrict__ R, float *__restrict__ cnt) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u, uk = (uint32_t)k;
    const int64_t r = (int64_t)blockIdx.x * CE_WAVES + wv;
    if (r >= pn) return;
    const uint8_t *tx = ctxt + ctof[r];
    const int32_t L = clen[r], nk = L >= k ? L - k + 1 : 0;
    uint32_t *vw = valid + cwoff[r];
    for (int32_t wd = (int32_t)lane; wd * 32 < L; wd += 64) {
        uint32_t bits = 0;
        for (int32_t b = 0; b < 32 && wd * 32 + b < L; ++b) bits |= (letter_code(tx[wd * 32 + b]) < 4u ? 1u : 0u) << b;
        vw[wd] = bits;
    }
    uint64_t *f_ = F + ckof[r], *r_ = R + ckof[r];
    float *c_ = cnt + ckof[r];
    for (int32_t p0 = (int32_t)lane * 32; p0 < nk; p0 += 64 * 32) {
        uint64_t f = 0, rv = 0;
        int32_t run = 0;
        for (int32_t q = 0; q < k; ++q) {
            const uint64_t s = letter_seed(tx[p0 + q]), sc = letter_rev_seed(tx[p0 + k - 1 - q]);
            run = s ? run + 1 : 0;
            f = rotl1(f) ^ s;
            rv = rotl1(rv) ^ sc;                                    // Horner from the window's last base
        }
        const int32_t pe = min(nk, p0 + 32);
        for (int32_t p = p0; p < pe; ++p) {
            if (p > p0) {
                const uint64_t s_out = letter_seed(tx[p - 1]), sc_out = letter_rev_seed(tx[p - 1]);
                const uint64_t s_in = letter_seed(tx[p + k - 1]), sc_in = letter_rev_seed(tx[p + k - 1]);
                run = s_in ? run + 1 : 0;
                f = rotl1(f) ^ rotl_var(s_out, uk) ^ s_in;
                rv = rotr1(rv) ^ rotr1(sc_out) ^ rotl_var(sc_in, uk - 1u);
            }
            f_[p] = f;
            r_[p] = stranded ? 0ull : rv;
                        c_[p] = run >= k ? graph_count(fv, stranded ? f : canonical(f, rv)) : 0.0f;
        }
    }
}

// the arrays of a piece in the context's arena; lay() is run once on an empty arena for the size and once on the buffer
struct PieceArrays {
    float *cnt, *thr, *cnt2;            // getKmers counts of the input [pt], thresholds [pn], counts of the stitched text [cpt]
    int32_t *ngap, *clen, *cnk, *nf;    // per sequence: gaps, stitched length, its k-mers, replacements of the mismatch pass
    uint8_t *txt, *ctxt, *row;          // input text, stitched text (capacity layout), code rows of the long sequences [cpt]
    uint32_t *flags, *valid, *over;     // RB_CORR_GAP per sequence, usable-letter bits of the stitched text, sequences that outgrew their slot
    void lay(Arena &a, int64_t pt, int64_t pn, int64_t tb, int64_t ctb, int64_t cpt, bool any_long, size_t valid_words) {
        cnt = a.take<float>((size_t)pt); thr = a.take<float>((size_t)pn); ngap = a.take<int32_t>((size_t)pn);
        txt = a.take<uint8_t>((size_t)tb); ctxt = a.take<uint8_t>((size_t)ctb); clen = a.take<int32_t>((size_t)pn);
        cnk = a.take<int32_t>((size_t)pn); flags = a.take<uint32_t>((size_t)pn); nf = a.take<int32_t>((size_t)pn);
        cnt2 = a.take<float>((size_t)cpt); row = a.take<uint8_t>(any_long ? (size_t)cpt : 0); valid = a.take<uint32_t>(valid_words);
        over = a.take<uint32_t>(4);
    }
};

}  // namespace

void rb::launch_text_kmers(rb_graph *g, int64_t pn, const int64_t *tof, const int64_t *kof, const uint32_t *woff, const uint8_t *txt, const int32_t *len,
                           uint32_t *valid, uint64_t *F, uint64_t *R, float *cnt, hipStream_t s) {
    hipLaunchKernelGGL(k_text_kmers, dim3(blocks_for(pn, CE_WAVES)), dim3(CE_TPB), 0, s, g->view(0, 0), (int)g->stranded, g->k, pn, tof, kof, woff, txt, len,
                       valid, F, R, cnt);
    RB_HIP(hipGetLastError());
}

void rb::CorrBody::prepare(int64_t pn_, const int64_t *kof, const int64_t *tof, const int64_t *ctof) {
    const int k = g->k;
    const int lds_row = rb::mismatch_lds_row();
    pn = pn_;
    pt = kof[pn] - kof[0]; tb = tof[pn] - tof[0]; ctb = ctof[pn] - ctof[0];
    // the piece's table: k-mer offsets, text offsets, capacity text offsets, capacity k-mer offsets [pn + 1 each], the sequences whose
    // capacity has more k-mers than a code row in LDS; then the capacity word offsets of the usable-letter bits
    tab.assign((size_t)(4 * pn + 4), 0);
    cwoff.assign((size_t)pn + 1, 0);
    std::vector<int64_t> longs;
    {
        int64_t *t_kof = tab.data(), *t_tof = t_kof + pn + 1, *t_ctof = t_tof + pn + 1, *t_ckof = t_ctof + pn + 1;
        for (int64_t i = 0; i <= pn; ++i) {
            t_kof[i] = kof[i] - kof[0];
            t_tof[i] = tof[i] - tof[0];
            t_ctof[i] = ctof[i] - ctof[0];
        }
        for (int64_t i = 0; i < pn; ++i) {
            const int64_t cl = t_ctof[i + 1] - t_ctof[i], cnk = cl >= k ? cl - k + 1 : 0;
            t_ckof[i + 1] = t_ckof[i] + cnk;
            cwoff[(size_t)i + 1] = cwoff[(size_t)i] + (uint32_t)((cl + 31) / 32);
            if (cnk > lds_row) longs.push_back(i);
        }
        cpt = t_ckof[pn];
    }
    RB_REQUIRE(cpt < ((int64_t)1 << 40) && (int64_t)cwoff[(size_t)pn] * 32 < ((int64_t)1 << 36), "%s: piece too large", who);
    tab.insert(tab.end(), longs.begin(), longs.end());            // (the pointers above are gone: this may move the table)
    nlong = (int64_t)tab.size() - (4 * pn + 4);
    const size_t tab_bytes = up16(tab.size() * 8);
    c->b0.reserve(tab_bytes + (size_t)(pn + 1) * 4 + 16);
    c->b1.reserve((size_t)cpt * 8 + 16);
    c->b2.reserve((size_t)cpt * 8 + 16);
    PieceArrays pa;
    Arena ar;
    const int64_t in_pt = own_input ? pt : 0, in_tb = own_input ? tb : 0;
    pa.lay(ar, in_pt, pn, in_tb, ctb, cpt, nlong != 0, (size_t)cwoff[(size_t)pn] + 1);
    c->b3.reserve(ar.at + 64);
    ar.base = c->b3.as<uint8_t>(); ar.at = 0;
    pa.lay(ar, in_pt, pn, in_tb, ctb, cpt, nlong != 0, (size_t)cwoff[(size_t)pn] + 1);
    dcnt2 = pa.cnt2; dng = pa.ngap; dclen = pa.clen; dcnk = pa.cnk; dnf = pa.nf;
    dctxt = pa.ctxt; drow = pa.row; dflags = pa.flags; dvalid = pa.valid; dover = pa.over;
    uint8_t *b0 = c->b0.as<uint8_t>();
    dkof = reinterpret_cast<const int64_t *>(b0); dtof = dkof + pn + 1; dctof = dtof + pn + 1; dckof = dctof + pn + 1; dids = dckof + pn + 1;
    dcwoff = reinterpret_cast<const uint32_t *>(b0 + tab_bytes);
    dF = c->b1.as<uint64_t>(); dR = c->b2.as<uint64_t>();
    own_txt = own_input ? pa.txt : nullptr; own_cnt = own_input ? pa.cnt : nullptr; own_thr = own_input ? pa.thr : nullptr;
    if (own_input) { dtxt = own_txt; dcnt = own_cnt; dthr = own_thr; dFin = dF; dRin = dR; }
    RB_HIP(hipMemcpyAsync(b0, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
    RB_HIP(hipMemcpyAsync(b0 + tab_bytes, cwoff.data(), cwoff.size() * 4, hipMemcpyHostToDevice, s));
    RB_HIP(hipMemsetAsync(dctxt, 0, (size_t)ctb, s));
    RB_HIP(hipMemsetAsync(dover, 0, 16, s));
}

void rb::CorrBody::run() {
    const int k = g->k, max_indel = p.max_indel_size, lookahead = p.lookahead;
    const float min_cov = p.min_kmer_cov, pid = p.percent_identity;
    const FilterView fv = g->view(0, 0);
    CorrPhaseTimer &ph = *this->ph;
    DevBuf &gbuf = *this->gbuf, &wbuf = *this->wbuf;
    const uint8_t *dtxt = this->dtxt;
    const float *dcnt = this->dcnt;
    // 1. the number of gaps per sequence
    ph.begin(1);
    hipLaunchKernelGGL((k_gap_scan<false>), dim3(blocks_for(pn, CE_WAVES)), dim3(CE_TPB), 0, s, k, pn, dkof, dcnt, dthr, (const int64_t *)nullptr, dng,
                       (rb_corr_gap *)nullptr);
    RB_HIP(hipGetLastError());
    ph.end();
    ngap.resize((size_t)pn);
    RB_HIP(hipMemcpyAsync(ngap.data(), dng, (size_t)pn * 4, hipMemcpyDeviceToHost, s));
    RB_HIP(hipStreamSynchronize(s));
    gof.assign((size_t)pn + 1, 0);
    for (int64_t i = 0; i < pn; ++i) gof[(size_t)i + 1] = gof[(size_t)i] + ngap[(size_t)i];
    G = gof[(size_t)pn];
    RB_REQUIRE(G < ((int64_t)1 << 31), "%s: piece too large", who);
    // gap-level arrays: gof [pn + 1], records [G], rof [G + 1], lof [G], the lists [G], then the pool and the Levenshtein rows
    int64_t *dlof; int32_t *dlist;
    auto lay_gaps = [&](Arena &x) {
        dgof = x.take<int64_t>((size_t)pn + 1); drecs = x.take<rb_corr_gap>((size_t)G); drof = x.take<int64_t>((size_t)G + 1);
        dlof = x.take<int64_t>((size_t)G); dlist = x.take<int32_t>((size_t)G);
    };
    Arena ga;
    lay_gaps(ga);
    const size_t g_fixed = ga.at;
    gbuf.reserve(g_fixed + 64);
    ga.base = gbuf.as<uint8_t>(); ga.at = 0;
    lay_gaps(ga);
    RB_HIP(hipMemcpyAsync(dgof, gof.data(), gof.size() * 8, hipMemcpyHostToDevice, s));
    uint8_t *dpool = nullptr;
    int *dlev = nullptr;
    if (G > 0) {
        ph.begin(1);
        hipLaunchKernelGGL((k_gap_scan<true>), dim3(blocks_for(pn, CE_WAVES)), dim3(CE_TPB), 0, s, k, pn, dkof, dcnt, dthr, dgof, (int32_t *)nullptr, drecs);
        RB_HIP(hipGetLastError());
        ph.end();
        recs.resize((size_t)G);
        RB_HIP(hipMemcpyAsync(recs.data(), drecs, (size_t)G * sizeof(rb_corr_gap), hipMemcpyDeviceToHost, s));
        RB_HIP(hipStreamSynchronize(s));
        // the lists: [no walk: SNV bubbles | tips shorter than lookahead | left tips | right tips | path gaps]
        rof.assign((size_t)G + 1, 0); lof.assign((size_t)G, -1);
        std::vector<int32_t> l_snv, l_short, l_left, l_right, l_path;
        int64_t lev_ints = 0;
        for (int64_t i = 0; i < G; ++i) {
            const rb_corr_gap &r = recs[(size_t)i];
            int64_t room;
            if (r.kind == RB_GAP_SNV) { l_snv.push_back((int32_t)i); room = k + 2; }
            else if (r.kind == RB_GAP_PATH) { l_path.push_back((int32_t)i); room = (int64_t)r.run + max_indel; }
            else { (r.run < lookahead ? l_short : r.kind == RB_GAP_LEFT_EDGE ? l_left : l_right).push_back((int32_t)i); room = r.run; }
            rof[(size_t)i + 1] = rof[(size_t)i] + room;
            if (r.kind != RB_GAP_SNV && r.run >= lookahead && (int64_t)r.run + k - 1 > LEV_LDS) { lof[(size_t)i] = lev_ints; lev_ints += (int64_t)r.run + k; }
        }
        lists.clear();
        const size_t o_snv = 0, o_short = l_snv.size(), o_left = o_short + l_short.size(), o_right = o_left + l_left.size(),
                     o_path = o_right + l_right.size();
        for (auto *l : {&l_snv, &l_short, &l_left, &l_right, &l_path}) lists.insert(lists.end(), l->begin(), l->end());
        // (growing gbuf would lose what is in it: the pool and the rows get a buffer laid out behind the fixed part, which is uploaded again)
        const size_t o_pool = g_fixed, o_lev = up16(o_pool + (size_t)rof[(size_t)G] + 16), g_all = o_lev + (size_t)lev_ints * 4 + 64;
        gbuf.reserve(g_all);                 // (may move the buffer: everything in it is uploaded again below)
        ga.base = gbuf.as<uint8_t>(); ga.at = 0;
        lay_gaps(ga);
        dpool = gbuf.as<uint8_t>() + o_pool;
        dlev = reinterpret_cast<int *>(gbuf.as<uint8_t>() + o_lev);
        RB_HIP(hipMemcpyAsync(dgof, gof.data(), gof.size() * 8, hipMemcpyHostToDevice, s));
        RB_HIP(hipMemcpyAsync(drecs, recs.data(), (size_t)G * sizeof(rb_corr_gap), hipMemcpyHostToDevice, s));
        RB_HIP(hipMemcpyAsync(drof, rof.data(), rof.size() * 8, hipMemcpyHostToDevice, s));
        RB_HIP(hipMemcpyAsync(dlof, lof.data(), lof.size() * 8, hipMemcpyHostToDevice, s));
        RB_HIP(hipMemcpyAsync(dlist, lists.data(), lists.size() * 4, hipMemcpyHostToDevice, s));
        const CorrView cv{dkof, dtof, dtxt, dFin, dRin, dcnt, drecs, drof, dpool, dlof, dlev};
        // 2. gaps that need no walk
        ph.begin(3);
        if (!l_snv.empty())
            hipLaunchKernelGGL(k_resolve_snv, dim3(blocks_for((int64_t)l_snv.size(), CE_WAVES)), dim3(CE_TPB), 0, s, fv, (int)g->stranded, k, cv,
                               dlist + o_snv, (int64_t)l_snv.size(), min_cov);
        if (!l_short.empty())
            hipLaunchKernelGGL(k_resolve_edge, dim3(blocks_for((int64_t)l_short.size(), CE_WAVES)), dim3(CE_TPB), 0, s, fv, (int)g->stranded, k, cv,
                               dlist + o_short, (int64_t)l_short.size(), lookahead, pid, min_cov, 0, (const uint8_t *)nullptr, (const float *)nullptr,
                               (const int32_t *)nullptr);
        RB_HIP(hipGetLastError());
        ph.end();
        // 3. the walks, as many at a time as WALK_CHUNK_BYTES holds with the uniform row of the longest of them, and their gaps
        auto chunks = [&](const std::vector<int32_t> &l, int64_t extra, auto per_walk, auto run) {
            size_t a = 0;
            while (a < l.size()) {
                size_t e = a;
                int64_t B = 1;
                while (e < l.size()) {
                    const int64_t nb2 = std::max<int64_t>(B, (int64_t)recs[(size_t)l[e]].run + extra);
                    if (e > a && (e - a + 1) * per_walk(nb2) > WALK_CHUNK_BYTES) break;
                    B = nb2; ++e;
                }
                run(a, e - a, (int)B);
                a = e;
            }
        };
        const size_t ks = (size_t)k;
        for (int side = 0; side < 2; ++side) {
            const std::vector<int32_t> &l = side ? l_right : l_left;
            const size_t o_l = side ? o_right : o_left;
            chunks(l, 0, [&](int64_t B) { return ks + rb::greedy_seq_stride(k, (int)B) + (size_t)B * 5 + 64; },
                   [&](size_t a, size_t cn, int B) {
                       Arena wa;
                       auto lay = [&](Arena &x, uint8_t *&seeds, uint8_t *&sq, uint8_t *&ob, float *&oc, int32_t *&ol, uint8_t *&orr, int32_t *&bd) {
                           seeds = x.take<uint8_t>(cn * ks); sq = x.take<uint8_t>(cn * rb::greedy_seq_stride(k, B)); ob = x.take<uint8_t>(cn * (size_t)B);
                           oc = x.take<float>(cn * (size_t)B); ol = x.take<int32_t>(cn); orr = x.take<uint8_t>(cn); bd = x.take<int32_t>(cn);
                       };
                       uint8_t *seeds, *sq, *ob, *orr; float *oc; int32_t *ol, *bd;
                       lay(wa, seeds, sq, ob, oc, ol, orr, bd);
                       wbuf.reserve(wa.at + 64);
                       wa.base = wbuf.as<uint8_t>(); wa.at = 0;
                       lay(wa, seeds, sq, ob, oc, ol, orr, bd);
                       const int32_t *lst = dlist + o_l + a;
                       ph.begin(2);
                       hipLaunchKernelGGL(k_walk_setup, dim3(blocks_for((int64_t)cn)), dim3(TPB), 0, s, k, side ? 1 : 0, max_indel, lst, (int64_t)cn, drecs, dtof,
                                          dtxt, (const uint8_t *)nullptr, seeds, (uint8_t *)nullptr, bd);
                       RB_HIP(hipGetLastError());
                       rb::launch_greedy_extend(g, side ? 0 : 1, seeds, cn, lookahead, B, bd, sq, ob, oc, ol, orr, s);
                       ph.end();
                       ph.begin(3);
                       hipLaunchKernelGGL(k_resolve_edge, dim3(blocks_for((int64_t)cn, CE_WAVES)), dim3(CE_TPB), 0, s, fv, (int)g->stranded, k, cv, lst,
                                          (int64_t)cn, lookahead, pid, min_cov, B, ob, oc, ol);
                       RB_HIP(hipGetLastError());
                       ph.end();
                   });
        }
        chunks(l_path, max_indel, [&](int64_t B) { return 2 * (ks + (ks + (size_t)B) + (size_t)B * 21 + 64); },
               [&](size_t a, size_t cn, int B) {
                   Arena wa;
                   struct W { uint8_t *seeds, *sq, *ob, *orr; uint64_t *of, *orv; float *oc; int32_t *ol, *bd; } L, Rw;
                   auto lay = [&](Arena &x, W &w) {
                       w.seeds = x.take<uint8_t>(cn * ks); w.sq = x.take<uint8_t>(cn * (ks + (size_t)B)); w.ob = x.take<uint8_t>(cn * (size_t)B);
                       w.of = x.take<uint64_t>(cn * (size_t)B); w.orv = x.take<uint64_t>(cn * (size_t)B); w.oc = x.take<float>(cn * (size_t)B);
                       w.ol = x.take<int32_t>(cn); w.orr = x.take<uint8_t>(cn); w.bd = x.take<int32_t>(cn);
                   };
                   lay(wa, L); lay(wa, Rw);
                   wbuf.reserve(wa.at + 64);
                   wa.base = wbuf.as<uint8_t>(); wa.at = 0;
                   lay(wa, L); lay(wa, Rw);
                   const int32_t *lst = dlist + o_path + a;
                   ph.begin(2);
                   // the first walk's seeds are the second's targets and the other way round
                   hipLaunchKernelGGL(k_walk_setup, dim3(blocks_for((int64_t)cn)), dim3(TPB), 0, s, k, 2, max_indel, lst, (int64_t)cn, drecs, dtof, dtxt,
                                      (const uint8_t *)nullptr, L.seeds, Rw.seeds, L.bd);
                   RB_HIP(hipGetLastError());
                   rb::launch_walk_max_cov(g, 0, L.seeds, Rw.seeds, cn, B, L.bd, min_cov, L.sq, L.ob, L.of, L.orv, L.oc, L.ol, L.orr, s);
                   hipLaunchKernelGGL(k_walk_setup, dim3(blocks_for((int64_t)cn)), dim3(TPB), 0, s, k, 3, max_indel, lst, (int64_t)cn, drecs, dtof, dtxt,
                                      (const uint8_t *)L.orr, (uint8_t *)nullptr, (uint8_t *)nullptr, Rw.bd);
                   RB_HIP(hipGetLastError());
                   rb::launch_walk_max_cov(g, 1, Rw.seeds, L.seeds, cn, B, Rw.bd, min_cov, Rw.sq, Rw.ob, Rw.of, Rw.orv, Rw.oc, Rw.ol, Rw.orr, s);
                   ph.end();
                   ph.begin(3);
                   hipLaunchKernelGGL(k_resolve_path, dim3(blocks_for((int64_t)cn, CE_WAVES)), dim3(CE_TPB), 0, s, k, cv, lst, (int64_t)cn, max_indel, pid, B,
                                      L.sq, L.of, L.ol, L.orr, Rw.sq, Rw.of, Rw.ol, Rw.orr);
                   RB_HIP(hipGetLastError());
                   ph.end();
               });
    }
    // 4. the new text, its getKmers rows, the mismatch pass
    ph.begin(4);
    hipLaunchKernelGGL(k_stitch, dim3(blocks_for(pn, CE_WAVES)), dim3(CE_TPB), 0, s, k, pn, dtof, dctof, dtxt, dgof, drecs, drof, dpool, dctxt, dclen, dcnk,
                       dflags, dover);
    RB_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_text_kmers, dim3(blocks_for(pn, CE_WAVES)), dim3(CE_TPB), 0, s, fv, (int)g->stranded, k, pn, dctof, dckof, dcwoff, dctxt, dclen,
                       dvalid, dF, dR, dcnt2);
    RB_HIP(hipGetLastError());
    ph.end();
    ph.begin(5);
    rb::launch_mismatch(g, min_cov, pn, dids, nlong, dckof, dcnk, dctof, dcwoff, dvalid, dctxt, dF, dR, dcnt2, drow, dthr, dnf, write_counts, s);
    ph.end();
}

extern "C" {
int rb_graph_correct_errors(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, const float *cov_threshold, const rb_corr_params *p,
                            int64_t *out_offsets, char *out_seq, int32_t *out_len, uint32_t *flags, rb_corr_gap *gaps, int64_t *gap_offsets) {
    return guarded([&] {
        RB_REQUIRE(g && offsets && cov_threshold && p && out_offsets && n >= 0, "rb_graph_correct_errors: null argument");
        RB_REQUIRE(!out_seq || (out_len && flags), "rb_graph_correct_errors: null argument");
        RB_REQUIRE(!g->shard, "rb_graph_correct_errors: not available on a shard handle");
        RB_REQUIRE(g->dbg.bits && g->cbf, "rb_graph_correct_errors: dbgbf or the counting filter has been destroyed");
        RB_REQUIRE(g->k >= 2, "rb_graph_correct_errors: k = %d (the mismatch pass's median of k - 1 counts needs k >= 2)", g->k);
        RB_REQUIRE(std::isfinite(p->percent_identity) && std::isfinite(p->min_kmer_cov), "rb_graph_correct_errors: percent_identity and min_kmer_cov must be finite");
        RB_REQUIRE(p->lookahead >= 1 && p->lookahead <= 16, "rb_graph_correct_errors: lookahead out of range [1, 16]");
        RB_REQUIRE(p->max_indel_size >= 0 && p->max_indel_size <= CE_MAX_INDEL, "rb_graph_correct_errors: max_indel_size out of range [0, %d]", CE_MAX_INDEL);
        RB_REQUIRE(!gaps || gap_offsets, "rb_graph_correct_errors: gaps needs gap_offsets");
        const int k = g->k, max_indel = p->max_indel_size;
        std::vector<int64_t> ko((size_t)n + 1);
        kmer_offsets(offsets, n, k, ko.data(), "rb_graph_correct_errors");
        for (int64_t i = 0; i < n; ++i)
            RB_REQUIRE(std::isfinite(cov_threshold[i]), "rb_graph_correct_errors: cov_threshold[%lld] is not finite", (long long)i);
        const int64_t text = n ? offsets[n] - offsets[0] : 0;
        RB_REQUIRE(text == 0 || seq, "rb_graph_correct_errors: null sequence text");
        out_offsets[0] = 0;
        for (int64_t i = 0; i < n; ++i) out_offsets[i + 1] = out_offsets[i] + corr_capacity(offsets[i + 1] - offsets[i], k, max_indel);
        if (!out_seq) {                                     // a size query: the capacity layouts
            if (gap_offsets) { gap_offsets[0] = 0; for (int64_t i = 0; i < n; ++i) gap_offsets[i + 1] = gap_offsets[i] + (ko[(size_t)i + 1] - ko[(size_t)i] + 1) / 2; }
            return;
        }
        if (gap_offsets) std::fill(gap_offsets, gap_offsets + n + 1, (int64_t)0);
        if (n == 0) return;
        // what no kernel touches comes back as it went in: sequences without a k-mer in pieces without one
        for (int64_t i = 0; i < n; ++i) {
            const int64_t l = offsets[i + 1] - offsets[i];
            if (l) memmove(out_seq + out_offsets[i], seq + offsets[i], (size_t)l);
            out_len[i] = (int32_t)l;
            flags[i] = 0;
        }
        const int64_t total = ko[(size_t)n];
        if (total == 0) return;
        RB_HIP(hipSetDevice(g->p.device));
        const int64_t ctext = out_offsets[n];
        HostPin pin_seq(seq + offsets[0], (size_t)text), pin_out(out_seq, (size_t)ctext), pin_thr(cov_threshold, (size_t)n * 4);
        QueryLease q(g);
        hipStream_t s = q.c->st;
        CorrPhaseTimer ph;
        ph.on = g->prof_on; ph.s = s;
        // the piece's gap-level arrays; the walks that run together.  Both belong to the call, not to the leased context: a context's four buffers are
        // taken (table, two hash rows, the arena).  A chunk that needs more than wbuf holds makes reserve() free it, and hipFree waits for the device — which
        // is what lets the next chunk overwrite rows that the previous chunk's kernels, still in flight on the stream, read: chunks of equal or smaller
        // size reuse the block in stream order, which is safe for the same stream.  The cost (an allocation a call, a device-wide wait per regrowth) is
        // accepted here: chunks are sized in descending need only by accident, and a call has few of them.
        DevBuf gbuf, wbuf;
        CorrBody body;
        body.g = g; body.c = q.c.get(); body.s = s; body.ph = &ph; body.gbuf = &gbuf; body.wbuf = &wbuf; body.p = *p;
        std::vector<int32_t> nf;
        int64_t gbase = 0;                                  // gap records of the pieces before this one
        int64_t piece_end = 0;
        // a piece's scratch goes by its CAPACITY k-mers (the stitched text's rows: 40 bytes each), up to 1 + max_indel / 2 per input k-mer: the pieces
        // are cut smaller by that factor, so a piece holds about 16 M capacity k-mers (RB_QUERY_PIECE still counts input k-mers)
        const int64_t piece_dflt = std::max<int64_t>(1, ((int64_t)16 << 20) / (1 + (max_indel + 1) / 2));
        for_each_host_piece(g, s, seq, offsets, ko.data(), n, "correct_errors", piece_dflt, [&](HostPiece &pc) {
            const int64_t ra = pc.ra, pn = pc.pn;
            if (gap_offsets) for (int64_t i = piece_end; i <= ra; ++i) gap_offsets[i] = gbase;
            const rb_batch *b = pc.batch();
            body.prepare(pn, ko.data() + ra, offsets + ra, out_offsets + ra);
            RB_HIP(hipMemcpyAsync(body.own_thr, cov_threshold + ra, (size_t)pn * 4, hipMemcpyHostToDevice, s));
            RB_HIP(hipMemcpyAsync(body.own_txt, seq + offsets[ra], (size_t)body.tb, hipMemcpyHostToDevice, s));
            pc.kernels_begin();
            // the count profile
            ph.begin(0);
            rb::launch_get_kmers(g, b, body.dkof, body.dF, body.dR, body.own_cnt, s);
            ph.end();
            body.run();
            pc.kernels_end();
            const int64_t G = body.G;
            nf.resize((size_t)pn);
            uint32_t over = 0;
            RB_HIP(hipMemcpyAsync(out_seq + out_offsets[ra], body.dctxt, (size_t)body.ctb, hipMemcpyDeviceToHost, s));
            RB_HIP(hipMemcpyAsync(out_len + ra, body.dclen, (size_t)pn * 4, hipMemcpyDeviceToHost, s));
            RB_HIP(hipMemcpyAsync(flags + ra, body.dflags, (size_t)pn * 4, hipMemcpyDeviceToHost, s));
            RB_HIP(hipMemcpyAsync(nf.data(), body.dnf, (size_t)pn * 4, hipMemcpyDeviceToHost, s));
            RB_HIP(hipMemcpyAsync(&over, body.dover, 4, hipMemcpyDeviceToHost, s));
            if (gaps && G > 0) RB_HIP(hipMemcpyAsync(gaps + gbase, body.drecs, (size_t)G * sizeof(rb_corr_gap), hipMemcpyDeviceToHost, s));
            pc.finish();
            ph.collect();
            if (over) {
                set_error("rb_graph_correct_errors: %u sequences of [%lld, %lld) outgrew their slots (internal error)", over, (long long)ra, (long long)pc.rb);
                throw HipError{RB_ERR_STATE};
            }
            for (int64_t i = 0; i < pn; ++i) {
                uint32_t f = flags[ra + i];
                if (nf[(size_t)i] > 0) f |= RB_CORR_MISMATCH;
                if (f) f |= RB_CORR_CORRECTED;
                flags[ra + i] = f;
            }
            if (gaps) for (int64_t i = 0; i < G; ++i) gaps[gbase + i].seq += (int32_t)ra;
            if (gap_offsets) for (int64_t i = 0; i <= pn; ++i) gap_offsets[ra + i] = gbase + body.gof[(size_t)i];
            gbase += G;
            piece_end = pc.rb + 1;
        });
        if (gap_offsets) for (int64_t i = piece_end; i <= n; ++i) gap_offsets[i] = gbase;
        if (ph.on) {
            std::lock_guard<std::mutex> lk(g->qm);
            for (int i = 0; i < CorrPhaseTimer::N; ++i) if (ph.launches[i]) g->prof_add(ph.names[i], ph.ms[i], ph.launches[i]);
        }
    });
}
}  // extern "C"
