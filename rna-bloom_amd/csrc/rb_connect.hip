// rb_connect.hip — connection of read segments through the graph (rb_graph_connect_segments): GraphUtils.connect over a segment list
// (R/util/GraphUtils.java:4836-4872), the two-string connect (:4874-4896) and the six-argument getMaxCoveragePath (:1591-1675), the first step of
// the fragment, single-end and long-read workers (R/RNABloom.java:1980, 2092, 2106, 4781-4829).  A connected string ends with the whole of its right
// segment, so the left k-mer of gap i is always the last k-mer of segment i - 1: every gap's path is independent of every other gap, and only the
// choice of the longest run is sequential.  TWO kernels: k_connect_gaps, a wavefront per gap — both walks, the meeting test and the verdict, with the
// gap's two path rows (a forward hash per k-mer, the walk's text a code per letter) in LDS or, for a large bound, in a row of device scratch the
// wavefront owns; and k_connect_reads, a wavefront per read — the scan of the read's gap records for the run the reference returns and the copy of
// that run's text.  Nothing is written to the graph (DESIGN.md §5 "Connection of read segments").
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rb_pieces.hpp"
#include "rb_lookup.hpp"
#include "rb_align.hpp"
#include "rb_wave.hpp"

using namespace rb;

#pragma clang fp contract(off)

namespace {

constexpr int CN_TPB = 256;
constexpr int CN_WAVES = CN_TPB / 64;            // gaps / reads a workgroup works on at a time: a wavefront each
constexpr int CN_LDS_BOUND = 128;                // the largest bound (gap length + k, so k as well) whose two path rows live in LDS
constexpr int64_t CN_MAX_ROWS = 4096;            // wavefronts of a gap launch (each takes gaps in turn; on device scratch each owns one row) ...
constexpr int64_t CN_MIN_ROWS = 64;
constexpr size_t CN_ROWS_BYTES = (size_t)512 << 20;   // ... fewer when the rows are large: as many as fit this, CN_MIN_ROWS at the least

static_assert(sizeof(rb_connect_rec) == 32 && sizeof(rb_connect_gap_rec) == 32, "the records are 8 ints each");

// A gap's rows for a bound of at most B: per walk the text in walking order (the k codes of its first k-mer, then a code per k-mer added) and the
// forward hashes of the k-mers added
struct CnLayout {
    size_t o_tl, o_tr, o_hl, o_hr, bytes;
    __host__ __device__ constexpr CnLayout(int64_t B, int k)
        : o_tl(0), o_tr(up16((size_t)(k + B + 1))), o_hl(2 * up16((size_t)(k + B + 1))), o_hr(2 * up16((size_t)(k + B + 1)) + (size_t)B * 8),
          bytes(up16(2 * up16((size_t)(k + B + 1)) + (size_t)B * 16)) {}
};
constexpr size_t CN_LDS_ROW_BYTES = CnLayout(CN_LDS_BOUND, CN_LDS_BOUND).bytes;

struct CnGap { int64_t loff, roff, poff; int32_t bound, run; };   // the left segment's last k-mer and the right segment's first in the piece's text; the gap's place
                                                                  // in the path letters; its bound; 0: its read is not judged, the gap is not run
struct CnRead { int64_t ent0, gap0, oof; int32_t n_ent, why; };   // the read's first entry, first gap, place in the text out; its entries; the host's verdict (RB_CONNECT_WHY_*)

struct CnGapArgs {
    FilterView fv;
    int stranded, k;
    float min_cov;
    const uint8_t *txt;                          // the piece's letters as the caller gave them
    const CnGap *gaps;
    const int32_t *order;                        // this launch works on gaps order[0 .. count)
    int64_t count;
    uint8_t *path;                               // per gap, at its poff: the last letter of each k-mer of a connecting path
    rb_connect_gap_rec *grecs;
    uint8_t *rows;
    int64_t rowB;                                // the bound the scratch rows are laid out for
};

struct CnRow { uint8_t *T; uint64_t *H; };

enum { CN_WALK_NONE = 0, CN_WALK_TARGET = 1, CN_WALK_LOOP = 2, CN_WALK_BOUND = 3, CN_WALK_MET = 4 };

// HashSet.contains / the descending search: the first (last: the last) of the n k-mers a walk added that equals the candidate (k codes at cand in the
// ASKING walk's order, forward hash fh), else WAVE_NOWHERE — entry j is the k codes at row.T + j + 1.  rev: the row's walk runs the other way.
__device__ __forceinline__ int cn_find(const CnRow &row, int n, const uint8_t *cand, uint64_t fh, bool rev, bool last, int k, uint32_t lane) {
    return wave_find(0, n, k, [&](int j) { return row.H[j]; }, fh, [&](int j, int q) { return row.T[j + 1 + q]; },
                     [&](int q) { return rev ? cand[k - 1 - q] : cand[q]; }, last, lane);
}

// One walk of getMaxCoveragePath (:1604-1623 to the right, :1630-1672 back): up to `bound` steps of Kmer.getMaxCovSuccessor / getMaxCovPredecessor
// (R/graph/Kmer.java:301-355: the first strictly largest count >= min_cov among A C G T) from the k-mer in own.T[0, k).  Lanes 0..3 roll the four
// neighbours' hashes and probe them side by side; a ballot over the largest key gives the first maximum.  tgt(q): code q of the target in this
// walk's order.  Ends: no neighbour; the best neighbour is the target (not added); it is a k-mer this walk added; the bound; (other != nullptr) it
// is entry `met` of the other walk, the LAST equal one — tested after the loop test, as the reference tests it.  n: the k-mers added.
template <class TGT>
__device__ __forceinline__ int cn_walk(const CnGapArgs &a, const WaveDir<> &dr, const CnRow &own, int bound, TGT tgt, const CnRow *other, int other_n, int &n,
                                       int &met, uint32_t lane) {
    const int k = a.k;
    uint64_t A = 0, B = 0;
    for (int q = 0; q < k; ++q) {
        const uint32_t w = own.T[q];
        A = rotl1(A) ^ seed_of(w ^ dr.xm);
        B ^= rotl_var(seed_of(w ^ dr.ym), (uint32_t)q);
    }
    int len = 0;
    while (len < bound) {
        uint64_t nA = 0, nB = 0;
        uint32_t key = 0;                        // 0: no neighbour with this base; else 1 + its count code
        if (lane < 4u) {
            dr.step(A, B, own.T[len], lane, nA, nB);
            const uint32_t code = count_code(a.fv, dr.hash(nA, nB));
            if (count_code_value(code) >= a.min_cov) key = code + 1u;
        }
        const uint32_t mx = max(max((uint32_t)__shfl((int)key, 0, 64), (uint32_t)__shfl((int)key, 1, 64)),
                                max((uint32_t)__shfl((int)key, 2, 64), (uint32_t)__shfl((int)key, 3, 64)));
        if (mx == 0u) { n = len; return CN_WALK_NONE; }
        const int bi = (int)__builtin_ctzll(__ballot(lane < 4u && key == mx));
        nA = wave_shfl64(nA, bi); nB = wave_shfl64(nB, bi);
        if (lane == 0) own.T[len + k] = (uint8_t)bi;
        wave_fence();
        const uint8_t *cand = own.T + len + 1;
        bool ne = false;
        for (int q = (int)lane; q < k; q += 64) ne = ne || cand[q] != tgt(q);
        if (!__ballot(ne)) { n = len; return CN_WALK_TARGET; }
        const uint64_t fh = dr.fwd(nA, nB);
        if (cn_find(own, len, cand, fh, false, false, k, lane) >= 0) { n = len; return CN_WALK_LOOP; }
        if (other) {
            const int j = cn_find(*other, other_n, cand, fh, true, true, k, lane);
            if (j >= 0) { n = len; met = j; return CN_WALK_MET; }
        }
        if (lane == 0) own.H[len] = fh;
        A = nA; B = nB;
        ++len;
        wave_fence();
    }
    n = len;
    return CN_WALK_BOUND;
}

__device__ __forceinline__ int cn_end_of(int walk_end) {
    return walk_end == CN_WALK_NONE ? RB_CONNECT_END_NO_NEIGHBOR : walk_end == CN_WALK_TARGET ? RB_CONNECT_END_ARRIVED
         : walk_end == CN_WALK_LOOP ? RB_CONNECT_END_LOOP : walk_end == CN_WALK_BOUND ? RB_CONNECT_END_BOUND : RB_CONNECT_END_MET;
}

// the record of a gap that is not run (its read is not judged)
__device__ __forceinline__ rb_connect_gap_rec cn_gap_not_run() {
    rb_connect_gap_rec v;
    v.connected = 0; v.how = RB_CONNECT_HOW_NOT_RUN; v.l_end = v.r_end = RB_CONNECT_END_NOT_RUN;
    v.l_added = v.r_added = 0; v.index = -1; v.path_len = 0;
    return v;
}

// gap gi of the piece by one wavefront with the rows WL / WR
__device__ __forceinline__ void cn_gap(const CnGapArgs &a, const CnRow &WL, const CnRow &WR, int64_t gi, uint32_t lane) {
    const int k = a.k;
    const CnGap gp = a.gaps[gi];
    rb_connect_gap_rec v = cn_gap_not_run();
    bool bad = gp.run == 0;
    if (!bad) {
        // the two k-mers in walking order; a letter outside ACGTU in either: the read is not judged (k_connect_reads says so), the gap is not run
        const uint8_t *lt = a.txt + gp.loff, *rt = a.txt + gp.roff;
        bool b = false;
        for (int q = (int)lane; q < k; q += 64) {
            const uint32_t cl = letter_code(lt[q]), cr = letter_code(rt[k - 1 - q]);
            b = b || cl > 3u || cr > 3u;
            WL.T[q] = (uint8_t)(cl & 3u); WR.T[q] = (uint8_t)(cr & 3u);
        }
        bad = __ballot(b) != 0ull;
        wave_fence();
    }
    if (bad) {
        if (lane == 0) a.grecs[gi] = v;
        return;
    }
    const int bound = gp.bound;
    const WaveDir<> dl = wave_dir(a.stranded, k, 0), drr = wave_dir(a.stranded, k, 1);
    // form 0: null; 1: the left walk arrived, the path is its nl k-mers; 2: the right walk met entry idx of the left path, the path is entries 0 .. idx
    // and the nr k-mers of the right walk; 3: the right walk arrived, the path is its nr k-mers
    int form = 0, nl = 0, nr = 0, idx = -1, plen = 0, met = -1;
    const int endl = cn_walk(a, dl, WL, bound, [&](int q) -> uint8_t { return WR.T[k - 1 - q]; }, nullptr, 0, nl, met, lane);
    v.l_end = cn_end_of(endl); v.l_added = nl;
    if (endl == CN_WALK_TARGET) { form = 1; plen = nl; v.how = RB_CONNECT_HOW_LEFT_ARRIVED; }
    else {
        const int endr = cn_walk(a, drr, WR, bound, [&](int q) -> uint8_t { return WL.T[k - 1 - q]; }, &WL, nl, nr, met, lane);
        v.r_end = cn_end_of(endr); v.r_added = nr;
        if (endr == CN_WALK_TARGET) { form = 3; plen = nr; v.how = RB_CONNECT_HOW_RIGHT_ARRIVED; }
        else if (endr == CN_WALK_LOOP) v.how = RB_CONNECT_HOW_RIGHT_LOOP;
        else if (endr == CN_WALK_MET) {
            const uint8_t *cand = WR.T + nr + 1;                                // the k-mer met, in the right walk's order
            v.index = met;
            if (ce_low_complexity([&](int q) -> uint32_t { return code_letter(cand[k - 1 - q]); }, k, lane)) v.how = RB_CONNECT_HOW_MEET_LOW_COMPLEXITY;
            else { form = 2; idx = met; plen = idx + 1 + nr; v.how = RB_CONNECT_HOW_PATHS_MEET; }
        } else v.how = RB_CONNECT_HOW_EXHAUSTED;
    }
    v.path_len = plen;
    v.connected = form != 0 && plen > 0 && plen <= bound;
    if (v.connected) {
        // the last letter of path k-mer x: a left entry's is the code it added; a right entry's is the first code of its k-mer in the right walk's order
        uint8_t *o = a.path + gp.poff;
        for (int x = (int)lane; x < plen; x += 64) {
            const uint8_t c = form == 1 ? WL.T[x + k] : form == 2 ? (x <= idx ? WL.T[x + k] : WR.T[nr + 1 + idx - x]) : WR.T[nr - x];
            o[x] = code_letter(c);
        }
    }
    if (lane == 0) a.grecs[gi] = v;
}

// A wavefront per gap, taking the launch's gaps in turn.  LDS_ROW: the gap's rows are in LDS (every bound of the launch <= CN_LDS_BOUND); else in
// the row of device scratch the wavefront owns, laid out for rowB.
template <bool LDS_ROW>
__global__ void __launch_bounds__(CN_TPB) k_connect_gaps(CnGapArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_row[CN_WAVES][LDS_ROW ? CN_LDS_ROW_BYTES : 16];
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const int64_t slot = (int64_t)blockIdx.x * CN_WAVES + wv, n_slots = (int64_t)gridDim.x * CN_WAVES;
    const CnLayout lay = LDS_ROW ? CnLayout(CN_LDS_BOUND, CN_LDS_BOUND) : CnLayout(a.rowB, a.k);
    uint8_t *row;
    if constexpr (LDS_ROW) row = s_row[wv]; else row = a.rows + (size_t)slot * lay.bytes;
    const CnRow WL{row + lay.o_tl, reinterpret_cast<uint64_t *>(row + lay.o_hl)}, WR{row + lay.o_tr, reinterpret_cast<uint64_t *>(row + lay.o_hr)};
    for (int64_t i = slot; i < a.count; i += n_slots) {
        cn_gap(a, WL, WR, (int64_t)a.order[i], lane);
        wave_fence();
    }
}

struct CnReadArgs {
    int k;
    int64_t pn;
    const uint8_t *txt;
    const int64_t *ent_off;                      // the piece's entries in txt
    const CnRead *reads;
    const CnGap *gaps;
    const uint8_t *path;
    rb_connect_gap_rec *grecs;
    rb_connect_rec *recs;
    uint8_t *out;
};

// A wavefront per read: the reference's loop over the read's gap records (:4848-4868) for the run it returns, the earlier one where two are equally
// long, and that run's text — the first segment, then per connected gap the path's letters and right[k - 1 ..], which is the formula of :4895
// byte for byte also where a path shorter than k - 1 k-mers lets the right segment overlap the left one.
__global__ void __launch_bounds__(CN_TPB) k_connect_reads(CnReadArgs a) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t r = (int64_t)blockIdx.x * CN_WAVES + wv;
    if (r >= a.pn) return;
    const int k = a.k;
    const CnRead rd = a.reads[r];
    const int64_t *eo = a.ent_off + rd.ent0;
    uint8_t *o = a.out + rd.oof;
    auto len_of = [&](int e) { return (int)(eo[e + 1] - eo[e]); };
    rb_connect_rec v;
    v.outcome = RB_CONNECT_NOT_JUDGED; v.why = rd.why; v.gaps = rd.n_ent / 2; v.connected = 0; v.first_seg = v.last_seg = -1; v.out_len = 0; v.pad = 0;
    if (rd.n_ent == 0) v.outcome = RB_CONNECT_EMPTY;
    else if (rd.n_ent == 1) {                                                    // the entry, untouched
        const int len = len_of(0);
        const uint8_t *t = a.txt + eo[0];
        for (int p = (int)lane; p < len; p += 64) o[p] = t[p];
        v.outcome = RB_CONNECT_SINGLE; v.first_seg = v.last_seg = 0; v.out_len = len;
    } else if (rd.why == RB_CONNECT_WHY_NONE) {
        bool b = false;
        for (int e = 0; e < rd.n_ent; e += 2) {
            const uint8_t *t = a.txt + eo[e];
            const int len = len_of(e);
            for (int p = (int)lane; p < len; p += 64) b = b || letter_code(t[p]) > 3u;
        }
        if (__ballot(b)) {
            v.why = RB_CONNECT_WHY_INVALID_LETTER;
            const rb_connect_gap_rec nr = cn_gap_not_run();
            for (int gi = (int)lane; gi < v.gaps; gi += 64) a.grecs[rd.gap0 + gi] = nr;
        } else {
            int last_start = 0, last_len = len_of(0), best_start = 0, best_end = 0, best_len = last_len;
            for (int e = 2; e < rd.n_ent; e += 2) {
                const rb_connect_gap_rec gr = a.grecs[rd.gap0 + (e - 1) / 2];
                if (gr.connected) {
                    ++v.connected;
                    last_len += gr.path_len + len_of(e) - k + 1;
                } else { last_start = e; last_len = len_of(e); }
                if (last_len > best_len) { best_start = last_start; best_end = e; best_len = last_len; }
            }
            int cur = len_of(best_start);
            {
                const uint8_t *t = a.txt + eo[best_start];
                for (int p = (int)lane; p < cur; p += 64) o[p] = code_letter(letter_code(t[p]));
            }
            for (int e = best_start + 2; e <= best_end; e += 2) {
                const int64_t g = rd.gap0 + (e - 1) / 2;
                const int plen = a.grecs[g].path_len, tail = len_of(e) - (k - 1);
                const uint8_t *pl = a.path + a.gaps[g].poff, *t = a.txt + eo[e] + (k - 1);
                for (int x = (int)lane; x < plen; x += 64) o[cur + x] = pl[x];
                cur += plen;
                for (int x = (int)lane; x < tail; x += 64) o[cur + x] = code_letter(letter_code(t[x]));
                cur += tail;
            }
            v.outcome = RB_CONNECT_CHAINED; v.first_seg = best_start; v.last_seg = best_end; v.out_len = cur;
        }
    }
    if (lane == 0) a.recs[r] = v;
}

void connect_call(rb_graph *g, const char *seq, const int64_t *so, const int64_t *rs, int64_t n, int lookahead, float min_cov, int64_t *out_offsets,
                  char *out_seq, rb_connect_rec *recs, rb_connect_gap_rec *grecs) {
    const char *who = "rb_graph_connect_segments";
    (void)lookahead;                                          // (the six-argument getMaxCoveragePath never reads it: rb_capi.h)
    RB_REQUIRE(g, "%s: null handle", who);
    RB_REQUIRE(!g->shard, "%s: not available on a shard handle", who);
    RB_REQUIRE(g->dbg.bits && g->cbf, "%s: dbgbf or the counting filter has been destroyed", who);
    RB_REQUIRE(std::isfinite(min_cov) && min_cov >= 0.0f, "%s: min_kmer_cov must be finite and not negative", who);
    RB_REQUIRE(n >= 0, "%s: n = %lld", who, (long long)n);
    if (n == 0) return;
    RB_REQUIRE(so && rs && out_offsets, "%s: null argument", who);
    RB_REQUIRE(recs || !out_seq, "%s: out_seq needs recs", who);
    const int k = g->k;
    for (int64_t i = 0; i < n; ++i) RB_REQUIRE(rs[i + 1] >= rs[i], "%s: decreasing read_segs at read %lld", who, (long long)i);
    // per read: the capacity of its text, its gaps, the host's verdict, its cost (letters + bounds: what a piece is cut by)
    std::vector<int64_t> gcum((size_t)n + 1, 0), cost((size_t)n + 1, 0);
    std::vector<int32_t> why((size_t)n, RB_CONNECT_WHY_NONE);
    out_offsets[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t m = rs[i + 1] - rs[i];
        RB_REQUIRE(m <= INT32_MAX / 2, "%s: read %lld has more entries than an int holds", who, (long long)i);
        int64_t cap = 0, bounds = 0;
        for (int64_t j = 0; j < m; ++j) {
            const int64_t len = so[rs[i] + j + 1] - so[rs[i] + j];
            RB_REQUIRE(len >= 0, "%s: decreasing seg_offsets at entry %lld", who, (long long)(rs[i] + j));
            if (j & 1) {
                RB_REQUIRE(len + k <= RB_CONNECT_MAX_BOUND, "%s: the gap at entry %lld has a bound of %lld (at most %d)", who, (long long)(rs[i] + j),
                           (long long)(len + k), RB_CONNECT_MAX_BOUND);
                cap += len + 1; bounds += len + k;
            } else {
                cap += len;
                if (m > 1 && len < k && why[(size_t)i] == RB_CONNECT_WHY_NONE) why[(size_t)i] = RB_CONNECT_WHY_SHORT;
            }
        }
        RB_REQUIRE(so[rs[i + 1]] - so[rs[i]] <= INT32_MAX / 2, "%s: read %lld has more letters than an int holds", who, (long long)i);
        if (m > 1 && !(m & 1)) why[(size_t)i] = RB_CONNECT_WHY_EVEN_COUNT;
        gcum[(size_t)i + 1] = gcum[(size_t)i] + m / 2;
        cost[(size_t)i + 1] = cost[(size_t)i] + (so[rs[i + 1]] - so[rs[i]]) + bounds + 1;
        out_offsets[i + 1] = out_offsets[i] + cap;
    }
    RB_REQUIRE(so[rs[n]] == so[rs[0]] || seq, "%s: null sequence text", who);
    if (!out_seq) return;
    RB_HIP(hipSetDevice(g->p.device));
    HostPin pin_out(out_seq, (size_t)out_offsets[n]), pin_rec(recs, (size_t)n * sizeof(rb_connect_rec));
    QueryLease q(g);
    hipStream_t s = q.c->st;
    // piece by piece (rb_pieces.hpp), whole reads, cut by the letters and the bounds: b0 the piece's tables, b1 its text, b2 the path letters and the
    // wavefronts' rows, b3 the records and the text out; with profiling on the kernels of every piece are timed: entry "connect"
    std::vector<uint8_t> tab;
    for_each_piece(g, s, [&](int64_t i) { return cost[(size_t)i]; }, n, (int64_t)16 << 20, "connect", [&](Piece &pc) {
        const int64_t ra = pc.ra, rb_ = pc.rb, pn = pc.pn;
        const int64_t ea = rs[ra], pe = rs[rb_] - ea, t0 = so[ea], pt = so[rs[rb_]] - t0, pg = gcum[(size_t)rb_] - gcum[(size_t)ra];
        const int64_t ot = out_offsets[rb_] - out_offsets[ra];
        // the tables: entry offsets [pe + 1], reads [pn], gaps [pg], the gaps' order [pg] — those whose rows fit LDS first
        const size_t o_eo = 0, o_rd = up16((size_t)(pe + 1) * 8), o_gp = o_rd + (size_t)pn * sizeof(CnRead), o_or = o_gp + (size_t)pg * sizeof(CnGap),
                     tab_bytes = up16(o_or + (size_t)pg * 4);
        tab.assign(tab_bytes, 0);
        int64_t *eo = reinterpret_cast<int64_t *>(tab.data() + o_eo);
        CnRead *rd = reinterpret_cast<CnRead *>(tab.data() + o_rd);
        CnGap *gp = reinterpret_cast<CnGap *>(tab.data() + o_gp);
        int32_t *order = reinterpret_cast<int32_t *>(tab.data() + o_or);
        for (int64_t j = 0; j <= pe; ++j) eo[j] = so[ea + j] - t0;
        int64_t gi = 0, pl = 0, small = 0, rowB = 0;
        for (int64_t i = 0; i < pn; ++i) {
            const int64_t r = ra + i, first = rs[r] - ea, m = rs[r + 1] - rs[r];
            rd[i] = CnRead{first, gi, out_offsets[r] - out_offsets[ra], (int32_t)m, why[(size_t)r]};
            for (int64_t j = 1; j < m; j += 2, ++gi) {
                const int64_t bound = eo[first + j + 1] - eo[first + j] + k;
                const bool run = why[(size_t)r] == RB_CONNECT_WHY_NONE;
                gp[gi] = CnGap{run ? eo[first + j] - k : 0, run ? eo[first + j + 1] : 0, pl, (int32_t)bound, run ? 1 : 0};
                pl += bound;
                if (bound <= CN_LDS_BOUND) ++small; else rowB = std::max(rowB, bound);
            }
        }
        {
            int64_t a_small = 0, a_large = small;
            for (int64_t x = 0; x < pg; ++x) order[gp[x].bound <= CN_LDS_BOUND ? a_small++ : a_large++] = (int32_t)x;
        }
        const int64_t large = pg - small;
        const CnLayout lay(std::max<int64_t>(rowB, 1), k);
        const int64_t rows = std::min(std::min(large, CN_MAX_ROWS), std::max(CN_MIN_ROWS, (int64_t)(CN_ROWS_BYTES / lay.bytes)));
        const unsigned blocks_large = blocks_for(rows, CN_WAVES), blocks_small = blocks_for(std::min(small, CN_MAX_ROWS), CN_WAVES);
        const size_t o_rows = up16((size_t)pl + 16);
        const size_t o_grec = 0, o_rec = o_grec + (size_t)pg * sizeof(rb_connect_gap_rec), o_txt = o_rec + (size_t)pn * sizeof(rb_connect_rec);
        q.c->b0.reserve(tab_bytes + 16);
        q.c->b1.reserve((size_t)pt + 16);
        q.c->b2.reserve(o_rows + (size_t)blocks_large * CN_WAVES * lay.bytes + 16);
        q.c->b3.reserve(o_txt + (size_t)ot + 16);
        uint8_t *d_tab = q.c->b0.as<uint8_t>(), *d_txt = q.c->b1.as<uint8_t>(), *base2 = q.c->b2.as<uint8_t>(), *base3 = q.c->b3.as<uint8_t>();
        RB_HIP(hipMemcpyAsync(d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, s));
        if (pt) RB_HIP(hipMemcpyAsync(d_txt, seq + t0, (size_t)pt, hipMemcpyHostToDevice, s));
        pc.kernels_begin();
        if (ot) RB_HIP(hipMemsetAsync(base3 + o_txt, 0, (size_t)ot, s));                // (what no read writes comes back as zeros, whatever the cuts)
        CnGapArgs a;
        a.fv = g->view(0, 0);
        a.stranded = (int)g->stranded; a.k = k; a.min_cov = min_cov;
        a.txt = d_txt;
        a.gaps = reinterpret_cast<const CnGap *>(d_tab + o_gp);
        a.path = base2;
        a.grecs = reinterpret_cast<rb_connect_gap_rec *>(base3 + o_grec);
        a.rows = base2 + o_rows;
        a.rowB = std::max<int64_t>(rowB, 1);
        if (small) {
            a.order = reinterpret_cast<const int32_t *>(d_tab + o_or); a.count = small;
            hipLaunchKernelGGL((k_connect_gaps<true>), dim3(blocks_small), dim3(CN_TPB), 0, s, a);
            RB_HIP(hipGetLastError());
        }
        if (large) {
            a.order = reinterpret_cast<const int32_t *>(d_tab + o_or) + small; a.count = large;
            hipLaunchKernelGGL((k_connect_gaps<false>), dim3(blocks_large), dim3(CN_TPB), 0, s, a);
            RB_HIP(hipGetLastError());
        }
        CnReadArgs ar;
        ar.k = k; ar.pn = pn; ar.txt = d_txt;
        ar.ent_off = reinterpret_cast<const int64_t *>(d_tab + o_eo);
        ar.reads = reinterpret_cast<const CnRead *>(d_tab + o_rd);
        ar.gaps = a.gaps; ar.path = base2; ar.grecs = a.grecs;
        ar.recs = reinterpret_cast<rb_connect_rec *>(base3 + o_rec);
        ar.out = base3 + o_txt;
        hipLaunchKernelGGL(k_connect_reads, dim3(blocks_for(pn, CN_WAVES)), dim3(CN_TPB), 0, s, ar);
        RB_HIP(hipGetLastError());
        pc.kernels_end();
        RB_HIP(hipMemcpyAsync(recs + ra, ar.recs, (size_t)pn * sizeof(rb_connect_rec), hipMemcpyDeviceToHost, s));
        if (grecs && pg) RB_HIP(hipMemcpyAsync(grecs + gcum[(size_t)ra], a.grecs, (size_t)pg * sizeof(rb_connect_gap_rec), hipMemcpyDeviceToHost, s));
        if (ot) RB_HIP(hipMemcpyAsync(out_seq + out_offsets[ra], ar.out, (size_t)ot, hipMemcpyDeviceToHost, s));
    });
}

}  // namespace

extern "C" {
int rb_graph_connect_segments(rb_graph *g, const char *seq, const int64_t *seg_offsets, const int64_t *read_segs, int64_t n, int lookahead, float min_kmer_cov,
                              int64_t *out_offsets, char *out_seq, rb_connect_rec *recs, rb_connect_gap_rec *gaps) {
    return guarded([&] { connect_call(g, seq, seg_offsets, read_segs, n, lookahead, min_kmer_cov, out_offsets, out_seq, recs, gaps); });
}
}  // extern "C"
