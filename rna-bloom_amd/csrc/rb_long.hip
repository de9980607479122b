// rb_long.hip — windowed correction of long reads (rb_graph_correct_long): GraphUtils.correctLongSequenceWindowed (R/util/GraphUtils.java:3087-3185),
// the second step of LongReadCorrectionWorker.run (R/RNABloom.java:3788-3840), with getCoverageStats (:1799-1848), correctInternalErrors (:3402-3602),
// the six-argument getMaxCoveragePath (:1591-1675) and trimLowCoverageEdgeKmers (:3187-3241).  Unlike correctErrorHelper (rb_correct.hip) the gaps of
// a window depend on each other — the left anchor is looked for in the CORRECTED list, an accepted path moves the cursor — so a window is one
// sequential job; windows of a pass are independent.  A wavefront per window and pass: k_long_window finds the window's threshold from a histogram
// of its count codes in LDS, scans it with ballots and resolves every run where it stands: an SNV bubble with a lane per candidate window, a path
// with the wavefront-level maximum-coverage step (lanes 0..3 roll and probe the four neighbours, rb_lookup.hpp) and hash sweeps confirmed on the
// bases for HashSet.contains / Kmer.equals, the percent identity by rb_align.hpp.  Every list of the reference is a chain of k-mers overlapping by
// k - 1 letters (rb_capi.h), so a list is its text: per pass the host cuts the windows, k_long_window writes each window's letters into its slot,
// k_long_stitch joins the slots into the sequence's next text and k_long_profile counts its k-mers; texts and counts stay on the device, sequences
// whose pass corrected nothing leave the live list through k_long_finish (edge trim, the copy into the caller's layout).  Nothing is written to the
// graph (DESIGN.md §5 "Long-read correction").
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

// Java float arithmetic: medians, the dropoff product and the percent identity are single float32 operations
#pragma clang fp contract(off)

namespace {

constexpr int LW_TPB = 256;
constexpr int LW_WAVES = LW_TPB / 64;            // windows / sequences a workgroup works on at a time: a wavefront each
constexpr int64_t LW_MAX_SLOTS = 2048;           // wavefronts of a window launch (each owns one set of rows in device scratch and takes windows in turn)
constexpr int64_t LW_MAX_SLOT = (int64_t)1 << 30;   // k-mers of a window's slot at the most: window_size * (2 + max(max_indel_size, 1)) is checked against it
constexpr int LW_MAX_INDEL = 4096;               // rb_graph_correct_errors' cap
constexpr int LW_NCTR = 10;                      // the record's event counters
constexpr int LW_RES = 2 + LW_NCTR;              // ints a window returns: k-mers, state, counters
enum { LW_SAME = 0, LW_CORRECTED = 1, LW_OUTGROWN = 2 };
enum { C_SNV_REPLACED = 0, C_SNV_KEPT, C_PATH_NONE, C_ZERO_ACCEPTED, C_ZERO_KEPT, C_10X, C_IDENTITY, C_COV_KEPT, C_SHORT, C_ANCHOR };

static_assert(sizeof(rb_long_rec) == 64, "rb_long_rec is 16 ints");

#define LW_FENCE_LDS() __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup")

struct LwSeq { int64_t toff, koff; int32_t len, nk; };                       // a sequence in the current text / count buffers
struct LwWin { int64_t toff, koff, ooff; int32_t n, cap; };                  // a window: its first letter, its first count, its slot (bytes into the slots), its k-mers, the slot's k-mers
struct LwJoin { int64_t src, dst; int32_t wfirst, nwin; };                   // a corrected sequence: its text now, its next text, its windows
struct LwFin { int64_t toff, koff, ooff; int32_t len, nk, cap, trim, id; };  // a sequence that leaves: where it is, its place and room in the caller's layout
struct LwOut { int32_t out_len, trim_begin, trim_end, flags, trimmed; };

// a wavefront's rows in device scratch: the counts of kmers2 (a slot's k-mers at the most), per walk the text (k + B codes in walking order), the
// forward hashes and count codes of the k-mers it added (B: the largest bound, the longest window + max_indel_size), the alignment's row
struct LwLayout {
    size_t o_c2, o_tl, o_tr, o_hl, o_hr, o_cl, o_cr, o_lev, bytes;
    __host__ __device__ LwLayout(int64_t cap, int64_t B, int64_t W, int k) {
        o_c2 = 0; o_tl = up16(o_c2 + (size_t)cap); o_tr = up16(o_tl + (size_t)(k + B + 1)); o_hl = up16(o_tr + (size_t)(k + B + 1));
        o_hr = o_hl + (size_t)B * 8; o_cl = o_hr + (size_t)B * 8; o_cr = up16(o_cl + (size_t)B); o_lev = up16(o_cr + (size_t)B);
        bytes = up16(o_lev + (size_t)(W + k) * 4);
    }
};

struct LwArgs {
    FilterView fv;
    int stranded, k, lookahead, max_indel, maxld;     // maxld: maxLengthDifference (:3473-3476)
    float grad, pid, min_cov;
    const uint8_t *txt, *cnt;                         // the live sequences' letters and count codes
    const LwWin *win;
    int64_t nwin;
    uint8_t *slots;                                   // per window: k - 1 letters before its first k-mer's last, then a letter per k-mer of kmers2
    int32_t *res;                                     // [nwin][LW_RES]
    uint8_t *rows;
    int64_t capmax, B, W;
};

// the largest count code among the lanes' and the lowest lane that holds it, as code * 64 + (63 - lane); all lanes get it
__device__ __forceinline__ uint32_t lw_max_key(uint32_t code, uint32_t lane) {
    uint32_t key = code * 64u + (63u - lane);
    for (int s = 32; s > 0; s >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, s, 64));
    return key;
}

// ---- getKmers' counts of device text: a wavefront per sequence, a lane per 32 windows (hashes rolled as k_text_kmers of rb_correct.hip rolls them);
// a window with a letter outside ACGTU counts 0
__global__ void __launch_bounds__(LW_TPB) k_long_profile(FilterView fv, int stranded, int k, const LwSeq *__restrict__ seqs, int64_t n,
                                                         const uint8_t *__restrict__ txt, uint8_t *__restrict__ cnt) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u, uk = (uint32_t)k;
    const int64_t r = (int64_t)blockIdx.x * LW_WAVES + wv;
    if (r >= n) return;
    const LwSeq sq = seqs[r];
    const uint8_t *tx = txt + sq.toff;
    uint8_t *c_ = cnt + sq.koff;
    const int32_t nk = sq.nk;
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
            c_[p] = (uint8_t)(run >= k ? count_code(fv, stranded ? f : canonical(f, rv)) : 0u);
        }
    }
}

// ---- the solid-k-mer screen (:3099-3110): k-mers with count >= min_cov, a wavefront per sequence
__global__ void __launch_bounds__(LW_TPB) k_long_solid(const LwSeq *__restrict__ seqs, int64_t n, const uint8_t *__restrict__ cnt, float min_cov,
                                                       int32_t *__restrict__ nsolid) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t r = (int64_t)blockIdx.x * LW_WAVES + wv;
    if (r >= n) return;
    const LwSeq sq = seqs[r];
    const uint8_t *c_ = cnt + sq.koff;
    int ns = 0;
    for (int32_t p0 = 0; p0 < sq.nk; p0 += 64) {
        const int32_t p = p0 + (int32_t)lane;
        ns += __popcll(__ballot(p < sq.nk && count_code_value(c_[p]) >= min_cov));
    }
    if (lane == 0) nsolid[r] = ns;
}

// the first index in [from, n) whose k-mer is bad (count < T) / good, else n
__device__ __forceinline__ int lw_next(const uint8_t *c, int from, int n, float T, bool want_bad, uint32_t lane) {
    return wave_first(from, n, [&](int j) { return (count_code_value(c[j]) < T) == want_bad; }, lane);
}

// a walk's rows: T the k codes of its first k-mer in walking order and a code per k-mer added, H / C the forward hash and count code of those
struct LwRow { uint8_t *T; uint64_t *H; uint8_t *C; };

// HashSet.contains / indexOf: the entry of the n a walk added that equals the candidate (k codes at cand, forward hash fh), else WAVE_NOWHERE — entry j
// is the k codes at row.T + j + 1.  rev: the row's walk runs the other way.
__device__ __forceinline__ int lw_find(const LwRow &row, int n, const uint8_t *cand, uint64_t fh, bool rev, int k, uint32_t lane) {
    return wave_find(0, n, k, [&](int j) { return row.H[j]; }, fh, [&](int j, int q) { return row.T[j + 1 + q]; },
                     [&](int q) { return rev ? cand[k - 1 - q] : cand[q]; }, false, lane);
}

// One walk of getMaxCoveragePath (:1604-1623 to the right, :1630-1672 back): up to `bound` steps of Kmer.getMaxCovSuccessor / getMaxCovPredecessor
// (R/graph/Kmer.java:301-355: the first strictly largest count >= min_cov among A C G T) from the k-mer in own.T[0, k).  tgt(q): code q of the
// target in this walk's order.  Ends 0: no neighbour; 1: the best neighbour is the target (not added); 2: it is a k-mer this walk added; 3: the
// bound; 4: (other != nullptr) it is entry `met` of the other walk — tested after 2, as the reference tests it.  n: the k-mers added.
enum { LW_END_NONE = 0, LW_END_TARGET = 1, LW_END_LOOP = 2, LW_END_BOUND = 3, LW_END_MET = 4 };
template <class TGT>
__device__ int lw_walk(const LwArgs &a, const WaveDir<> &dr, const LwRow &own, int bound, TGT tgt, const LwRow *other, int other_n, int &n, int &met,
                       uint32_t lane) {
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
        uint32_t code = 0;
        if (lane < 4u) {
            dr.step(A, B, own.T[len], lane, nA, nB);
            code = count_code(a.fv, dr.hash(nA, nB));
        }
        int bi = -1;
        uint32_t bcode = 0;
        for (int b = 0; b < 4; ++b) {
            const uint32_t cb = (uint32_t)__shfl((int)code, b, 64);
            if (count_code_value(cb) >= a.min_cov && (bi < 0 || cb > bcode)) { bi = b; bcode = cb; }
        }
        if (bi < 0) { n = len; return LW_END_NONE; }
        nA = wave_shfl64(nA, bi); nB = wave_shfl64(nB, bi);
        if (lane == 0) own.T[len + k] = (uint8_t)bi;
        wave_fence();
        const uint8_t *cand = own.T + len + 1;
        bool ne = false;
        for (int q = (int)lane; q < k; q += 64) ne = ne || cand[q] != tgt(q);
        if (!__ballot(ne)) { n = len; return LW_END_TARGET; }
        const uint64_t fh = dr.fwd(nA, nB);
        if (lw_find(own, len, cand, fh, false, k, lane) >= 0) { n = len; return LW_END_LOOP; }
        if (other) {
            const int j = lw_find(*other, other_n, cand, fh, true, k, lane);
            if (j >= 0) { n = len; met = j; return LW_END_MET; }
        }
        if (lane == 0) { own.H[len] = fh; own.C[len] = (uint8_t)bcode; }
        A = nA; B = nB;
        ++len;
        wave_fence();
    }
    n = len;
    return LW_END_BOUND;
}

// correctInternalErrors of window w with the threshold of its counts, by one wavefront
__device__ void lw_window(const LwArgs &a, int64_t w, uint8_t *row, int *hist, uint8_t (*snv)[RB_MAX_K], uint32_t lane) {
    const int k = a.k;
    const LwWin wn = a.win[w];
    const int n = wn.n, cap = wn.cap;
    const uint8_t *tx = a.txt + wn.toff, *c = a.cnt + wn.koff;
    int32_t *res = a.res + w * LW_RES;
    int ctr[LW_NCTR];
    for (int q = 0; q < LW_NCTR; ++q) ctr[q] = 0;
    int state = LW_SAME, m = 0;
    auto done = [&]() {
        if (lane == 0) {
            res[0] = state == LW_CORRECTED ? m : n;
            res[1] = state;
            for (int q = 0; q < LW_NCTR; ++q) res[2 + q] = ctr[q];
        }
    };
    if (n < a.lookahead) { done(); return; }                                    // :3140
    // ---- getCoverageStats (:1799-1848) from the histogram of the 129 count codes
    for (int q = (int)lane; q < 129; q += 64) hist[q] = 0;
    LW_FENCE_LDS();
    for (int j = (int)lane; j < n; j += 64) atomicAdd(&hist[c[j]], 1);
    LW_FENCE_LDS();
    float T;
    {
        auto kth = [&](int rank) -> uint32_t {                                  // sorted[rank] as a code
            int cum = 0;
            for (uint32_t q = 0; q < 129u; ++q) { cum += hist[q]; if (cum > rank) return q; }
            return 128u;
        };
        const float hi = count_code_value(kth(n / 2));
        T = (n & 1) ? hi : (count_code_value(kth(n / 2 - 1)) + hi) / 2.0f;
        float dropoff = 0.0f;
        {
            const int idx = n - a.lookahead;                                    // the walk starts at sorted[idx] and goes down
            const uint32_t c0 = kth(idx);
            int below = 0;
            for (uint32_t q = 0; q < c0; ++q) below += hist[q];
            float last = count_code_value(c0);
            bool found = idx - below > 0 && last < last * a.grad;               // the next entry has the same count
            if (!found)
                for (int q = (int)c0 - 1; q >= 0; --q) {
                    if (hist[q] == 0) continue;
                    const float cv = count_code_value((uint32_t)q);
                    if (cv < last * a.grad) { found = true; break; }
                    last = cv;
                    if (hist[q] > 1 && cv < cv * a.grad) { found = true; break; }
                }
            if (found) dropoff = last;
        }
        if (dropoff > 0.0f) T = fmaxf(dropoff, a.min_cov);
    }
    if (!(T > 0.0f)) { done(); return; }                                        // no count is below it
    // ---- the scan (:3420-3595).  slot: k - 1 letters, then the last letter of every k-mer of kmers2; C2: their count codes
    uint8_t *slot = a.slots + wn.ooff, *out = slot + (k - 1);
    const LwLayout lay(a.capmax, a.B, a.W, k);
    uint8_t *C2 = row + lay.o_c2;
    const LwRow WL{row + lay.o_tl, reinterpret_cast<uint64_t *>(row + lay.o_hl), row + lay.o_cl};
    const LwRow WR{row + lay.o_tr, reinterpret_cast<uint64_t *>(row + lay.o_hr), row + lay.o_cr};
    int *lev = reinterpret_cast<int *>(row + lay.o_lev);
    for (int x = (int)lane; x < k - 1; x += 64) slot[x] = tx[x];
    bool corrected = false, outgrown = false;
    auto append_orig = [&](int from, int to) {                                  // window k-mers [from, to) as they are
        const int cnt = to - from;
        if (m + cnt > cap) { outgrown = true; return; }
        for (int x = (int)lane; x < cnt; x += 64) { out[m + x] = tx[from + x + k - 1]; C2[m + x] = c[from + x]; }
        m += cnt;
        wave_fence();
    };
    int i = 0, rs = 0;                                                          // the cursor; the first k-mer of the open run (numBadKmersSince = i - rs)
    while (i < n && !outgrown) {
        if (i == rs) {                                                          // no run open: good k-mers up to the next bad one
            const int g = lw_next(c, i, n, T, true, lane);
            append_orig(i, g);
            i = rs = g;
            if (g >= n) break;
        }
        const int e = lw_next(c, i, n, T, false, lane);                         // the good k-mer that ends the run
        if (e >= n) { i = n; break; }
        const int run = e - rs;
        int nxt = e;                                                            // the k-mer appended behind the run (:3578)
        if (m == 0) append_orig(rs, e);                                         // :3426-3431
        else if (run == k - 1) {                                                // ---- an SNV bubble (:3432-3467)
            // S = first bad k-mer[0, k-1) + var = tx[rs .. e) + n + tx[e .. e + k - 1): letter k - 1 is the candidate's, every window holds it
            auto S = [&](int x) -> uint32_t { return x < k - 1 ? tx[rs + x] : tx[rs + x - 1]; };
            for (int win = (int)lane; win < k; win += 64) {
                uint64_t f = 0, r = 0;
                bool ok = true;
                for (int q = 0; q < k; ++q) {
                    const int xf = win + q, xr = win + k - 1 - q;
                    uint32_t cf = 4u, cr = 4u;
                    if (xf != k - 1) { cf = letter_code(S(xf)); ok = ok && cf < 4u; }
                    if (xr != k - 1) cr = letter_code(S(xr));
                    f = rotl1(f) ^ (cf < 4u ? seed_of(cf) : 0ull);
                    r = rotl1(r) ^ (cr < 4u ? seed_of(3u - cr) : 0ull);
                }
                uint64_t h[4];
#pragma unroll
                for (uint32_t b = 0; b < 4u; ++b) {
                    const uint64_t nf = f ^ rotl_var(seed_of(b), (uint32_t)win), nr = r ^ rotl_var(seed_of(3u - b), (uint32_t)(k - 1 - win));
                    h[b] = a.stranded ? nf : canonical(nf, nr);
                }
                uint32_t cd[4];
                count_lookup4(a.fv, h, [&](uint32_t b, bool in, uint32_t mn) { cd[b] = in ? 1u + mn : 0u; });
#pragma unroll
                for (int b = 0; b < 4; ++b) snv[b][win] = (uint8_t)(ok ? cd[b] : 0u);
            }
            LW_FENCE_LDS();
            // the variants: the alternatives of the last bad k-mer's first letter whose k-mer (the candidate's last window) has count >= min_cov;
            // that window is one of the k whose minimum is tested, so the alternatives' mask and the minimum decide
            const uint32_t alts = alt_mask(tx[e - 1]);
            float best = 0.0f;                                                  // Float.MIN_VALUE: medians are multiples of 0.5
            int besta = -1;
            for (int b = 0; b < 4; ++b) {
                if (!((alts >> b) & 1u)) continue;
                const uint8_t *cb = snv[b];
                if (count_code_value(min_code([&](int p) -> uint32_t { return cb[p]; }, 0, k, lane)) < a.min_cov) continue;
                const float med = median_code([&](int p) -> uint32_t { return cb[p]; }, k, lane);
                if (med > best) { best = med; besta = b; }
            }
            if (besta >= 0 && best >= a.min_cov) {
                if (m + k > cap) { outgrown = true; break; }
                for (int x = (int)lane; x < k; x += 64) { out[m + x] = x == 0 ? code_letter((uint32_t)besta) : tx[e + x - 1]; C2[m + x] = snv[besta][x]; }
                m += k;
                wave_fence();
                corrected = true;
                ++ctr[C_SNV_REPLACED];
            } else { append_orig(rs, e); ++ctr[C_SNV_KEPT]; }
            LW_FENCE_LDS();
        } else if (run < k - 1 - a.max_indel) {                                 // :3468-3471: the good k-mer joins the run
            ++ctr[C_SHORT];
            i = e + 1;
            continue;
        } else {                                                                // ---- a path (:3472-3571)
            const int last = m - 1;
            int bl = last, br = e;
            // both scans let a strictly greater count take over, so each ends at the largest count's entry nearest to where it started: 64
            // entries a step, a lane each, the key (code, nearness) reduced over the wavefront
            {
                uint32_t bc = C2[bl];
                const int stop = max(0, last - a.lookahead);
                for (int hi = last - 2; hi >= stop; hi -= 64) {
                    const int j = hi - (int)lane;
                    const uint32_t key = lw_max_key(j >= stop ? C2[j] : 0u, lane);
                    if ((key >> 6) > bc) { bc = key >> 6; bl = hi - (int)(63u - (key & 63u)); }
                }
                bc = c[br];
                const int stop_r = min(e + a.lookahead, n - 1);
                for (int lo = e + 1; lo <= stop_r; lo += 64) {
                    const int j = lo + (int)lane;
                    const uint32_t key = lw_max_key(j <= stop_r ? c[j] : 0u, lane);
                    if ((key >> 6) > bc) { bc = key >> 6; br = lo + (int)(63u - (key & 63u)); }
                }
            }
            if (bl != last || br != e) ++ctr[C_ANCHOR];
            const int bound = run + a.maxld;
            // L = slot[bl .. bl + k), R = tx[br .. br + k): both have a count above 0 and so letters of ACGTU only
            for (int q = (int)lane; q < k; q += 64) { WL.T[q] = (uint8_t)(letter_code(slot[bl + q]) & 3u); WR.T[q] = (uint8_t)(letter_code(tx[br + k - 1 - q]) & 3u); }
            wave_fence();
            // form 0: null; 1: the walk to the right arrived, the path is its nl k-mers; 2: the walk back met entry idx of it, the path is entries
            // 0 .. idx and the nr k-mers of the walk back; 3: the walk back arrived, the path is its nr k-mers
            int form = 0, nl = 0, nr = 0, idx = 0, plen = 0;
            {
                const WaveDir<> dl = wave_dir(a.stranded, k, 0), drr = wave_dir(a.stranded, k, 1);
                int met = -1;
                const int endl = lw_walk(a, dl, WL, bound, [&](int q) -> uint8_t { return WR.T[k - 1 - q]; }, nullptr, 0, nl, met, lane);
                if (endl == LW_END_TARGET) { form = 1; plen = nl; }
                else {
                    const int endr = lw_walk(a, drr, WR, bound, [&](int q) -> uint8_t { return WL.T[k - 1 - q]; }, &WL, nl, nr, met, lane);
                    if (endr == LW_END_TARGET) { form = 3; plen = nr; }
                    else if (endr == LW_END_MET) {
                        const uint8_t *cand = WR.T + nr + 1;                    // the k-mer met, in the walk back's order
                        if (!ce_low_complexity([&](int q) -> uint32_t { return code_letter(cand[k - 1 - q]); }, k, lane)) { form = 2; idx = met; plen = idx + 1 + nr; }
                    }
                }
            }
            const int mm = nr - 1 + (form == 2 ? 1 : 0);                        // letter x behind the joint / of form 3 is WR.T[mm + ...] (below)
            // the path's k-mer x: its last letter and its count code
            auto p_letter = [&](int x) -> uint8_t {
                return code_letter(form == 1 ? WL.T[x + k] : form == 2 ? (x <= idx ? WL.T[x + k] : WR.T[mm + 1 + idx - x]) : WR.T[mm + 1 - x]);
            };
            auto p_code = [&](int x) -> uint32_t { return form == 1 ? WL.C[x] : form == 2 ? (x <= idx ? WL.C[x] : WR.C[mm + idx - x]) : WR.C[mm - x]; };
            bool accept = false;
            if (form == 0 || plen == 0) ++ctr[C_PATH_NONE];                     // :3506
            else {
                const int ladj = last - bl, radj = br - e, ori_len = run + ladj + radj;
                const bool len_ok = abs(ori_len - plen) <= a.maxld;
                bool zero = false;
                for (int j0 = rs; j0 < e && !zero; j0 += 64) { const int j = j0 + (int)lane; zero = __ballot(j < e && c[j] == 0) != 0ull; }
                if (zero) { accept = len_ok; ++ctr[accept ? C_ZERO_ACCEPTED : C_ZERO_KEPT]; }      // :3512-3536
                else {
                    const float alt = median_code(p_code, plen, lane);
                    const float ori = median_code([&](int p) -> uint32_t { return c[rs + p]; }, run, lane);
                    if (2.0f * ori <= alt && len_ok) {
                        if (ori < a.min_cov && alt >= 10.0f * ori) { accept = true; ++ctr[C_10X]; }
                        else {
                            const int t0 = e - run - ladj, tlen = ori_len + k - 1, slen = plen + k - 1;       // window k-mers [t0, e + radj)
                            if (t0 >= 0) {
                                // assemble(path): the first k-mer's letters, then a letter per k-mer
                                auto s = [&](int x) -> uint32_t {
                                    return code_letter(form == 1 ? WL.T[1 + x] : form == 2 ? (x < idx + k ? WL.T[1 + x] : WR.T[mm - (x - (idx + k))]) : WR.T[mm + k - x]);
                                };
                                const int d = ce_distance(s, slen, [&](int x) -> uint32_t { return tx[t0 + x]; }, tlen, lev, lane);
                                wave_fence();
                                if (ce_identity(d, slen, tlen) >= a.pid) { accept = true; ++ctr[C_IDENTITY]; }
                            }
                        }
                    }
                    if (!accept) ++ctr[C_COV_KEPT];
                }
            }
            if (accept) {                                                       // back to L, the path, on at R
                m = bl + 1;
                if (m + plen > cap) { outgrown = true; break; }
                for (int x = (int)lane; x < plen; x += 64) { out[m + x] = p_letter(x); C2[m + x] = (uint8_t)p_code(x); }
                m += plen;
                wave_fence();
                corrected = true;
                nxt = br;
            } else append_orig(rs, e);
        }
        if (outgrown) break;
        append_orig(nxt, nxt + 1);
        i = rs = nxt + 1;
    }
    if (!outgrown && rs < n && rs > 0) append_orig(rs, n);                      // :3588-3595 (a run that is the whole window has rs == 0 and m == 0)
    state = outgrown ? LW_OUTGROWN : corrected ? LW_CORRECTED : LW_SAME;
    done();
}

// A wavefront per window, taking windows in turn; its rows are its slot of a.rows
__global__ void __launch_bounds__(LW_TPB) k_long_window(LwArgs a, size_t row_bytes) {
    __shared__ int s_hist[LW_WAVES][132];
    __shared__ uint8_t s_snv[LW_WAVES][4][RB_MAX_K];
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const int64_t slot = (int64_t)blockIdx.x * LW_WAVES + wv, n_slots = (int64_t)gridDim.x * LW_WAVES;
    uint8_t *row = a.rows + (size_t)slot * row_bytes;
    for (int64_t w = slot; w < a.nwin; w += n_slots) {
        lw_window(a, w, row, s_hist[wv], s_snv[wv], lane);
        wave_fence();
    }
}

// ---- stitch: a wavefront per corrected sequence writes its next text: the first k - 1 letters, then every window's letters — its slot's if the
// window was corrected, its own otherwise
__global__ void __launch_bounds__(LW_TPB) k_long_stitch(int k, const LwJoin *__restrict__ joins, int64_t n, const LwWin *__restrict__ win,
                                                        const int32_t *__restrict__ res, const uint8_t *__restrict__ txt, const uint8_t *__restrict__ slots,
                                                        uint8_t *__restrict__ ntxt) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t r = (int64_t)blockIdx.x * LW_WAVES + wv;
    if (r >= n) return;
    const LwJoin jn = joins[r];
    uint8_t *o = ntxt + jn.dst;
    for (int x = (int)lane; x < k - 1; x += 64) o[x] = txt[jn.src + x];
    int64_t at = k - 1;
    for (int32_t w = jn.wfirst; w < jn.wfirst + jn.nwin; ++w) {
        const LwWin wn = win[w];
        const int32_t len = res[(int64_t)w * LW_RES];
        const uint8_t *src = res[(int64_t)w * LW_RES + 1] == LW_CORRECTED ? slots + wn.ooff + (k - 1) : txt + wn.toff + (k - 1);
        for (int32_t x = (int32_t)lane; x < len; x += 64) o[at + x] = src[x];
        at += len;
    }
}

// ---- a sequence leaves: trimLowCoverageEdgeKmers (:3173-3179, :3187-3241) where asked, then its text into the caller's layout if it fits
__global__ void __launch_bounds__(LW_TPB) k_long_finish(int k, const LwFin *__restrict__ fins, int64_t n, const uint8_t *__restrict__ txt,
                                                        const uint8_t *__restrict__ cnt, float min_cov, uint8_t *__restrict__ fin_txt,
                                                        LwOut *__restrict__ outs) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t r = (int64_t)blockIdx.x * LW_WAVES + wv;
    if (r >= n) return;
    const LwFin f = fins[r];
    const uint8_t *c = cnt + f.koff;
    const int nk = f.nk;
    LwOut o{f.len, -1, -1, 0, 0};
    int t0 = 0, tlen = f.len;
    if (f.trim && nk > 0 && median_code([&](int p) -> uint32_t { return c[p]; }, nk, lane) >= 2.0f * min_cov) {
        auto good = [&](int j) { return count_code_value(c[j]) >= min_cov; };
        int head = nk, tail = -1;                                               // the first i with i - 1 and i good; the last i > head with i and i + 1 good
        for (int j = 1 + (int)lane; j < nk; j += 64) if (good(j - 1) && good(j)) { head = j; break; }
        for (int s = 32; s > 0; s >>= 1) head = min(head, __shfl_xor(head, s, 64));
        if (head == nk) head = 0;
        for (int j = head + 1 + (int)lane; j + 1 < nk; j += 64) if (good(j) && good(j + 1)) tail = j;
        for (int s = 32; s > 0; s >>= 1) tail = max(tail, __shfl_xor(tail, s, 64));
        tail = tail < 0 ? nk : tail + 2;
        if (head > 0 || tail < nk) {
            o.trim_begin = head; o.trim_end = tail; o.trimmed = 1;
            if (tail - head > 1) { t0 = head; tlen = tail - head + k - 1; }
            else { tlen = 0; o.flags |= RB_LONG_TRIMMED_TO_NOTHING; }
            o.out_len = tlen;
        }
    }
    if (tlen > f.cap) o.flags |= RB_LONG_OVERFLOW;
    else for (int x = (int)lane; x < tlen; x += 64) fin_txt[f.ooff + x] = txt[f.toff + t0 + x];
    if (lane == 0) outs[f.id] = o;
}

// the windows of a list of nk k-mers (:3124-3135)
template <class F> void cut_windows(int64_t nk, int window, bool to_shift, F &&f) {
    const int64_t shift = window / 2;
    int64_t end = 0;
    for (int64_t i = 0; i < nk; i = end) {
        end = std::min<int64_t>(i + window + (i == 0 && to_shift ? shift : 0), nk);
        if (end + shift >= nk) end = nk;
        f(i, end);
    }
}

void long_call(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, const rb_long_params *p, const int64_t *out_offsets, char *out_seq,
               rb_long_rec *recs) {
    const char *who = "rb_graph_correct_long";
    RB_REQUIRE(g && p, "%s: null argument", who);
    RB_REQUIRE(!g->shard, "%s: not available on a shard handle", who);
    RB_REQUIRE(g->dbg.bits && g->cbf, "%s: dbgbf or the counting filter has been destroyed", who);
    const int k = g->k;
    RB_REQUIRE(k >= 2, "%s: k = %d (an SNV bubble is a run of k - 1 >= 1 k-mers)", who, k);
    RB_REQUIRE(std::isfinite(p->max_cov_gradient) && std::isfinite(p->percent_identity), "%s: max_cov_gradient and percent_identity must be finite", who);
    RB_REQUIRE(p->window_size >= 1 && p->window_size <= RB_LONG_MAX_WINDOW, "%s: window_size = %d (1 .. %d)", who, p->window_size, RB_LONG_MAX_WINDOW);
    RB_REQUIRE(p->lookahead >= 1 && p->lookahead <= RB_LONG_MAX_WINDOW, "%s: lookahead = %d (1 .. %d)", who, p->lookahead, RB_LONG_MAX_WINDOW);
    RB_REQUIRE(p->max_itr >= 0, "%s: max_itr = %d", who, p->max_itr);
    RB_REQUIRE(p->max_indel_size >= 0 && p->max_indel_size <= LW_MAX_INDEL, "%s: max_indel_size out of range [0, %d]", who, LW_MAX_INDEL);
    // a window has up to 2 window_size k-mers (the first of a shifted pass, merged with the rest) and its slot len + (len / 2) * max(max_indel_size, 1)
    RB_REQUIRE((int64_t)p->window_size * (2 + std::max(p->max_indel_size, 1)) <= LW_MAX_SLOT,
               "%s: window_size * (2 + max(max_indel_size, 1)) = %lld: a window's slot would hold more than 2^30 k-mers", who,
               (long long)p->window_size * (2 + std::max(p->max_indel_size, 1)));
    RB_REQUIRE(n >= 0, "%s: n = %lld", who, (long long)n);
    if (n == 0) return;
    RB_REQUIRE(offsets && out_offsets && out_seq && recs, "%s: null argument", who);
    std::vector<int64_t> ko((size_t)n + 1);
    kmer_offsets(offsets, n, k, ko.data(), who);
    for (int64_t i = 0; i < n; ++i) RB_REQUIRE(out_offsets[i + 1] >= out_offsets[i], "%s: out_offsets[%lld] > out_offsets[%lld]", who, (long long)i, (long long)i + 1);
    RB_REQUIRE(offsets[n] == offsets[0] || seq, "%s: null sequence text", who);
    const int window = p->window_size, lookahead = p->lookahead, max_indel = p->max_indel_size, grow = std::max(max_indel, 1);
    const float min_cov = (float)p->min_kmer_cov;
    // what no kernel touches: the sequences without a k-mer come back as they went in
    for (int64_t i = 0; i < n; ++i) {
        rb_long_rec &rc = recs[i];
        memset(&rc, 0, sizeof rc);
        rc.trim_begin = rc.trim_end = -1;
        if (ko[(size_t)i + 1] > ko[(size_t)i]) continue;
        const int64_t l = offsets[i + 1] - offsets[i];
        rc.status = RB_LONG_NO_KMER; rc.out_len = (int32_t)l;
        if (l > out_offsets[i + 1] - out_offsets[i]) rc.flags |= RB_LONG_OVERFLOW;
        else if (l) memmove(out_seq + out_offsets[i], seq + offsets[i], (size_t)l);
    }
    if (ko[(size_t)n] == 0) return;
    RB_HIP(hipSetDevice(g->p.device));
    QueryLease q(g);
    RB_REQUIRE(g->dbg.bits && g->cbf, "%s: dbgbf or the counting filter has been destroyed", who);
    hipStream_t s = q.c->st;
    const FilterView fv = g->view(0, 0);
    // The call's own buffers (a context's four are one piece's tables in the other calls; here every pass lays out anew): text and counts twice
    // — a pass reads one pair and writes the other —, the tables of a pass, the windows' slots and results, the wavefronts' rows, the final texts
    // and records.  A buffer that has to grow is freed first, and hipFree waits for the device, so no kernel in flight loses what it reads.
    DevBuf b_txt[2], b_cnt[2], b_tab, b_slots, b_res, b_rows, b_fin, b_out;
    std::vector<LwSeq> live, next;
    std::vector<int64_t> ids, next_ids;           // the piece's sequence behind each live entry
    std::vector<LwWin> wins;
    std::vector<LwJoin> joins;
    std::vector<LwFin> fins;
    std::vector<int32_t> res, nsolid, wfirst;
    std::vector<LwOut> outs;
    std::vector<uint8_t> tab;
    // piece by piece (rb_pieces.hpp), 4 M k-mers a piece; with profiling on every piece's passes are timed as one interval: entry "correct_long"
    for_each_piece(g, s, [&](int64_t i) { return ko[(size_t)i]; }, n, (int64_t)4 << 20, "correct_long", [&](Piece &pc) {
        const int64_t ra = pc.ra, rb_ = pc.rb, pn = pc.pn, pt = ko[(size_t)rb_] - ko[(size_t)ra];
        if (pt == 0) return;
        const int64_t tb = offsets[rb_] - offsets[ra], ob = out_offsets[rb_] - out_offsets[ra];
        b_txt[0].reserve((size_t)tb + 16); b_cnt[0].reserve((size_t)pt + 16);
        b_fin.reserve((size_t)ob + 16); b_out.reserve((size_t)pn * sizeof(LwOut) + 16);
        outs.assign((size_t)pn, LwOut{0, -1, -1, 0, 0});
        int cur = 0;
        // the tables of a step go up in one copy: tab is laid out on the host, b_tab holds it
        auto upload = [&](const void *a0, size_t n0, const void *a1, size_t n1, const void *a2, size_t n2, size_t &o1, size_t &o2) {
            o1 = up16(n0); o2 = up16(o1 + n1);
            tab.assign(up16(o2 + n2) + 16, 0);
            if (n0) memcpy(tab.data(), a0, n0);
            if (n1) memcpy(tab.data() + o1, a1, n1);
            if (n2) memcpy(tab.data() + o2, a2, n2);
            RB_HIP(hipStreamSynchronize(s));               // (the kernels of the step before read the table that is about to be overwritten)
            b_tab.reserve(tab.size());
            RB_HIP(hipMemcpyAsync(b_tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice, s));
            RB_HIP(hipStreamSynchronize(s));               // (tab is pageable and reused)
        };
        size_t o1 = 0, o2 = 0;
        live.clear(); ids.clear();
        for (int64_t i = 0; i < pn; ++i) {
            const int64_t nk = ko[(size_t)(ra + i + 1)] - ko[(size_t)(ra + i)];
            if (nk == 0) continue;
            live.push_back(LwSeq{offsets[ra + i] - offsets[ra], ko[(size_t)(ra + i)] - ko[(size_t)ra], (int32_t)(offsets[ra + i + 1] - offsets[ra + i]), (int32_t)nk});
            ids.push_back(i);
        }
        RB_HIP(hipMemcpyAsync(b_txt[0].p, seq + offsets[ra], (size_t)tb, hipMemcpyHostToDevice, s));
        upload(live.data(), live.size() * sizeof(LwSeq), nullptr, 0, nullptr, 0, o1, o2);
        pc.kernels_begin();
        int64_t nl = (int64_t)live.size();
        hipLaunchKernelGGL(k_long_profile, dim3(blocks_for(nl, LW_WAVES)), dim3(LW_TPB), 0, s, fv, (int)g->stranded, k, reinterpret_cast<const LwSeq *>(b_tab.p), nl,
                           b_txt[0].as<uint8_t>(), b_cnt[0].as<uint8_t>());
        RB_HIP(hipGetLastError());
        // a sequence leaves: those of `which` (indices into live) with the buffers they are in
        auto finish = [&](const std::vector<int64_t> &which, bool screened_out) {
            if (which.empty()) return;
            fins.clear();
            for (int64_t li : which) {
                const LwSeq &sq = live[(size_t)li];
                const int64_t id = ids[(size_t)li];
                fins.push_back(LwFin{sq.toff, sq.koff, out_offsets[ra + id] - out_offsets[ra], sq.len, sq.nk,
                                     (int32_t)std::min<int64_t>(INT32_MAX, out_offsets[ra + id + 1] - out_offsets[ra + id]),
                                     !screened_out && p->trim_low_cov_edges ? 1 : 0, (int32_t)id});
                recs[ra + id].status = screened_out ? RB_LONG_NULL : RB_LONG_UNCHANGED;
            }
            size_t x1, x2;
            upload(fins.data(), fins.size() * sizeof(LwFin), nullptr, 0, nullptr, 0, x1, x2);
            hipLaunchKernelGGL(k_long_finish, dim3(blocks_for((int64_t)fins.size(), LW_WAVES)), dim3(LW_TPB), 0, s, k, reinterpret_cast<const LwFin *>(b_tab.p),
                               (int64_t)fins.size(), b_txt[cur].as<uint8_t>(), b_cnt[cur].as<uint8_t>(), min_cov, b_fin.as<uint8_t>(), b_out.as<LwOut>());
            RB_HIP(hipGetLastError());
        };
        std::vector<int64_t> leaving;
        if (p->min_num_solid > 0) {                          // the screen (:3099-3110)
            b_res.reserve((size_t)nl * 4 + 16);
            hipLaunchKernelGGL(k_long_solid, dim3(blocks_for(nl, LW_WAVES)), dim3(LW_TPB), 0, s, reinterpret_cast<const LwSeq *>(b_tab.p), nl, b_cnt[0].as<uint8_t>(),
                               min_cov, b_res.as<int32_t>());
            RB_HIP(hipGetLastError());
            nsolid.resize((size_t)nl);
            RB_HIP(hipMemcpyAsync(nsolid.data(), b_res.p, (size_t)nl * 4, hipMemcpyDeviceToHost, s));
            RB_HIP(hipStreamSynchronize(s));
            next.clear(); next_ids.clear();
            for (int64_t li = 0; li < nl; ++li) {
                if (nsolid[(size_t)li] < p->min_num_solid) leaving.push_back(li);
                else { next.push_back(live[(size_t)li]); next_ids.push_back(ids[(size_t)li]); }
            }
            finish(leaving, true);
            live.swap(next); ids.swap(next_ids);
        }
        bool to_shift = false;
        for (int itr = 0; itr < p->max_itr && !live.empty(); ++itr) {
            nl = (int64_t)live.size();
            // 1. the windows, their slots, the rows of the longest of them
            wins.clear(); wfirst.assign((size_t)nl + 1, 0);
            int64_t slot_bytes = 0, W = 0, capmax = 0;
            for (int64_t li = 0; li < nl; ++li) {
                const LwSeq &sq = live[(size_t)li];
                cut_windows(sq.nk, window, to_shift, [&](int64_t a, int64_t e) {
                    const int64_t len = e - a, cap = len + (len / 2) * grow;
                    wins.push_back(LwWin{sq.toff + a, sq.koff + a, slot_bytes, (int32_t)len, (int32_t)cap});
                    slot_bytes += up16((size_t)(cap + k - 1));
                    W = std::max(W, len); capmax = std::max(capmax, cap);
                });
                wfirst[(size_t)li + 1] = (int32_t)wins.size();
            }
            const int64_t nw = (int64_t)wins.size(), B = W + max_indel;
            if (nw >= INT32_MAX) {                               // (capmax <= LW_MAX_SLOT by the check of the arguments)
                set_error("%s: a pass over sequences [%lld, %lld) has %lld windows, more than an int holds: use smaller pieces", who, (long long)ra, (long long)rb_, (long long)nw);
                throw HipError{RB_ERR_STATE};
            }
            const LwLayout lay(capmax, B, W, k);
            const int64_t slots_n = std::min(nw, LW_MAX_SLOTS);
            const unsigned blocks = blocks_for(slots_n, LW_WAVES);
            upload(wins.data(), wins.size() * sizeof(LwWin), nullptr, 0, nullptr, 0, o1, o2);
            b_slots.reserve((size_t)slot_bytes + 16);
            b_res.reserve((size_t)nw * LW_RES * 4 + 16);
            b_rows.reserve((size_t)blocks * LW_WAVES * lay.bytes + 16);
            LwArgs a;
            a.fv = fv; a.stranded = (int)g->stranded; a.k = k; a.lookahead = lookahead; a.max_indel = max_indel;
            a.maxld = p->percent_identity < 1.0f ? max_indel : 0;
            a.grad = p->max_cov_gradient; a.pid = p->percent_identity; a.min_cov = min_cov;
            a.txt = b_txt[cur].as<uint8_t>(); a.cnt = b_cnt[cur].as<uint8_t>();
            a.win = reinterpret_cast<const LwWin *>(b_tab.p); a.nwin = nw;
            a.slots = b_slots.as<uint8_t>(); a.res = b_res.as<int32_t>(); a.rows = b_rows.as<uint8_t>();
            a.capmax = capmax; a.B = B; a.W = W;
            // 2. one launch over the windows
            hipLaunchKernelGGL(k_long_window, dim3(blocks), dim3(LW_TPB), 0, s, a, lay.bytes);
            RB_HIP(hipGetLastError());
            res.resize((size_t)nw * LW_RES);
            RB_HIP(hipMemcpyAsync(res.data(), b_res.p, res.size() * 4, hipMemcpyDeviceToHost, s));
            RB_HIP(hipStreamSynchronize(s));
            // 3. who corrected: their next texts; who did not leaves
            leaving.clear(); next.clear(); next_ids.clear(); joins.clear();
            int64_t ntb = 0, npt = 0;
            bool any = false;
            for (int64_t li = 0; li < nl; ++li) {
                const LwSeq &sq = live[(size_t)li];
                rb_long_rec &rc = recs[ra + ids[(size_t)li]];
                bool corrected = false;
                int64_t nk2 = 0;
                for (int32_t w = wfirst[(size_t)li]; w < wfirst[(size_t)li + 1]; ++w) {
                    const int32_t *r = res.data() + (size_t)w * LW_RES;
                    if (r[1] == LW_OUTGROWN) {
                        set_error("%s: a window of sequence %lld outgrew its slot (internal error)", who, (long long)(ra + ids[(size_t)li]));
                        throw HipError{RB_ERR_STATE};
                    }
                    corrected = corrected || r[1] == LW_CORRECTED;
                    nk2 += r[0];
                    int32_t *ct = &rc.snv_replaced;
                    for (int c = 0; c < LW_NCTR; ++c) ct[c] += r[2 + c];
                }
                if (!corrected) { leaving.push_back(li); continue; }
                any = true;
                ++rc.passes;
                if (nk2 + k - 1 > INT32_MAX / 2) {
                    set_error("%s: sequence %lld grew beyond 2^30 letters", who, (long long)(ra + ids[(size_t)li]));
                    throw HipError{RB_ERR_STATE};
                }
                joins.push_back(LwJoin{sq.toff, ntb, wfirst[(size_t)li], wfirst[(size_t)li + 1] - wfirst[(size_t)li]});
                next.push_back(LwSeq{ntb, npt, (int32_t)(nk2 + k - 1), (int32_t)nk2});
                next_ids.push_back(ids[(size_t)li]);
                ntb += nk2 + k - 1; npt += nk2;
            }
            finish(leaving, false);
            if (!any) { live.clear(); break; }
            const int nxt = cur ^ 1;
            const int64_t nj = (int64_t)joins.size();
            upload(joins.data(), joins.size() * sizeof(LwJoin), wins.data(), wins.size() * sizeof(LwWin), next.data(), next.size() * sizeof(LwSeq), o1, o2);
            b_txt[nxt].reserve((size_t)ntb + 16); b_cnt[nxt].reserve((size_t)npt + 16);
            const uint8_t *tb8 = b_tab.as<uint8_t>();
            hipLaunchKernelGGL(k_long_stitch, dim3(blocks_for(nj, LW_WAVES)), dim3(LW_TPB), 0, s, k, reinterpret_cast<const LwJoin *>(tb8), nj,
                               reinterpret_cast<const LwWin *>(tb8 + o1), b_res.as<int32_t>(), b_txt[cur].as<uint8_t>(), b_slots.as<uint8_t>(), b_txt[nxt].as<uint8_t>());
            RB_HIP(hipGetLastError());
            // 4. the counts of the new texts
            hipLaunchKernelGGL(k_long_profile, dim3(blocks_for(nj, LW_WAVES)), dim3(LW_TPB), 0, s, fv, (int)g->stranded, k, reinterpret_cast<const LwSeq *>(tb8 + o2), nj,
                               b_txt[nxt].as<uint8_t>(), b_cnt[nxt].as<uint8_t>());
            RB_HIP(hipGetLastError());
            cur = nxt;
            live.swap(next); ids.swap(next_ids);
            to_shift = !to_shift;
        }
        if (!live.empty()) {                                 // max_itr passes are over (or there were none)
            leaving.resize(live.size());
            for (size_t li = 0; li < live.size(); ++li) leaving[li] = (int64_t)li;
            finish(leaving, false);
        }
        pc.kernels_end();
        // only the final copy crosses to the host
        std::vector<uint8_t> fin_host((size_t)ob);
        RB_HIP(hipMemcpyAsync(outs.data(), b_out.p, (size_t)pn * sizeof(LwOut), hipMemcpyDeviceToHost, s));
        if (ob) RB_HIP(hipMemcpyAsync(fin_host.data(), b_fin.p, (size_t)ob, hipMemcpyDeviceToHost, s));
        pc.finish();                                        // (outs and fin_host are on the host)
        for (int64_t i = 0; i < pn; ++i) {
            rb_long_rec &rc = recs[ra + i];
            if (rc.status == RB_LONG_NO_KMER) continue;
            const LwOut &o = outs[(size_t)i];
            rc.out_len = o.out_len; rc.trim_begin = o.trim_begin; rc.trim_end = o.trim_end; rc.flags = o.flags;
            if (rc.status == RB_LONG_UNCHANGED && (rc.passes > 0 || o.trimmed)) rc.status = RB_LONG_CHANGED;
            if (!(o.flags & RB_LONG_OVERFLOW) && o.out_len > 0)
                memcpy(out_seq + out_offsets[ra + i], fin_host.data() + (out_offsets[ra + i] - out_offsets[ra]), (size_t)o.out_len);
        }
    });
}

}  // namespace

extern "C" {
int rb_graph_correct_long(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, const rb_long_params *p, const int64_t *out_offsets,
                          char *out_seq, rb_long_rec *recs) {
    return guarded([&] { long_call(g, seq, offsets, n, p, out_offsets, out_seq, recs); });
}
}  // extern "C"
