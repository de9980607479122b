// rb_overlap.hip — overlap of read pairs (rb_graph_overlap_pairs): GraphUtils.overlap (R/util/GraphUtils.java:4898-5063) over
// SeqUtils.overlapMaximally (R/util/SeqUtils.java:1335-1379), the first half of overlapAndConnect, on the device.  A wavefront per pair:
// both reads are staged as bytes in LDS (exact-byte comparison: no 2-bit packing), a lane per shift looks for the smallest shift at
// which the reads agree over the extent they share, and the rest is decided from the overlap's length: no graph look-up when it is at
// least k, the k - 1 - o spanning windows of the joined text (and, where those fail, the reads' edge windows) when it is shorter.
// Nothing is written to the graph; the pairs the reference would rescue are reported (DESIGN.md §5 "Overlap of read pairs").
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rb_pieces.hpp"
#include "rb_lookup.hpp"
#include "rb_wave.hpp"

using namespace rb;

// Java float arithmetic: isRepeat's thresholds are one float32 product each
#pragma clang fp contract(off)

namespace {

constexpr int OV_TPB = 256;
constexpr int OV_WAVES = OV_TPB / 64;    // pairs per workgroup: a wavefront each
constexpr int OV_LDS_ROW = 1024;         // bytes of LDS a pair's two reads may take (the right read starts at a multiple of 4); longer pairs are read from device memory

__host__ __device__ inline int64_t ov_right_at(int64_t ll) { return (ll + 3) & ~(int64_t)3; }
__host__ __device__ inline bool ov_fits_lds(int64_t ll, int64_t rl) { return ov_right_at(ll) + rl <= OV_LDS_ROW; }

// SeqUtils.nucleotideArrayIndex(int) :315-330: upper case only, U as T, -1 for everything else
__device__ __forceinline__ int ov_nt_index(uint32_t ch) {
    switch (ch) {
        case 'A': return 0;
        case 'C': return 1;
        case 'G': return 2;
        case 'T': case 'U': return 3;
        default: return -1;
    }
}

// two reads, and the text overlapped = a + b[o ..] they spell when the last o bytes of a are the first o of b
struct OvText {
    const uint8_t *a, *b;
    int la, o;
    __device__ __forceinline__ uint32_t operator()(int p) const { return p < la ? a[p] : b[p - la + o]; }
};
struct OvRead {
    const uint8_t *a;
    __device__ __forceinline__ uint32_t operator()(int p) const { return a[p]; }
};

// overlapMaximally's loop (:1343-1368) and both `contains` (:1370-1376) in one form: the smallest shift s in [0, max_shift] at which b agrees
// with a over the extent they share, a[s, min(s + bl, al)) == b[0, ...), or -1.  Lane j owns shift base + j, compares four bytes at a time and
// gives up at the first difference; a ballot picks the lowest passing lane.  Reads stay inside [a, a + al) and [b, b + bl).
__device__ int ov_match(const uint8_t *a, int al, const uint8_t *b, int bl, int max_shift, uint32_t lane) {
    for (int base = 0; base <= max_shift; base += 64) {
        const int s = base + (int)lane;
        bool ok = s <= max_shift;
        if (ok) {
            const int e = min(bl, al - s);
            int i = 0;
            for (; ok && i + 4 <= e; i += 4) {
                uint32_t x, y;
                __builtin_memcpy(&x, &a[s + i], 4);
                __builtin_memcpy(&y, &b[i], 4);
                ok = x == y;
            }
            for (; ok && i < e; ++i) ok = a[s + i] == b[i];
        }
        const unsigned long long m = __ballot(ok);
        if (m) return base + (int)__builtin_ctzll(m);
    }
    return -1;
}

// the getKmers count of the window of k letters at w of text t (0 where a letter is outside ACGTU, else graph.getCount of its hash:
// BloomFilterDeBruijnGraph.java:562-570), and whether its k bytes are all equal (SeqUtils.isHomopolymer(byte[]) :354-368).  Both strands are
// rolled one letter a step (rotations by one only).
template <typename T> __device__ float ov_window_count(const FilterView &fv, int stranded, int k, const T &t, int w, bool &homo) {
    uint64_t f = 0, r = 0;
    bool ok = true;
    const uint32_t c0 = t(w);
    homo = true;
    for (int j = 0; j < k; ++j) {
        const uint32_t c = t(w + j);
        const uint64_t s = letter_seed(c);                 // (0 for a letter outside ACGTU, and for no other)
        f = rotl(f, 1) ^ s;
        if (!stranded) r = rotl(r, 1) ^ letter_rev_seed(t(w + k - 1 - j));
        ok = ok && s != 0ull;
        homo = homo && c == c0;
    }
    if (!ok) return 0.0f;
    const uint64_t h = stranded ? f : canonical(f, r);
    return count_value(fv, h);
}

// does one of the windows [w0, w1) of t have count == 1?  A lane per window.
template <typename T> __device__ bool ov_any_singleton(const FilterView &fv, int stranded, int k, const T &t, int w0, int w1, uint32_t lane) {
    bool any = false;
    for (int base = w0; base < w1; base += 64) {
        const int w = base + (int)lane;
        bool homo;
        any = any || (w < w1 && ov_window_count(fv, stranded, k, t, w, homo) == 1.0f);
    }
    return __ballot(any) != 0ull;
}

// SeqUtils.isRepeat(String) :417-456 of b[0, n): 0 no, 1 yes, 2 the reference throws (nucleotideArrayIndex gives -1 and indexes an array).  The
// reference's loops run as they stand, one after the other with their early returns, the whole wavefront in step: lane c keeps the
// counter of base / dinucleotide / trinucleotide c, a signed byte as in the reference (it wraps at 128), and a ballot sees a threshold reached.
__device__ int ov_is_repeat(const uint8_t *b, int n, uint32_t lane) {
    const float thr = 0.9f;
    const int t[3] = {(int)java_round((float)n * thr), (int)java_round((float)(n / 2) * thr), (int)java_round((float)(n / 3) * thr)};
    for (int m = 1; m <= 3; ++m)                         // m letters a unit
        for (int start = 0; start < m; ++start) {
            int8_t cnt = 0;
            for (int i = start; i < n - (m - 1); i += m) {
                int idx = 0;
                for (int j = 0; j < m; ++j) {
                    const int c = ov_nt_index(b[i + j]);
                    if (c < 0) return 2;
                    idx = idx * 4 + c;
                }
                if ((int)lane == idx) cnt = (int8_t)(cnt + 1);
                if (__ballot((int)lane == idx && (int)cnt >= t[m - 1])) return 1;
            }
        }
    return 0;
}

__device__ __forceinline__ void ov_put(rb_overlap_rec *rec, int outcome, int why, uint32_t flags, int overlap, int out_len, int span_first, int span_n) {
    rb_overlap_rec v;
    v.outcome = outcome; v.why = why; v.flags = flags; v.overlap = overlap; v.out_len = out_len; v.span_first = span_first; v.span_n = span_n; v.pad = 0;
    *rec = v;
}

// A wavefront per pair: pair r of the piece is ltx[lof[r], lof[r + 1]) and rtx[rof[r], rof[r + 1]); its record goes to recs[r] and its text to
// out[lof[r] + rof[r] ...] (room for both reads).  LDS_ROW: workgroup b takes pairs 4 b .. 4 b + 3, both reads of each in LDS, and leaves the
// pairs that do not fit OV_LDS_ROW to the other instantiation, which takes the pairs listed in ids and reads them where they are.
template <bool LDS_ROW>
__global__ void __launch_bounds__(OV_TPB) k_overlap(FilterView fv, int stranded, int k, int min_overlap, float min_cov, int64_t pn,
                                                    const int64_t *__restrict__ ids, int64_t n_ids, const int64_t *__restrict__ lof,
                                                    const int64_t *__restrict__ rof, const uint8_t *__restrict__ ltx, const uint8_t *__restrict__ rtx,
                                                    uint8_t *__restrict__ out, rb_overlap_rec *__restrict__ recs) {
    __shared__ __attribute__((aligned(16))) uint8_t s_row[OV_WAVES][LDS_ROW ? OV_LDS_ROW : 16];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t slot = (int64_t)blockIdx.x * OV_WAVES + wv;
    int64_t r;
    if constexpr (LDS_ROW) { if (slot >= pn) return; r = slot; }
    else { if (slot >= n_ids) return; r = ids[slot]; }
    const int64_t l0 = lof[r], r0 = rof[r];
    const int ll = (int)(lof[r + 1] - l0), rl = (int)(rof[r + 1] - r0);
    if (LDS_ROW != ov_fits_lds(ll, rl)) return;
    rb_overlap_rec *rec = recs + r;
    if (min(ll, rl) < max(k, min_overlap)) {
        if (lane == 0) ov_put(rec, RB_OVL_NONE, RB_OVL_WHY_SHORT, 0u, 0, 0, 0, 0);
        return;
    }
    const uint8_t *L, *R;
    if constexpr (LDS_ROW) {
        uint8_t *row = s_row[wv];
        const int ra = (int)ov_right_at(ll);
        for (int p = (int)lane; p < ll; p += 64) row[p] = ltx[l0 + p];
        for (int p = (int)lane; p < rl; p += 64) row[ra + p] = rtx[r0 + p];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        L = row; R = row + ra;
    } else { L = ltx + l0; R = rtx + r0; }
    uint8_t *o_txt = out + l0 + r0;

    // overlapMaximally(left, right, minOverlap), then the dovetail attempt with the roles exchanged (:4901-4923)
    const uint8_t *A = L, *B = R;
    int la = ll, lb = rl;
    uint32_t flags = 0;
    bool b_holds_a = false;                               // overlapped = b through `right.contains(left)` (:1374)
    int s = ov_match(A, la, B, lb, la - min_overlap, lane);
    if (s < 0 && la < lb) {
        b_holds_a = ov_match(B, lb, A, la, lb - la, lane) >= 0;
    }
    if (s < 0 && !b_holds_a) {
        const int mo2 = max(min_overlap, min(ll, rl) * 3 / 4);
        s = ov_match(R, rl, L, ll, rl - mo2, lane);
        if (s < 0) {                                      // (the swapped call's two `contains` would have been hits of the first call)
            if (lane == 0) ov_put(rec, RB_OVL_NONE, RB_OVL_WHY_NO_MATCH, 0u, 0, 0, 0, 0);
            return;
        }
        A = R; B = L; la = rl; lb = ll; flags = RB_OVL_SWAPPED;
    }
    // |overlapped| and the bases overlapped
    const int len = b_holds_a ? lb : (s + lb < la ? la : s + lb);
    const int o = la + lb - len;
    if (o >= k) {
        if (len == max(la, lb)) {                         // :4935-4944: the longer read's k-mers
            const bool left = la >= lb;
            const uint8_t *src = left ? A : B;
            for (int p = (int)lane; p < len; p += 64) o_txt[p] = src[p];
            if (lane == 0) ov_put(rec, left ? RB_OVL_LEFT : RB_OVL_RIGHT, RB_OVL_WHY_FOUND, flags, o, len, 0, 0);
            return;
        }
        // :4946-4960: right's k-mers 0 .. o - k are all homopolymers iff right[0, o) is one letter (k >= 2; every 1-mer is one)
        bool same = true;
        if (k > 1) {
            const uint32_t c0 = B[0];
            for (int p = (int)lane; p < o; p += 64) same = same && B[p] == c0;
        }
        if (__ballot(!same) == 0ull) {
            if (lane == 0) ov_put(rec, RB_OVL_NONE, RB_OVL_WHY_NO_COMPLEX, flags, o, 0, 0, 0);
            return;
        }
        const OvText t{A, B, la, o};
        for (int p = (int)lane; p < len; p += 64) o_txt[p] = (uint8_t)t(p);
        if (lane == 0) ov_put(rec, RB_OVL_MERGED, RB_OVL_WHY_FOUND, flags, o, len, 0, 0);
        return;
    }
    // the overlap is smaller than k (:4974-5059): windows la - k + 1 .. la - o - 1 of overlapped span it
    const OvText t{A, B, la, o};
    const int sp0 = la - k + 1, sn = k - 1 - o;
    int first_bad = sn;                                   // index of the first spanning k-mer below min_cov
    bool complex_any = false;                             // a spanning k-mer before it that is no homopolymer
    for (int base = 0; base < sn && first_bad == sn; base += 64) {
        const int i = base + (int)lane;
        bool homo = true, bad = false;
        if (i < sn) bad = ov_window_count(fv, stranded, k, t, sp0 + i, homo) < min_cov;
        const unsigned long long mb = __ballot(bad);
        if (mb) first_bad = base + (int)__builtin_ctzll(mb);
        complex_any = complex_any || __ballot(i < min(sn, first_bad) && !homo) != 0ull;
    }
    if (first_bad < sn) {
        const int nka = la - k + 1, nkb = lb - k + 1;
        int why = RB_OVL_WHY_FOUND;
        if (!ov_any_singleton(fv, stranded, k, OvRead{B}, 0, min(o, nkb), lane)) why = RB_OVL_WHY_NO_RIGHT_SINGLETON;
        else if (!ov_any_singleton(fv, stranded, k, OvRead{A}, max(0, nka - o), nka, lane)) why = RB_OVL_WHY_NO_LEFT_SINGLETON;
        else {
            const int rep = ov_is_repeat(B, o, lane);
            if (rep) why = rep == 1 ? RB_OVL_WHY_REPEAT : RB_OVL_WHY_REPEAT_THROWS;
        }
        if (why != RB_OVL_WHY_FOUND) {
            if (lane == 0) ov_put(rec, RB_OVL_NONE, why, flags, o, 0, 0, 0);
            return;
        }
    } else if (sn > 0 && !complex_any) {
        if (lane == 0) ov_put(rec, RB_OVL_NONE, RB_OVL_WHY_NO_COMPLEX, flags, o, 0, 0, 0);
        return;
    }
    for (int p = (int)lane; p < len; p += 64) o_txt[p] = (uint8_t)t(p);
    if (lane == 0) ov_put(rec, first_bad < sn ? RB_OVL_RESCUE : RB_OVL_SPANNED, RB_OVL_WHY_FOUND, flags, o, len, sp0, sn);
}

}  // namespace

extern "C" {
int rb_graph_overlap_pairs(rb_graph *g, const char *lseq, const int64_t *loffsets, const char *rseq, const int64_t *roffsets, int64_t n,
                           int min_overlap, float min_kmer_cov, int64_t *out_offsets, char *out_seq, rb_overlap_rec *recs) {
    return guarded([&] {
        RB_REQUIRE(g && loffsets && roffsets && out_offsets && n >= 0, "rb_graph_overlap_pairs: null argument");
        RB_REQUIRE(recs || !out_seq, "rb_graph_overlap_pairs: out_seq needs recs");
        RB_REQUIRE(!g->shard, "rb_graph_overlap_pairs: not available on a shard handle");
        RB_REQUIRE(g->dbg.bits && g->cbf, "rb_graph_overlap_pairs: dbgbf or the counting filter has been destroyed");
        RB_REQUIRE(min_overlap >= 1, "rb_graph_overlap_pairs: min_overlap = %d (at least 1)", min_overlap);
        RB_REQUIRE(std::isfinite(min_kmer_cov), "rb_graph_overlap_pairs: min_kmer_cov must be finite");
        for (int64_t i = 0; i < n; ++i) {
            const int64_t ll = loffsets[i + 1] - loffsets[i], rl = roffsets[i + 1] - roffsets[i];
            RB_REQUIRE(ll >= 0 && rl >= 0, "rb_graph_overlap_pairs: decreasing offsets at pair %lld", (long long)i);
            RB_REQUIRE(ll + rl <= INT32_MAX, "rb_graph_overlap_pairs: pair %lld has more letters than an int holds", (long long)i);
        }
        const int64_t ltext = n ? loffsets[n] - loffsets[0] : 0, rtext = n ? roffsets[n] - roffsets[0] : 0;
        RB_REQUIRE((ltext == 0 || lseq) && (rtext == 0 || rseq), "rb_graph_overlap_pairs: null sequence text");
        // the capacity layout: both reads' letters, whatever comes of the pair
        auto cap = [&](int64_t i) { return (loffsets[i] - loffsets[0]) + (roffsets[i] - roffsets[0]); };
        for (int64_t i = 0; i <= n; ++i) out_offsets[i] = n ? cap(i) : 0;
        if (!out_seq || n == 0) return;
        RB_REQUIRE(recs, "rb_graph_overlap_pairs: null recs");
        RB_HIP(hipSetDevice(g->p.device));
        HostPin pin_l(ltext ? lseq + loffsets[0] : nullptr, (size_t)ltext), pin_r(rtext ? rseq + roffsets[0] : nullptr, (size_t)rtext), pin_out(out_seq, (size_t)(ltext + rtext)),
                pin_rec(recs, (size_t)n * sizeof(rb_overlap_rec));
        QueryLease q(g);
        hipStream_t s = q.c->st;
        const FilterView fv = g->view(0, 0);
        // piece by piece (rb_pieces.hpp), cut by the letters of both reads, 64 M a piece: b0 the piece's table, b1 / b2 the reads' text, b3 records
        // and text out; with profiling on the kernels of every piece are timed: entry "overlap"
        std::vector<int64_t> tab;
        for_each_piece(g, s, cap, n, (int64_t)64 << 20, "overlap", [&](Piece &pc) {
            const int64_t ra = pc.ra, rb_ = pc.rb, pn = pc.pn;
            const int64_t lt = loffsets[rb_] - loffsets[ra], rt = roffsets[rb_] - roffsets[ra];
            // the piece's table: left offsets [pn + 1], right offsets [pn + 1], the pairs that do not fit a row of LDS
            tab.assign((size_t)(2 * pn + 2), 0);
            for (int64_t i = 0; i <= pn; ++i) {
                tab[(size_t)i] = loffsets[ra + i] - loffsets[ra];
                tab[(size_t)(pn + 1 + i)] = roffsets[ra + i] - roffsets[ra];
            }
            for (int64_t i = 0; i < pn; ++i)
                if (!ov_fits_lds(tab[(size_t)i + 1] - tab[(size_t)i], tab[(size_t)(pn + 2 + i)] - tab[(size_t)(pn + 1 + i)])) tab.push_back(i);
            const int64_t nlong = (int64_t)tab.size() - (2 * pn + 2);
            const size_t o_txt = (size_t)pn * sizeof(rb_overlap_rec);
            q.c->b0.reserve(tab.size() * 8);
            q.c->b1.reserve((size_t)lt + 16);
            q.c->b2.reserve((size_t)rt + 16);
            q.c->b3.reserve(o_txt + (size_t)(lt + rt) + 16);
            const int64_t *dlof = q.c->b0.as<int64_t>(), *drof = dlof + pn + 1, *dids = drof + pn + 1;
            rb_overlap_rec *drec = q.c->b3.as<rb_overlap_rec>();
            uint8_t *dout = q.c->b3.as<uint8_t>() + o_txt;
            RB_HIP(hipMemcpyAsync(q.c->b0.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
            if (lt) RB_HIP(hipMemcpyAsync(q.c->b1.p, lseq + loffsets[ra], (size_t)lt, hipMemcpyHostToDevice, s));
            if (rt) RB_HIP(hipMemcpyAsync(q.c->b2.p, rseq + roffsets[ra], (size_t)rt, hipMemcpyHostToDevice, s));
            if (lt + rt) RB_HIP(hipMemsetAsync(dout, 0, (size_t)(lt + rt), s));     // (what no pair writes comes back as zeros, whatever the cuts)
            pc.kernels_begin();
            hipLaunchKernelGGL((k_overlap<true>), dim3(blocks_for(pn, OV_WAVES)), dim3(OV_TPB), 0, s, fv, (int)g->stranded, g->k, min_overlap, min_kmer_cov,
                               pn, (const int64_t *)nullptr, (int64_t)0, dlof, drof, q.c->b1.as<uint8_t>(), q.c->b2.as<uint8_t>(), dout, drec);
            RB_HIP(hipGetLastError());
            if (nlong) {
                hipLaunchKernelGGL((k_overlap<false>), dim3(blocks_for(nlong, OV_WAVES)), dim3(OV_TPB), 0, s, fv, (int)g->stranded, g->k, min_overlap,
                                   min_kmer_cov, pn, dids, nlong, dlof, drof, q.c->b1.as<uint8_t>(), q.c->b2.as<uint8_t>(), dout, drec);
                RB_HIP(hipGetLastError());
            }
            pc.kernels_end();
            RB_HIP(hipMemcpyAsync(recs + ra, drec, (size_t)pn * sizeof(rb_overlap_rec), hipMemcpyDeviceToHost, s));
            if (lt + rt) RB_HIP(hipMemcpyAsync(out_seq + out_offsets[ra], dout, (size_t)(lt + rt), hipMemcpyDeviceToHost, s));
        });
    });
}
}  // extern "C"
