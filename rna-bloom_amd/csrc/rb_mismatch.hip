// rb_mismatch.hip — mismatch correction of host sequences (rb_graph_correct_mismatches): GraphUtils.correctMismatches
// (R/util/GraphUtils.java:3914-3996, the last step of correctErrorHelper :3904) on the device.  Per piece the getKmers kernel leaves the
// forward / reverse hashes and the count of every window in device scratch; k_mismatch then runs the reference's two scans, a wavefront per
// sequence, on a row of one count code per window, and rewrites text, hashes and codes in place wherever a variant wins.  Only the
// sequences and thresholds go in and the corrected sequences, the number of replacements and (on request) the final count rows come out
// (DESIGN.md §5 "Mismatch correction").
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rb_pieces.hpp"
#include "rb_lookup.hpp"
#include "rb_wave.hpp"

using namespace rb;

// Java float arithmetic: the median of an even number of counts is one float32 sum and one float32 division
#pragma clang fp contract(off)

namespace {

constexpr int MM_TPB = 256;
constexpr int MM_WAVES = MM_TPB / 64;    // sequences per workgroup: a wavefront each
constexpr int MM_LDS_ROW = 4096;         // windows of a sequence whose code row lives in LDS; longer ones keep it in device scratch
constexpr int MM_SLOTS = (RB_MAX_K + 63) / 64;   // windows a lane owns of the k windows of one candidate

// the smallest count code (count_code_of, rb_device.hpp) whose value is >= t (129: none): `count >= t` is `code >= mm_threshold_code(t)` for every count there is
__device__ __forceinline__ uint32_t mm_threshold_code(float t, uint32_t lane) {
    const unsigned long long m0 = __ballot(count_code_value(lane) >= t), m1 = __ballot(count_code_value(64u + lane) >= t);
    if (m0) return (uint32_t)__builtin_ctzll(m0);
    if (m1) return 64u + (uint32_t)__builtin_ctzll(m1);
    return count_code_value(128u) >= t ? 128u : 129u;
}

// are the bases [j, j + k) of the sequence usable, position q (the one being replaced by A C G T) left out?
__device__ __forceinline__ bool mm_window_clean(const uint32_t *__restrict__ vw, uint32_t j, uint32_t k, uint32_t q) {
    bool ok = true;
    for (uint32_t b = j; b < j + k;) {
        const uint32_t lo = b & 31u, n = min(32u - lo, j + k - b);
        const uint32_t mask = (n == 32u ? ~0u : ((1u << n) - 1u)) << lo;
        uint32_t miss = ~vw[b >> 5] & mask;
        if ((q >> 5) == (b >> 5)) miss &= ~(1u << (q & 31u));
        ok = ok && miss == 0u;
        b += n;
    }
    return ok;
}

// One window of a candidate under each of the four substitutions: ntHash is XOR-linear, so with the replaced base at exponent ef on the
// forward strand and er on the reverse strand the variant's hashes are f ^ rotl(seed(old) ^ seed(new), ef) and the mirrored term — no
// rolling.  Returns the four count codes (byte a = substitution a; 0 where the window has another unusable base, `clean` false) and in
// `inmask` bit a = the variant window is in dbgbf (graph.contains: the Bloom bits alone).  With two hash functions per filter — every
// configuration the reference runs — the probes of the four variants are issued together (count_lookup4, rb_lookup.hpp); a substitution
// that is not tried (the base itself) probes its neighbour's lines again instead of the window's own.
__device__ __forceinline__ uint32_t mm_variant_codes(const FilterView &fv, int stranded, uint64_t f, uint64_t r, uint64_t so, uint64_t sco,
                                                     uint32_t ef, uint32_t er, uint32_t altmask, bool clean, uint32_t &inmask) {
    uint64_t h[4];
#pragma unroll
    for (uint32_t a = 0; a < 4u; ++a) {
        const uint64_t nf = f ^ rotl_var(so ^ seed_of(a), ef);
        const uint64_t nr = r ^ rotl_var(sco ^ seed_of(3u - a), er);
        h[a] = stranded ? nf : canonical(nf, nr);
    }
#pragma unroll
    for (uint32_t a = 0; a < 4u; ++a)
        if (!((altmask >> a) & 1u)) h[a] = h[a ^ 1u];
    uint32_t codes = 0, ins = 0;
    count_lookup4(fv, h, [&](uint32_t a, bool in, uint32_t mn) {
        ins |= (in ? 1u : 0u) << a;
        codes |= ((in && clean) ? 1u + mn : 0u) << (8u * a);
    });
    inmask = ins;
    return codes;
}

// Common.getMedian (R/util/Common.java:41-50) of the n codes a wavefront holds in c[] (lane l, slot s: element 64 s + l; 255 past the end):
// sorted[n / 2], or (sorted[n / 2 - 1] + sorted[n / 2]) / 2.0f.  An order statistic is found by bisection over the 129 code values with
// one ballot per slot and step: no sort, no LDS.  Not kth_code (rb_lookup.hpp): the slots are registers, which a slot index known only at run
// time would send to scratch, so the loop over them stays unrolled here; the even / odd rule on top is the shared one.
__device__ __forceinline__ uint32_t mm_kth(const uint32_t (&c)[MM_SLOTS], int n, int rank) {
    uint32_t lo = 0, hi = 128;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        int cnt = 0;
#pragma unroll
        for (int s = 0; s < MM_SLOTS; ++s)
            if (s * 64 < n) cnt += __popcll(__ballot(c[s] <= mid));
        if (cnt >= rank + 1) hi = mid; else lo = mid + 1u;
    }
    return lo;
}
__device__ __forceinline__ float mm_median(const uint32_t (&c)[MM_SLOTS], int n) {
    return median_of_kth([&](int rank) { return mm_kth(c, n, rank); }, n);
}

// A wavefront per sequence: sequence r of the piece has windows [kof[r], kof[r + 1]) of F / R / cnt (what the getKmers kernel left) and
// text txt[tof[r] ...].  LDS_ROW: workgroup b takes sequences 4 b .. 4 b + 3, the code row of each in LDS, and leaves those with more
// than MM_LDS_ROW windows to the other instantiation, which takes the sequences listed in ids and keeps the row in grow.
//   Both scans of the reference are one loop here (dir 0: i = 1 .. nk - k - 1 ascending, dir 1: i = nk - 2 .. k descending): 64 positions
// are tested at a time (count[i] < T, the neighbour behind >= T, the k-mer k windows on >= T: three code compares), the ballot's first
// position is handled and the scan resumes right behind it on the changed row.  In both directions the k windows that hold the replaced
// base are j0 .. j0 + k - 1 with the base q = j0 + k - 1 at offset k - 1 - w of window j0 + w, the baseline is the median of the k - 1
// codes row[j0 .. j0 + k - 2] (getMedianKmerCoverage(kmers, i, i + k - 1): one short of the k windows — reproduced), and the variant
// k-mer that has to be in dbgbf is window i itself (w = 0 forward, w = k - 1 in reverse).  Lane w owns window j0 + w (w += 64 while
// w < k), expands all four substitutions at once (mm_variant_codes) and parks the four codes in LDS; minimum >= min_kmer_cov is one
// ballot per slot, the median a bisection (mm_median).  A winner rewrites the base, the valid bit, k codes and k hash pairs.
//   The wavefront's lanes hand values to each other through the code row and its own rows of hashes in device memory: the fence after the
// row is filled and after every replacement waits for those stores before any lane reads them.
template <bool LDS_ROW>
__global__ void __launch_bounds__(MM_TPB) k_mismatch(FilterView fv, int stranded, int k, float min_cov, int64_t pn, const int64_t *__restrict__ ids,
                                                     int64_t n_ids, const int64_t *__restrict__ kof, const int64_t *__restrict__ tof,
                                                     const int32_t *__restrict__ nks, const uint32_t *__restrict__ woff, uint32_t *valid, uint8_t *txt, uint64_t *F, uint64_t *R, float *cnt,
                                                     uint8_t *grow, const float *__restrict__ thr, int32_t *__restrict__ n_fixed, int write_counts) {
    __shared__ uint8_t s_row[MM_WAVES][LDS_ROW ? MM_LDS_ROW : 4];
    __shared__ uint32_t s_vc[MM_WAVES][RB_MAX_K];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t slot = (int64_t)blockIdx.x * MM_WAVES + wv;
    int64_t r;
    if constexpr (LDS_ROW) { if (slot >= pn) return; r = slot; }
    else { if (slot >= n_ids) return; r = ids[slot]; }
    const int64_t k0 = kof[r];
    const int32_t nk = nks ? nks[r] : (int32_t)(kof[r + 1] - k0);
    if (LDS_ROW ? nk > MM_LDS_ROW : nk <= MM_LDS_ROW) return;     // (ids may list a sequence by its capacity: the row of a short one is the other instantiation's)
    const float T = thr[r];
    if (nk <= k + 1 || !(T > 0.0f)) {                    // neither loop of the reference has a position / no count is below T
        if (lane == 0) n_fixed[r] = 0;
        return;
    }
    uint8_t *row;
    if constexpr (LDS_ROW) row = s_row[wv]; else row = grow + k0;
    uint32_t *vc = s_vc[wv];
    uint32_t *vw = valid + woff[r];
    uint8_t *tx = txt + tof[r];
    uint64_t *f_ = F + k0, *r_ = R + k0;
    float *c_ = cnt + k0;
    const uint32_t tcode = mm_threshold_code(T, lane), mcode = mm_threshold_code(min_cov, lane);
    for (int32_t p = (int32_t)lane; p < nk; p += 64) row[p] = (uint8_t)count_code_of(c_[p]);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    int32_t nfix = 0;
    for (int dir = 0; dir < 2; ++dir) {
        const int32_t step = dir ? -1 : 1, lim = dir ? k : nk - k - 1;
        int32_t base = dir ? nk - 2 : 1;
        while (dir ? base >= lim : base <= lim) {
            const int32_t p = base + step * (int32_t)lane;
            bool cand = false;
            if (dir ? p >= lim : p <= lim) cand = row[p] < tcode && row[p - step] >= tcode && row[p + step * k] >= tcode;
            const unsigned long long m = __ballot(cand);
            if (!m) { base += step * 64; continue; }
            const int32_t i = base + step * (int32_t)__builtin_ctzll(m);
            const int32_t j0 = dir ? i - k + 1 : i, gw = dir ? k - 1 : 0, q = j0 + k - 1;
            const uint32_t ch = tx[q];
            const uint32_t altmask = alt_mask(ch);
            const uint64_t so = letter_seed(ch), sco = letter_rev_seed(ch);
            // the k windows under the four substitutions
            uint32_t gl = 0;
            for (int32_t w = (int32_t)lane; w < k; w += 64) {
                const int32_t j = j0 + w;
                uint32_t in;
                const uint32_t pk = mm_variant_codes(fv, stranded, f_[j], stranded ? 0ull : r_[j], so, sco, (uint32_t)w, (uint32_t)(k - 1 - w), altmask,
                                                     mm_window_clean(vw, (uint32_t)j, (uint32_t)k, (uint32_t)q), in);
                vc[w] = pk;
                if (w == gw) gl = in;
            }
            const uint32_t gate = (uint32_t)__shfl((int)gl, gw & 63, 64) & altmask;      // getRightVariants / getLeftVariants(String): contains(v)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            uint32_t cc[MM_SLOTS];
#pragma unroll
            for (int s = 0; s < MM_SLOTS; ++s) { const int32_t w = s * 64 + (int32_t)lane; cc[s] = w < k - 1 ? row[j0 + w] : 255u; }
            float best = mm_median(cc, k - 1);
            int besta = -1;
            for (int a = 0; a < 4; ++a) {
                if (!((gate >> a) & 1u)) continue;
                bool low = false;
#pragma unroll
                for (int s = 0; s < MM_SLOTS; ++s) {
                    const int32_t w = s * 64 + (int32_t)lane;
                    cc[s] = w < k ? (vc[w] >> (8 * a)) & 255u : 255u;
                    low = low || cc[s] < mcode;
                }
                if (__ballot(low)) continue;                         // getMinMedMaxKmerCoverage: m[0] >= minKmerCov
                const float med = mm_median(cc, k);
                if (med > best) { best = med; besta = a; }           // strictly: the first of equal medians stays
            }
            if (besta >= 0) {
                const uint64_t df = so ^ seed_of((uint32_t)besta), dr = sco ^ seed_of(3u - (uint32_t)besta);
                for (int32_t w = (int32_t)lane; w < k; w += 64) {
                    const int32_t j = j0 + w;
                    row[j] = (uint8_t)((vc[w] >> (8 * besta)) & 255u);
                    f_[j] ^= rotl_var(df, (uint32_t)w);
                    if (!stranded) r_[j] ^= rotl_var(dr, (uint32_t)(k - 1 - w));
                }
                if (lane == 0) {
                    tx[q] = code_letter((uint32_t)besta);
                    vw[q >> 5] |= 1u << (q & 31);
                }
                ++nfix;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            }
            base = i + step;
        }
    }
    if (write_counts)
        for (int32_t p = (int32_t)lane; p < nk; p += 64) c_[p] = count_code_value(row[p]);
    if (lane == 0) n_fixed[r] = nfix;
}

}  // namespace

int rb::mismatch_lds_row() { return MM_LDS_ROW; }
void rb::launch_mismatch(rb_graph *g, float min_kmer_cov, int64_t pn, const int64_t *ids, int64_t n_ids, const int64_t *kof, const int32_t *nks,
                         const int64_t *tof, const uint32_t *woff, uint32_t *valid, uint8_t *txt, uint64_t *F, uint64_t *R, float *cnt, uint8_t *grow,
                         const float *thr, int32_t *n_fixed, int write_counts, hipStream_t s) {
    const FilterView fv = g->view(0, 0);
    hipLaunchKernelGGL((k_mismatch<true>), dim3(blocks_for(pn, MM_WAVES)), dim3(MM_TPB), 0, s, fv, (int)g->stranded, g->k, min_kmer_cov, pn,
                       (const int64_t *)nullptr, (int64_t)0, kof, tof, nks, woff, valid, txt, F, R, cnt, grow, thr, n_fixed, write_counts);
    RB_HIP(hipGetLastError());
    if (n_ids) {
        hipLaunchKernelGGL((k_mismatch<false>), dim3(blocks_for(n_ids, MM_WAVES)), dim3(MM_TPB), 0, s, fv, (int)g->stranded, g->k, min_kmer_cov, pn, ids,
                           n_ids, kof, tof, nks, woff, valid, txt, F, R, cnt, grow, thr, n_fixed, write_counts);
        RB_HIP(hipGetLastError());
    }
}

extern "C" {
int rb_graph_correct_mismatches(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, const float *cov_threshold, float min_kmer_cov,
                                char *out_seq, int32_t *n_fixed, int64_t *koffsets, float *counts) {
    return guarded([&] {
        RB_REQUIRE(g && offsets && cov_threshold && out_seq && n_fixed && n >= 0, "rb_graph_correct_mismatches: null argument");
        RB_REQUIRE(!g->shard, "rb_graph_correct_mismatches: not available on a shard handle");
        RB_REQUIRE(g->dbg.bits && g->cbf, "rb_graph_correct_mismatches: dbgbf or the counting filter has been destroyed");
        RB_REQUIRE(g->k >= 2, "rb_graph_correct_mismatches: k = %d (the reference's median of k - 1 counts needs k >= 2)", g->k);
        RB_REQUIRE(std::isfinite(min_kmer_cov), "rb_graph_correct_mismatches: min_kmer_cov must be finite");
        RB_REQUIRE(!counts || koffsets, "rb_graph_correct_mismatches: counts needs koffsets");
        std::vector<int64_t> ko((size_t)n + 1);
        kmer_offsets(offsets, n, g->k, ko.data(), "rb_graph_correct_mismatches");
        for (int64_t i = 0; i < n; ++i)
            RB_REQUIRE(std::isfinite(cov_threshold[i]), "rb_graph_correct_mismatches: cov_threshold[%lld] is not finite", (long long)i);
        const int64_t text = n ? offsets[n] - offsets[0] : 0;
        RB_REQUIRE(text == 0 || seq, "rb_graph_correct_mismatches: null sequence text");
        if (koffsets) std::copy(ko.begin(), ko.end(), koffsets);
        if (n == 0) return;
        // what no kernel touches comes back as it went in: sequences shorter than k, pieces without a k-mer
        std::fill(n_fixed, n_fixed + n, 0);
        if (text && out_seq != seq) memmove(out_seq + offsets[0], seq + offsets[0], (size_t)text);
        const int64_t total = ko[(size_t)n];
        if (total == 0) return;
        RB_HIP(hipSetDevice(g->p.device));
        HostPin pin_seq(seq + offsets[0], (size_t)text), pin_out(out_seq + offsets[0], (size_t)text), pin_thr(cov_threshold, (size_t)n * 4),
                pin_nf(n_fixed, (size_t)n * 4), pin_cnt(counts, counts ? (size_t)total * 4 : 0);
        QueryLease q(g);
        hipStream_t s = q.c->st;
        // piece by piece (rb_pieces.hpp): 21 bytes of scratch a k-mer (two hashes, the count, the long sequences' code row), the text and the
        // piece's batch; with profiling on the kernels of every piece are timed: entry "mismatches"
        std::vector<int64_t> tab;
        for_each_host_piece(g, s, seq, offsets, ko.data(), n, "mismatches", [&](HostPiece &pc) {
            const int64_t ra = pc.ra, pn = pc.pn, pt = pc.pt, tb = offsets[pc.rb] - offsets[ra];
            // the piece's table behind its k-mer offsets: text offsets [pn + 1], the sequences whose code row does not fit LDS
            tab.assign((size_t)pn + 1, 0);
            for (int64_t i = 0; i <= pn; ++i) tab[(size_t)i] = offsets[ra + i] - offsets[ra];
            for (int64_t i = 0; i < pn; ++i)
                if (ko[(size_t)(ra + i + 1)] - ko[(size_t)(ra + i)] > MM_LDS_ROW) tab.push_back(i);
            const int64_t nlong = (int64_t)tab.size() - (pn + 1);
            // b3: counts [pt] floats, thresholds [pn], replacements [pn], text [tb], code rows of the long sequences [pt]
            const size_t o_thr = (size_t)pt * 4, o_nf = o_thr + (size_t)pn * 4, o_txt = o_nf + (size_t)pn * 4, o_row = up16(o_txt + (size_t)tb);
            q.c->b3.reserve(o_row + (nlong ? (size_t)pt : 0) + 16);
            uint8_t *base3 = q.c->b3.as<uint8_t>();
            float *dcnt = reinterpret_cast<float *>(base3), *dthr = reinterpret_cast<float *>(base3 + o_thr);
            int32_t *dnf = reinterpret_cast<int32_t *>(base3 + o_nf);
            uint8_t *dtxt = base3 + o_txt, *drow = base3 + o_row;
            RB_HIP(hipMemcpyAsync(dthr, cov_threshold + ra, (size_t)pn * 4, hipMemcpyHostToDevice, s));
            RB_HIP(hipMemcpyAsync(dtxt, seq + offsets[ra], (size_t)tb, hipMemcpyHostToDevice, s));
            const PieceRows rows(g, *q.c, pc, tab.data(), tab.size());
            const rb_batch *b = pc.batch();
            const int64_t *dkof = rows.kof, *dtof = dkof + pn + 1, *dids = dtof + pn + 1;
            rb::launch_mismatch(g, min_kmer_cov, pn, dids, nlong, dkof, nullptr, dtof, b->woff, b->valid, dtxt, q.c->b1.as<uint64_t>(), q.c->b2.as<uint64_t>(),
                                dcnt, drow, dthr, dnf, counts ? 1 : 0, s);
            pc.kernels_end();
            RB_HIP(hipMemcpyAsync(out_seq + offsets[ra], dtxt, (size_t)tb, hipMemcpyDeviceToHost, s));
            RB_HIP(hipMemcpyAsync(n_fixed + ra, dnf, (size_t)pn * 4, hipMemcpyDeviceToHost, s));
            if (counts) RB_HIP(hipMemcpyAsync(counts + ko[(size_t)ra], dcnt, (size_t)pt * 4, hipMemcpyDeviceToHost, s));
        });
    });
}
}  // extern "C"
