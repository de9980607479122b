// rb_coverage.hip — coverage statistics of the count profile of resident reads (rb_graph_read_coverage): the handful of numbers stage 2
// reduces every read's sorted getKmers counts to (getCoverageStats, the threshold searches of correctErrorsSE / correctErrorsPE, the
// solid-k-mer count and windows of correctLongSequenceWindowed, the isRepeat screen of the single-end worker), computed on the device
// from a 129-bin histogram per segment instead of a sort on the host (DESIGN.md §5 "Coverage statistics").
#include <math.h>
#include <cmath>

#include <algorithm>
#include <vector>

#include "rb_pieces.hpp"
#include "rb_repeat.hpp"
#include "rb_covwalk.hpp"
#include "rb_wave.hpp"

using namespace rb;

// Java float arithmetic: every product and sum below is one float32 operation, rounded once (no contraction into fma)
#pragma clang fp contract(off)

namespace {

constexpr int COV_TPB = 256;
constexpr int64_t COV_LONG = 4096;       // segments of at least this many windows get a workgroup of their own

__device__ __forceinline__ bool window_usable(const uint32_t *vw, uint32_t b0, int k) {
    for (uint32_t b = b0; b < b0 + (uint32_t)k; ++b)
        if (!((vw[b >> 5] >> (b & 31u)) & 1u)) return false;
    return true;
}

struct CovSrc {                                        // the reads a segment's windows come from (n_complex)
    const uint64_t *codes;
    const uint32_t *valid, *woff;
    uint32_t r0;                                       // batch index of the piece's first read
};

// SPB segments per workgroup of COV_TPB threads (4: a wavefront each; 1: the whole workgroup for one long segment).  seg_row[s] .. seg_row[s+1]
// is segment s's range of the piece's profile; segments [0, half) come from `a` (out_lo), [half, n_seg) from `bsrc` (out_hi), each
// the mate of the one `half` away.  COMPLEX (reads mode): segment s is read s of its source, n_complex is computed.
// ids != nullptr: segment of workgroup i is ids[i] (the long ones); else segments of COV_LONG windows or more are skipped.
template <int SPB, bool COMPLEX>
__global__ void __launch_bounds__(COV_TPB) k_cov_stats(const float *__restrict__ prof, const int64_t *__restrict__ seg_row, int64_t n_seg,
                                                       int64_t half, const int64_t *__restrict__ ids, int64_t n_ids, rb_cov_params p, int k,
                                                       int pe, CovSrc a, CovSrc bsrc, rb_cov_stats *__restrict__ out_lo,
                                                       rb_cov_stats *__restrict__ out_hi) {
    constexpr int TPS = COV_TPB / SPB;                 // threads per segment
    __shared__ uint32_t hist[SPB][COV_BINS + 1];       // bin counts, then cum (exclusive prefix; [COV_BINS] = n)
    __shared__ uint32_t nsc[SPB][2];                   // n_solid, n_complex
    __shared__ float res[SPB][12];                     // order statistics and walk results
    __shared__ uint32_t fl[SPB];
    const int grp = (int)threadIdx.x / TPS, lt = (int)threadIdx.x % TPS;
    int64_t s = ids ? ((int64_t)blockIdx.x < n_ids ? ids[blockIdx.x] : -1) : (int64_t)blockIdx.x * SPB + grp;
    if (s >= n_seg) s = -1;
    const int64_t row = s >= 0 ? seg_row[s] : 0, n = s >= 0 ? seg_row[s + 1] - row : 0;
    const bool mine = s >= 0 && (ids || n < COV_LONG);
    uint32_t *h = hist[grp];
    for (int i = lt; i <= COV_BINS; i += TPS) h[i] = 0u;
    if (lt < 2) nsc[grp][lt] = 0u;
    if (lt == 0) fl[grp] = 0u;
    __syncthreads();
    if (mine) {
        uint32_t solid = 0, cplx = 0;
        const CovSrc &src = s < half ? a : bsrc;
        const int64_t rd = s < half ? s : s - half;
        const uint32_t wr = COMPLEX ? src.woff[src.r0 + (uint32_t)rd] : 0u;
        const uint32_t *cw32 = COMPLEX ? reinterpret_cast<const uint32_t *>(src.codes + wr) : nullptr;
        const uint32_t *vw = COMPLEX ? src.valid + wr : nullptr;
        const int t1 = (int)java_round((float)k * 0.9f), t2 = (int)java_round((float)(k / 2) * 0.9f), t3 = (int)java_round((float)(k / 3) * 0.9f);
        for (int64_t i = lt; i < n; i += TPS) {
            const float c = prof[row + i];
            atomicAdd(&h[count_code_of(c)], 1u);
            solid += c >= p.min_kmer_cov ? 1u : 0u;
            if (COMPLEX && (c > 0.0f || window_usable(vw, (uint32_t)i, k)) && !window_is_repeat(cw32, (uint32_t)i, k, t1, t2, t3)) ++cplx;
        }
        if (solid) atomicAdd(&nsc[grp][0], solid);
        if (COMPLEX && cplx) atomicAdd(&nsc[grp][1], cplx);
    }
    __syncthreads();
    // exclusive prefix of the bins over one wavefront: lane l holds bins 2l, 2l+1 (and 128)
    uint32_t x0 = 0, x1 = 0, x2 = 0, inc = 0;
    if (lt < 64) {
        x0 = h[2 * lt]; x1 = h[2 * lt + 1]; x2 = lt == 63 ? h[128] : 0u;
        inc = x0 + x1 + x2;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(inc, d, 64);
            if (lt >= d) inc += y;
        }
    }
    __syncthreads();
    if (lt < 64) {
        const uint32_t exc = inc - (x0 + x1 + x2);
        h[2 * lt] = exc; h[2 * lt + 1] = exc + x0;
        if (lt == 63) { h[128] = exc + x0 + x1; h[129] = inc; }
    }
    __syncthreads();
    // lanes 0..7: the order statistics; 8: correctErrorsSE's walk; 9: correctErrorsPE's; 10: getCoverageStats' drop-off
    if (mine && n > 0 && lt < 11) {
        const int64_t halfLen = n / 2, q1i = n / 4, q3i = halfLen + q1i;
        if (lt < 8) {
            const int64_t base = lt < 3 ? q1i : lt < 5 ? halfLen : q3i;       // ranks 0, q1-1, q1, half-1, half, q3-1, q3, n-1
            const int64_t rk = lt == 0 ? 0 : lt == 7 ? n - 1 : base - ((lt & 1) ? 1 : 0);
            res[grp][lt] = rk >= 0 ? count_code_value((uint32_t)bin_of_rank(h, rk)) : 0.0f;
        } else if (lt == 8) {
            const int64_t start = n - 1 - java_round((float)n * p.cov_fpr);
            bool found = false;
            res[grp][8] = start >= 0 ? cov_walk(h, start, p.max_cov_gradient, true, found) : 0.0f;
            atomicOr(&fl[grp], found ? RB_COV_SE_FOUND : 0u);
        } else if (lt == 9) {
            bool found = false;
            float t = 0.0f;
            if (pe) {
                const int64_t o = s < half ? s + half : s - half, no = seg_row[o + 1] - seg_row[o];
                const int64_t nfp = java_round((float)(n > no ? n : no) * p.cov_fpr);
                int64_t start = n - 1;
                if (start > nfp) start -= nfp;
                t = cov_walk(h, start, p.max_cov_gradient, false, found);
            }
            res[grp][9] = t;
            atomicOr(&fl[grp], found ? RB_COV_PE_FOUND : 0u);
        } else {
            bool found = false;
            float d = 0.0f;
            if (n >= p.lookahead) {
                d = cov_walk(h, n - p.lookahead, p.max_cov_gradient, true, found);
                if (!found) d = 0.0f;
            }
            res[grp][10] = d;
        }
    }
    __syncthreads();
    if (mine && lt == 0) {
        rb_cov_stats r;
        r.n = (int32_t)n; r.n_solid = (int32_t)nsc[grp][0]; r.n_complex = COMPLEX ? (int32_t)nsc[grp][1] : 0;
        if (n > 0) {
            const float *v = res[grp];
            r.flags = fl[grp];
            r.min = v[0]; r.max = v[7];
            r.median = n % 2 == 0 ? (v[3] + v[4]) / 2.0f : v[4];
            r.q1 = n % 4 == 0 ? (v[1] + v[2]) / 2.0f : v[2];
            r.q3 = n % 4 == 0 ? (v[5] + v[6]) / 2.0f : v[6];
            r.dropoff = v[10]; r.se_threshold = v[8]; r.pe_threshold = v[9];
        } else {
            r.flags = 0u; r.min = r.q1 = r.median = r.q3 = r.max = r.dropoff = r.se_threshold = r.pe_threshold = 0.0f;
        }
        (s < half ? out_lo + s : out_hi + (s - half))[0] = r;
    }
}

// windows of the first pass of correctLongSequenceWindowed (GraphUtils.java:3110-3140) over a read of nk k-mers: their start offsets
template <typename F> void for_each_window(int64_t nk, int64_t W, F &&f) {
    const int64_t shift = W / 2;
    for (int64_t i = 0, end = 0; i < nk; i = end) {
        end = std::min(i + W, nk);
        if (end + shift >= nk) end = nk;
        f(i);
    }
}
int64_t count_windows(int64_t nk, int64_t W) {
    int64_t c = 0;
    for_each_window(nk, W, [&](int64_t) { ++c; });
    return c;
}

}  // namespace

extern "C" {
int rb_graph_read_coverage(rb_graph *g, const rb_batch *b, int64_t first, int64_t n, const rb_batch *mates, int64_t mate_first,
                           const rb_cov_params *p, int64_t *seg_offsets, rb_cov_stats *out, int out_on_device) {
    return guarded([&] {
        RB_REQUIRE(g && b && p, "rb_graph_read_coverage: null argument");
        RB_REQUIRE(!g->shard, "rb_graph_read_coverage: queries are not available on a shard handle");
        RB_REQUIRE(b->device == g->p.device, "rb_graph_read_coverage: batch and graph live on different devices");
        RB_REQUIRE(first >= 0 && n >= 0 && first + n <= b->n_reads, "rb_graph_read_coverage: read range outside the batch");
        RB_REQUIRE(p->segments == RB_COV_READS || p->segments == RB_COV_WINDOWS, "rb_graph_read_coverage: segments must be RB_COV_READS (0) or RB_COV_WINDOWS (1)");
        RB_REQUIRE(p->segments == RB_COV_READS || p->window >= 1, "rb_graph_read_coverage: window must be >= 1");
        RB_REQUIRE(p->lookahead >= 1, "rb_graph_read_coverage: lookahead must be >= 1");
        RB_REQUIRE(std::isfinite(p->max_cov_gradient) && p->max_cov_gradient >= 0.0f, "rb_graph_read_coverage: max_cov_gradient must be finite and >= 0");
        RB_REQUIRE(p->cov_fpr >= 0.0f && p->cov_fpr <= 1.0f, "rb_graph_read_coverage: cov_fpr must be in [0, 1]");
        RB_REQUIRE(std::isfinite(p->min_kmer_cov), "rb_graph_read_coverage: min_kmer_cov must be finite");
        if (mates) {
            RB_REQUIRE(p->segments == RB_COV_READS, "rb_graph_read_coverage: mates are only available with RB_COV_READS");
            RB_REQUIRE(mates->device == g->p.device, "rb_graph_read_coverage: mate batch and graph live on different devices");
            RB_REQUIRE(mate_first >= 0 && mate_first + n <= mates->n_reads, "rb_graph_read_coverage: mate range outside the mate batch");
        }
        RB_REQUIRE(p->segments == RB_COV_READS || seg_offsets || n == 0, "rb_graph_read_coverage: seg_offsets is required with RB_COV_WINDOWS");
        RB_REQUIRE(g->cbf, "rb_graph_read_coverage: the counting filter has been destroyed");
        if (seg_offsets) seg_offsets[0] = 0;
        if (n == 0) return;
        const bool windows = p->segments == RB_COV_WINDOWS;
        RB_HIP(hipSetDevice(g->p.device));
        QueryLease q(g);
        hipStream_t s = q.c->st;
        // k-mers per read (and per mate): the lengths come back once, 4 bytes a read
        std::vector<uint32_t> len((size_t)n * (mates ? 2 : 1));
        RB_HIP(hipMemcpyAsync(len.data(), b->len + first, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        if (mates) RB_HIP(hipMemcpyAsync(len.data() + n, mates->len + mate_first, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        RB_HIP(hipStreamSynchronize(s));
        const uint32_t uk = (uint32_t)g->k;
        auto nk = [&](size_t i) -> int64_t { return len[i] >= uk ? (int64_t)(len[i] - uk + 1) : 0; };
        std::vector<int64_t> segoff((size_t)n + 1, 0);
        for (int64_t i = 0; i < n; ++i) segoff[(size_t)i + 1] = segoff[(size_t)i] + (windows ? count_windows(nk((size_t)i), p->window) : 1);
        if (seg_offsets) std::copy(segoff.begin(), segoff.end(), seg_offsets);
        if (!out) return;
        const int64_t n_rec = segoff[(size_t)n] + (mates ? n : 0);
        if (n_rec == 0) return;
        // pieces of <= 64 M windows + reads (rb_pieces.hpp; the profile is 4 bytes a window, a record 48 bytes): scratch stays bounded whatever n is
        const std::vector<int64_t> cut = piece_cuts_by_cost([&](int64_t i) { return 1 + nk((size_t)i) + (mates ? 1 + nk((size_t)(n + i)) : 0); }, n,
                                                            query_piece_max((int64_t)64 << 20));
        // per piece, one host table uploaded to b0: koffsets of the reads [pn + 1] (of the mates [pn + 1]), segment rows [nseg + 1], long segments
        struct Piece { int64_t ra, rb, nseg, nlo, nlong, kmers; size_t ko_b, row_at, long_at; std::vector<int64_t> tab; };
        std::vector<Piece> pcs;
        size_t max_tab = 0;
        int64_t max_kmers = 0, max_rec = 0;
        for (size_t c = 0; c + 1 < cut.size(); ++c) {
            Piece pc{cut[c], cut[c + 1], 0, 0, 0, 0, 0, 0, 0, {}};
            const int64_t pn = pc.rb - pc.ra;
            std::vector<int64_t> &t = pc.tab;
            t.push_back(0);
            for (int64_t i = pc.ra; i < pc.rb; ++i) t.push_back(t.back() + nk((size_t)i));
            if (mates) {
                pc.ko_b = t.size() - 1;                     // the mates' koffsets continue the reads' rows
                for (int64_t i = pc.ra; i < pc.rb; ++i) t.push_back(t.back() + nk((size_t)(n + i)));
            }
            pc.kmers = t.back();
            if (windows) {
                pc.row_at = t.size();
                for (int64_t i = 0; i < pn; ++i) for_each_window(nk((size_t)(pc.ra + i)), p->window, [&](int64_t w) { t.push_back(t[(size_t)i] + w); });
                t.push_back(pc.kmers);
            }
            pc.nseg = (int64_t)(t.size() - pc.row_at) - 1;
            pc.nlo = mates ? pn : pc.nseg;
            pc.long_at = t.size();
            for (int64_t j = 0; j < pc.nseg; ++j)
                if (t[pc.row_at + (size_t)j + 1] - t[pc.row_at + (size_t)j] >= COV_LONG) t.push_back(j);
            pc.nlong = (int64_t)(t.size() - pc.long_at);
            max_tab = std::max(max_tab, t.size());
            max_kmers = std::max(max_kmers, pc.kmers);
            max_rec = std::max(max_rec, pc.nseg);
            pcs.push_back(std::move(pc));
        }
        q.c->b0.reserve(max_tab * 8);
        q.c->b1.reserve((size_t)std::max<int64_t>(max_kmers, 1) * 4);
        if (!out_on_device) q.c->b2.reserve((size_t)max_rec * sizeof(rb_cov_stats) * 2);
        HostPin pin_out(out_on_device ? nullptr : out, (size_t)n_rec * sizeof(rb_cov_stats));
        int64_t *dtab = q.c->b0.as<int64_t>();
        float *prof = q.c->b1.as<float>();
        rb_cov_stats *buf[2] = {q.c->b2.as<rb_cov_stats>(), q.c->b2.as<rb_cov_stats>() + max_rec};
        rb::Stream s2;
        std::vector<rb::Event> ev;
        if (!out_on_device) RB_HIP(hipStreamCreateWithFlags(&s2.s, hipStreamNonBlocking));
        std::vector<hipEvent_t> copied;                     // per piece: its records are on the host (its buffer is free again)
        for (size_t c = 0; c < pcs.size(); ++c) {
            const Piece &pc = pcs[c];
            const int64_t pn = pc.rb - pc.ra;
            RB_HIP(hipMemcpyAsync(dtab, pc.tab.data(), pc.tab.size() * 8, hipMemcpyHostToDevice, s));
            launch_batch_counts(g, b, b->h_woff[(size_t)(first + pc.ra)], (int64_t)b->h_woff[(size_t)(first + pc.rb)] - b->h_woff[(size_t)(first + pc.ra)],
                                (uint32_t)(first + pc.ra), dtab, 0, prof, s);
            if (mates)
                launch_batch_counts(g, mates, mates->h_woff[(size_t)(mate_first + pc.ra)],
                                    (int64_t)mates->h_woff[(size_t)(mate_first + pc.rb)] - mates->h_woff[(size_t)(mate_first + pc.ra)],
                                    (uint32_t)(mate_first + pc.ra), dtab + pc.ko_b, 0, prof, s);
            rb_cov_stats *lo, *hi;
            if (out_on_device) { lo = out + segoff[(size_t)pc.ra]; hi = out + segoff[(size_t)n] + pc.ra; }
            else {
                if (c >= 2) RB_HIP(hipStreamWaitEvent(s, copied[c - 2], 0));
                lo = buf[c & 1]; hi = lo + pc.nlo;
            }
            const CovSrc sa{b->codes, b->valid, b->woff, (uint32_t)(first + pc.ra)};
            const CovSrc sb = mates ? CovSrc{mates->codes, mates->valid, mates->woff, (uint32_t)(mate_first + pc.ra)} : sa;
            const int64_t *rows = dtab + pc.row_at, *longs = dtab + pc.long_at;
            const int pe = mates ? 1 : 0;
            if (pc.nseg == 0) {
            } else if (windows) {
                hipLaunchKernelGGL((k_cov_stats<4, false>), dim3(blocks_for(pc.nseg, 4)), dim3(COV_TPB), 0, s, prof, rows, pc.nseg, pc.nlo,
                                   (const int64_t *)nullptr, (int64_t)0, *p, g->k, pe, sa, sb, lo, hi);
                if (pc.nlong)
                    hipLaunchKernelGGL((k_cov_stats<1, false>), dim3((unsigned)pc.nlong), dim3(COV_TPB), 0, s, prof, rows, pc.nseg, pc.nlo, longs,
                                       pc.nlong, *p, g->k, pe, sa, sb, lo, hi);
            } else {
                hipLaunchKernelGGL((k_cov_stats<4, true>), dim3(blocks_for(pc.nseg, 4)), dim3(COV_TPB), 0, s, prof, rows, pc.nseg, pc.nlo,
                                   (const int64_t *)nullptr, (int64_t)0, *p, g->k, pe, sa, sb, lo, hi);
                if (pc.nlong)
                    hipLaunchKernelGGL((k_cov_stats<1, true>), dim3((unsigned)pc.nlong), dim3(COV_TPB), 0, s, prof, rows, pc.nseg, pc.nlo, longs,
                                       pc.nlong, *p, g->k, pe, sa, sb, lo, hi);
            }
            RB_HIP(hipGetLastError());
            if (out_on_device) continue;
            ev.emplace_back(); RB_HIP(hipEventCreateWithFlags(&ev.back().e, hipEventDisableTiming)); const hipEvent_t e = ev.back();
            ev.emplace_back(); RB_HIP(hipEventCreateWithFlags(&ev.back().e, hipEventDisableTiming)); const hipEvent_t e2 = ev.back();
            RB_HIP(hipEventRecord(e, s));
            RB_HIP(hipStreamWaitEvent(s2, e, 0));
            const size_t rs = sizeof(rb_cov_stats);
            if (pc.nlo) RB_HIP(hipMemcpyAsync(out + segoff[(size_t)pc.ra], lo, (size_t)pc.nlo * rs, hipMemcpyDeviceToHost, s2));
            if (mates) RB_HIP(hipMemcpyAsync(out + segoff[(size_t)n] + pc.ra, hi, (size_t)pn * rs, hipMemcpyDeviceToHost, s2));
            RB_HIP(hipEventRecord(e2, s2));
            copied.push_back(e2);
        }
        RB_HIP(hipStreamSynchronize(s));
        if (s2) RB_HIP(hipStreamSynchronize(s2));
    });
}
}  // extern "C"
