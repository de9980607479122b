// rb_pairseg.hip — paired-k-mer segmentation of host sequences (rb_graph_paired_kmer_segments): GraphUtils.breakWithReadPairedKmers and
// breakWithFragPairedKmers (R/util/GraphUtils.java:4184-4405) on the device.  k_pair_support probes the pair filter for every pair position
// and leaves one support bit per position in device scratch; k_pair_segments walks those bits a sequence per lane and writes the segments.
// Only the sequences go in and the segments (plus, on request, one support byte per k-mer) come out (DESIGN.md §5 "Paired-k-mer segments").
#include <algorithm>
#include <vector>

#include "rb_pieces.hpp"

using namespace rb;

namespace {

constexpr int PS_TPB = 256;
constexpr int PS_GROUP = 8;              // pair positions of a lane whose probes are in flight together

// getKmers' rolling hash of one strand pair over the windows of a sequence, as k_get_kmers rolls it (unusable bases hash as seed 0 forward;
// the reverse-strand seed follows rnz, NTHash.java:30 `ch & 7`): the lane's left windows and their partners d windows on are two of these
struct Roll {
    const uint64_t *cw;
    const uint32_t *vw, *zw;
    uint32_t k, pos;                     // pos: start of the current window
    uint64_t f, r;
    __device__ __forceinline__ void seeds(uint32_t b, uint64_t &s, uint64_t &sc) const {
        const uint32_t c = (uint32_t)(cw[b >> 5] >> (2u * (b & 31u))) & 3u;
        s = ((vw[b >> 5] >> (b & 31u)) & 1u) ? seed_of(c) : 0ull;
        sc = ((zw[b >> 5] >> (b & 31u)) & 1u) ? seed_of(3u - c) : 0ull;
    }
    __device__ __forceinline__ void start(uint32_t p) {
        pos = p; f = 0; r = 0;
        for (uint32_t j = 0; j < k; ++j) {
            uint64_t s, sc;
            seeds(p + j, s, sc);
            f = rotl(f, 1) ^ s;
            r ^= rotl(sc, j);
        }
    }
    __device__ __forceinline__ void next() {
        uint64_t so, sco, si, sci;
        seeds(pos, so, sco);
        seeds(pos + k, si, sci);
        f = rotl(f, 1) ^ rotl(so, k) ^ si;
        r = rotr(r, 1) ^ rotr(sco, 1) ^ rotl(sci, k - 1u);
        ++pos;
    }
};

// One lane per 64 pair positions of a sequence: rolls windows p and p + d together, forms Kmer.getKmerPairHashValue (R/graph/Kmer.java:65-67,
// CanonicalKmer.java:61-72) and looks it up in the pair filter — BloomFilter.lookup's bits, all of them (the early exit changes only the
// traffic).  The probes of PS_GROUP positions (two hash functions at a time) are issued before any is consumed: a lane keeps up to 16 random
// lines in flight, as k_batch_counts does.  Sequence r of the piece owns support words [swo[r], swo[r + 1]) for its max(0, nk - d) positions;
// bits past the last position are 0.  sup_bytes (optional): byte kof[r] + p = bit p.  Without sup_bytes a word that lies wholly outside the
// positions the walk reads ([rangeStart, rangeEnd - 1 - d] of rng) is not probed: it is written 0.
__global__ void __launch_bounds__(PS_TPB) k_pair_support(const uint32_t *__restrict__ bits, Mod mod, int num_hash, uint64_t kmul, int stranded,
                                                         int k, int d, const uint64_t *__restrict__ codes, const uint32_t *__restrict__ valid,
                                                         const uint32_t *__restrict__ rnz, const uint32_t *__restrict__ woff,
                                                         const int64_t *__restrict__ kof, const int64_t *__restrict__ swo,
                                                         const int64_t *__restrict__ rng, int64_t pn, int64_t n_words, uint64_t *__restrict__ sup,
                                                         uint8_t *__restrict__ sup_bytes) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_words) return;
    int64_t lo = 0, hi = pn;                                 // the sequence whose words hold t: the last r with swo[r] <= t
    while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (swo[mid] <= t) lo = mid; else hi = mid; }
    const int64_t r = lo;
    const int64_t npos = kof[r + 1] - kof[r] - d, w = t - swo[r], p0 = w * 64;
    const int np = npos - p0 < 64 ? (int)(npos - p0) : 64;
    if (!sup_bytes && (p0 + np - 1 < rng[2 * r] || p0 > rng[2 * r + 1] - 1 - d)) { sup[t] = 0ull; return; }
    const uint32_t wr = woff[r];
    Roll L{codes + wr, valid + wr, rnz + wr, (uint32_t)k, 0, 0, 0}, R = L;
    L.start((uint32_t)p0);
    R.start((uint32_t)(p0 + d));
    uint64_t word = 0;
    for (int g = 0; g < np; g += PS_GROUP) {
        uint64_t key[PS_GROUP];
#pragma unroll
        for (int q = 0; q < PS_GROUP; ++q) {
            if (g + q < np) {
                if (g + q > 0) { L.next(); R.next(); }
                const uint64_t pf = combine(L.f, R.f);
                key[q] = stranded ? pf : smin(pf, combine(R.r, L.r));
            } else key[q] = key[0];
        }
        uint32_t hit = (1u << PS_GROUP) - 1u;
        for (int j = 0; j < num_hash; j += 2) {
            const bool two = j + 1 < num_hash;
            uint64_t ia[PS_GROUP], ib[PS_GROUP];
            uint32_t wa[PS_GROUP], wb[PS_GROUP];
#pragma unroll
            for (int q = 0; q < PS_GROUP; ++q) {
                ia[q] = index_of(multi_hash(key[q], (uint32_t)j, kmul), mod);
                ib[q] = two ? index_of(multi_hash(key[q], (uint32_t)j + 1u, kmul), mod) : ia[q];
            }
#pragma unroll
            for (int q = 0; q < PS_GROUP; ++q) wa[q] = bits[ia[q] >> 5];
#pragma unroll
            for (int q = 0; q < PS_GROUP; ++q) wb[q] = two ? bits[ib[q] >> 5] : ~0u;
#pragma unroll
            for (int q = 0; q < PS_GROUP; ++q)
                hit &= ~((((wa[q] >> (uint32_t)(ia[q] & 31u)) & (wb[q] >> (uint32_t)(ib[q] & 31u)) & 1u) ^ 1u) << q);
        }
        const int m = np - g < PS_GROUP ? np - g : PS_GROUP;
        word |= (uint64_t)(hit & ((1u << m) - 1u)) << g;
    }
    sup[t] = word;
    if (sup_bytes)
        for (int j = 0; j < np; ++j) sup_bytes[kof[r] + p0 + j] = (uint8_t)((word >> j) & 1ull);
}

// first position in [p, last] whose support bit is `want`, else last + 1
__device__ __forceinline__ int32_t next_bit(const uint64_t *__restrict__ w, int32_t p, int32_t last, bool want) {
    while (p <= last) {
        const uint64_t x = (want ? w[p >> 6] : ~w[p >> 6]) >> (uint32_t)(p & 63);
        if (x) { const int32_t q = p + (int32_t)__builtin_ctzll(x); return q <= last ? q : last + 1; }
        p = (p | 63) + 1;
    }
    return last + 1;
}

// One lane per sequence: the reference's loop over [rangeStart, lastIndex] (GraphUtils.java:4184-4310; both branches, interlockDistance 0),
// run by maximal runs of supported positions.  A run [a, b] of at least n positions opens a segment at a (the position where the count
// first reaches n, minus n - 1) and leaves end = b + d (its last position counts, and every one before it set a smaller end); a shorter run
// changes nothing.  The misses between two runs close an open segment iff the last of them is >= end (end does not move over misses).
// A sequence never has more segments than its slots (consecutive starts are >= d + 1 apart); should it, the extra ones are not written and
// *overflow counts the sequence, which the caller turns into an error.
__global__ void __launch_bounds__(PS_TPB) k_pair_segments(const uint64_t *__restrict__ sup, const int64_t *__restrict__ swo,
                                                          const int64_t *__restrict__ cap, const int64_t *__restrict__ rng, int64_t pn, int d,
                                                          int npr, int2 *__restrict__ segs, int32_t *__restrict__ n_segs, int32_t *__restrict__ overflow) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= pn) return;
    const uint64_t *w = sup + swo[r];
    const int32_t rs = (int32_t)rng[2 * r], last = (int32_t)rng[2 * r + 1] - 1 - d;
    const int64_t room = cap[r + 1] - cap[r];
    int2 *out = segs + cap[r];
    int32_t cur = rs, start = -1, end = -1;
    int64_t n = 0;
    while (cur <= last) {
        const int32_t a = next_bit(w, cur, last, true);
        if (a > last) break;
        if (start >= 0 && a - 1 >= cur && a - 1 >= end) {
            if (n < room) out[n] = make_int2(start, end + 1);
            ++n; start = -1;
        }
        const int32_t b = next_bit(w, a, last, false) - 1;
        if (b - a + 1 >= npr) { if (start < 0) start = a; end = b + d; }
        cur = b + 1;
    }
    if (start >= 0 && last >= cur && last >= end) {
        if (n < room) out[n] = make_int2(start, end + 1);
        ++n; start = -1;
    }
    if (start >= 0) {
        if (n < room) out[n] = make_int2(start, end + 1);
        ++n;
    }
    n_segs[r] = (int32_t)(n < room ? n : room);
    if (n > room) atomicAdd(overflow, 1);
}

}  // namespace

extern "C" {
int rb_graph_paired_kmer_segments(rb_graph *g, int which, const char *seq, const int64_t *offsets, int64_t n, int num_pairs_required,
                                  const int32_t *ranges, int64_t *seg_offsets, int32_t *segs, int32_t *n_segs, uint8_t *support,
                                  int64_t *koffsets) {
    return guarded([&] {
        RB_REQUIRE(g && offsets && seg_offsets && n >= 0, "rb_graph_paired_kmer_segments: null argument");
        RB_REQUIRE(!g->shard, "rb_graph_paired_kmer_segments: not available on a shard handle");
        RB_REQUIRE(which == RB_RPKBF || which == RB_FPKBF, "rb_graph_paired_kmer_segments: which must be RB_RPKBF (%d) or RB_FPKBF (%d), not %d",
                   RB_RPKBF, RB_FPKBF, which);
        RB_REQUIRE(bit_filter(g, which)->bits, which == RB_RPKBF
                   ? "rb_graph_paired_kmer_segments: the graph has no read-paired k-mer filter (created without useReadPairedKmers)"
                   : "rb_graph_paired_kmer_segments: the graph has no fragment-paired k-mer filter (rb_graph_init_fragment_pairs was never called)");
        const int d = which == RB_RPKBF ? g->read_d : g->frag_d;
        RB_REQUIRE(d >= 1, "rb_graph_paired_kmer_segments: the %s-paired k-mer distance is %d (set it to >= 1 first)", which == RB_RPKBF ? "read" : "fragment", d);
        RB_REQUIRE(num_pairs_required >= 1, "rb_graph_paired_kmer_segments: num_pairs_required must be >= 1, not %d", num_pairs_required);
        RB_REQUIRE(!support || koffsets, "rb_graph_paired_kmer_segments: support needs koffsets");
        RB_REQUIRE(!segs || n_segs, "rb_graph_paired_kmer_segments: segs needs n_segs");
        RB_REQUIRE(n == 0 || seq || offsets[n] == offsets[0], "rb_graph_paired_kmer_segments: null sequence text");
        std::vector<int64_t> ko((size_t)n + 1), so((size_t)n + 1, 0);
        kmer_offsets(offsets, n, g->k, ko.data(), "rb_graph_paired_kmer_segments");
        for (int64_t i = 0; i < n; ++i) {
            const int64_t nk = ko[(size_t)i + 1] - ko[(size_t)i], rs = ranges ? ranges[2 * i] : 0, re = ranges ? ranges[2 * i + 1] : nk;
            RB_REQUIRE(rs >= 0 && rs <= re && re <= nk, "rb_graph_paired_kmer_segments: range [%lld, %lld) of sequence %lld is outside [0, %lld]",
                       (long long)rs, (long long)re, (long long)i, (long long)nk);
            const int64_t span = re - 1 - d - rs;              // lastIndex - rangeStart
            so[(size_t)i + 1] = so[(size_t)i] + (span >= 0 ? span / (d + 1) + 1 : 0);
        }
        std::copy(so.begin(), so.end(), seg_offsets);
        if (koffsets) std::copy(ko.begin(), ko.end(), koffsets);
        if (!segs || n == 0) return;
        std::fill(n_segs, n_segs + n, 0);
        const int64_t total = ko[(size_t)n];
        if (total == 0) return;
        RB_HIP(hipSetDevice(g->p.device));
        HostPin pin_seq(seq + offsets[0], (size_t)(offsets[n] - offsets[0])), pin_segs(segs, (size_t)so[(size_t)n] * 8),
                pin_sup(support, support ? (size_t)total : 0);
        QueryLease q(g);
        const BitFilter *f = bit_filter(g, which);
        RB_REQUIRE(f->bits, "rb_graph_paired_kmer_segments: the pair filter is gone");
        hipStream_t s = q.c->st;
        // piece by piece (rb_pieces.hpp): the piece's batch (≈ 0.3 B a base) and 1 bit a position are all the scratch there is; with profiling
        // on the two kernels of every piece are timed: entry "pair_segments"
        std::vector<int64_t> tab;
        for_each_host_piece(g, s, seq, offsets, ko.data(), n, "pair_segments", [&](HostPiece &pc) {
            const int64_t ra = pc.ra, rb_ = pc.rb, pn = pc.pn, pt = pc.pt;
            // the piece's table: k-mer offsets [pn + 1], support-word offsets [pn + 1], segment slots [pn + 1], ranges [2 pn]
            tab.assign((size_t)(5 * pn + 3), 0);
            int64_t *kof = tab.data(), *swo = kof + pn + 1, *cap = swo + pn + 1, *rng = cap + pn + 1;
            for (int64_t i = 0; i < pn; ++i) {
                const int64_t nk = ko[(size_t)(ra + i + 1)] - ko[(size_t)(ra + i)], np = nk > d ? nk - d : 0;
                kof[i + 1] = kof[i] + nk;
                swo[i + 1] = swo[i] + (np + 63) / 64;
                cap[i + 1] = cap[i] + so[(size_t)(ra + i + 1)] - so[(size_t)(ra + i)];
                rng[2 * i] = ranges ? ranges[2 * (ra + i)] : 0;
                rng[2 * i + 1] = ranges ? ranges[2 * (ra + i) + 1] : nk;
            }
            const int64_t nw = swo[pn], nc = cap[pn];
            if (nw == 0 || (nc == 0 && !support)) {           // nothing to probe: no segment, every support byte 0
                if (support) std::fill(support + ko[(size_t)ra], support + ko[(size_t)rb_], (uint8_t)0);
                return;
            }
            const rb_batch *b = pc.batch();
            q.c->b0.reserve(tab.size() * 8);
            q.c->b1.reserve((size_t)nw * 8);
            q.c->b2.reserve((size_t)nc * 8 + (size_t)pn * 4 + 4);
            if (support) q.c->b3.reserve((size_t)pt);
            const int64_t *dkof = q.c->b0.as<int64_t>(), *dswo = dkof + pn + 1, *dcap = dswo + pn + 1, *drng = dcap + pn + 1;
            int2 *dsegs = q.c->b2.as<int2>();
            int32_t *dn = reinterpret_cast<int32_t *>(dsegs + nc), *dover = dn + pn;
            int32_t over = 0;
            RB_HIP(hipMemcpyAsync(q.c->b0.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
            RB_HIP(hipMemsetAsync(dover, 0, 4, s));
            if (support) RB_HIP(hipMemsetAsync(q.c->b3.p, 0, (size_t)pt, s));
            pc.kernels_begin();
            hipLaunchKernelGGL(k_pair_support, dim3(blocks_for(nw, PS_TPB)), dim3(PS_TPB), 0, s, (const uint32_t *)f->bits, f->mod, f->num_hash,
                               kmul_of(g->k), (int)g->stranded, g->k, d, b->codes, b->valid, b->rnz, b->woff, dkof, dswo, drng, pn, nw,
                               q.c->b1.as<uint64_t>(), support ? q.c->b3.as<uint8_t>() : nullptr);
            RB_HIP(hipGetLastError());
            if (nc) {
                hipLaunchKernelGGL(k_pair_segments, dim3(blocks_for(pn, PS_TPB)), dim3(PS_TPB), 0, s, q.c->b1.as<uint64_t>(), dswo, dcap, drng, pn,
                                   d, num_pairs_required, dsegs, dn, dover);
                RB_HIP(hipGetLastError());
            }
            pc.kernels_end();
            if (nc) {
                RB_HIP(hipMemcpyAsync(segs + 2 * so[(size_t)ra], dsegs, (size_t)nc * 8, hipMemcpyDeviceToHost, s));
                RB_HIP(hipMemcpyAsync(n_segs + ra, dn, (size_t)pn * 4, hipMemcpyDeviceToHost, s));
                RB_HIP(hipMemcpyAsync(&over, dover, 4, hipMemcpyDeviceToHost, s));
            }
            if (support) RB_HIP(hipMemcpyAsync(support + ko[(size_t)ra], q.c->b3.p, (size_t)pt, hipMemcpyDeviceToHost, s));
            pc.finish();                                        // (`over` is on the host)
            if (over) {
                set_error("rb_graph_paired_kmer_segments: %d sequences of reads [%lld, %lld) have more segments than their slots (internal error)",
                          over, (long long)ra, (long long)rb_);
                throw HipError{RB_ERR_STATE};
            }
        });
    });
}
}  // extern "C"
