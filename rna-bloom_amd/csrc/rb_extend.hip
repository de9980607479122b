// rb_extend.hip — paired-k-mer branch extension of host sequences: rb_graph_extend_se = GraphUtils.extendRightSE / extendLeftSE
// (R/util/GraphUtils.java:6018-6204) over countKmerPairsSE / countKmerPairsReversedSE (:5718-5790), and rb_graph_extend_pe = extendRightPE /
// extendLeftPE (:6206-6414) over countKmerPairsPE / countKmerPairsReversedPE (:5792-5888) and graph.isRepeatKmer, both on
// naiveExtend{Right,Left}NoBackChecks (:6888-6933, :7067-7112), on the device.  Only the last min(n, d) k-mers of a sequence matter to the
// step (PE: max(d_r, d_f)), so the host hands the device the last (first, for the left-hand direction) d + k - 1 letters of every sequence;
// per piece the getKmers kernel leaves their hashes and counts in device scratch and k_extend runs the step, a wavefront per sequence: the up
// to 4 first-level and 16 second-level naive walks advance side by side, a lane per (walk, neighbour base), and the pair look-ups of a finished
// walk go a lane per walked k-mer.  The two steps are one body, the fragment-paired one a compile-time variant (template parameter PE).
// The step of one sequence (ex_one and what it is made of) lives in rb_extend_step.hpp, which rb_join.hip shares; this file has the kernel over a
// piece's sequences and the host side.  Nothing is written to the graph (DESIGN.md §5 "Branch extension", "Fragment-paired branch extension").
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

#include "rb_pieces.hpp"
#include "rb_extend_step.hpp"

using namespace rb;

// Java float arithmetic: the score is one float32 product and one float32 quotient, the median of an even number of counts one sum and one quotient
#pragma clang fp contract(off)

namespace {

// A wavefront per sequence, taking sequences in turn.  PE: the fragment-paired step.  LDS_ROW: the wavefront's rows are in LDS
// (d <= EX_LDS_D); else in its slot of `scratch`.
template <bool PE, bool LDS_ROW>
__global__ void __launch_bounds__(EX_TPB) k_extend(ExArgsT<PE> a, uint8_t *scratch, size_t row_bytes) {
    __shared__ __attribute__((aligned(16))) uint8_t s_row[EX_WAVES][LDS_ROW ? ex_row_bytes(EX_LDS_D) : 16];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t slot = (int64_t)blockIdx.x * EX_WAVES + wv, n_slots = (int64_t)gridDim.x * EX_WAVES;
    uint8_t *row;
    if constexpr (LDS_ROW) row = s_row[wv]; else row = scratch + (size_t)slot * row_bytes;
    for (int64_t r = slot; r < a.pn; r += n_slots) {
        ex_one<PE>(a, r, row, lane);
        wave_fence();
    }
}

template <bool PE> void ex_blank(std::conditional_t<PE, rb_extend_pe_rec, rb_extend_rec> &v, int d) {
    v.outcome = RB_EXT_NONE; v.why = RB_EXT_WHY_SHORT; v.n_candidates = 0; v.out_len = 0; v.last_partnered = -1; v.winner = -1; v.score = 0.0f;
    if constexpr (PE) { v.read_pairs = 0; v.frag_pairs = 0; v.max_ext = d - 2; } else v.pairs = 0;
}

// rb_graph_extend_se (PE false) and rb_graph_extend_pe (PE true): the checks, the cut of every sequence to the letters the step reads, and the
// pieces.  d is the distance the bounds, the rows and the output stride follow (read-paired for SE, fragment-paired for PE); the device
// gets the last (first, for the left-hand direction) max(d_r, d) + k - 1 letters of a sequence.
template <bool PE>
void extend_call(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, int direction, const float *min_kmer_cov, char *out_bases, float *out_count,
                 std::conditional_t<PE, rb_extend_pe_rec, rb_extend_rec> *recs) {
    using Rec = std::conditional_t<PE, rb_extend_pe_rec, rb_extend_rec>;
    const char *who = PE ? "rb_graph_extend_pe" : "rb_graph_extend_se";
    RB_REQUIRE(g, "%s: null handle", who);
    RB_REQUIRE(!g->shard, "%s: not available on a shard handle", who);
    RB_REQUIRE(g->dbg.bits && g->cbf, "%s: dbgbf or the counting filter has been destroyed", who);
    RB_REQUIRE(g->rpk.bits, "%s: the graph has no read-paired k-mer filter (created without useReadPairedKmers, or destroyed)", who);
    if (PE) RB_REQUIRE(g->fpk.bits, "%s: the graph has no fragment-paired k-mer filter (rb_graph_init_fragment_pairs was not called, or it was destroyed)", who);
    const int d_r = g->read_d, d = PE ? g->frag_d : d_r, k = g->k;
    RB_REQUIRE(d_r >= 2, "%s: the read-paired k-mer distance is %d (the step needs d >= 2)", who, d_r);
    if (PE) RB_REQUIRE(d >= 2, "%s: the fragment-paired k-mer distance is %d (the step needs d >= 2)", who, d);
    RB_REQUIRE(direction == 0 || direction == 1, "%s: direction must be 0 (right) or 1 (left), not %d", who, direction);
    RB_REQUIRE(n >= 0, "%s: n = %lld", who, (long long)n);
    if (n == 0) return;
    RB_REQUIRE(offsets && min_kmer_cov && out_bases && recs, "%s: null argument", who);
    std::vector<int64_t> ko((size_t)n + 1), to((size_t)n + 1, 0);
    kmer_offsets(offsets, n, k, ko.data(), who);
    RB_REQUIRE(offsets[n] == offsets[0] || seq, "%s: null sequence text", who);
    for (int64_t i = 0; i < n; ++i)
        RB_REQUIRE(std::isfinite(min_kmer_cov[i]) && min_kmer_cov[i] >= 0.0f, "%s: min_kmer_cov[%lld] must be finite and not negative", who, (long long)i);
    // the step reads the last min(nk, max(d_r, d)) k-mers of a sequence only: the device gets that many k-mers' letters at the end it extends
    const int64_t keep = (int64_t)std::max(d_r, d) + k - 1, stride = (int64_t)d + 2;
    for (int64_t i = 0; i < n; ++i) to[(size_t)i + 1] = to[(size_t)i] + std::min(offsets[i + 1] - offsets[i], keep);
    std::vector<char> text((size_t)to[(size_t)n]);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i], take = to[(size_t)i + 1] - to[(size_t)i];
        if (take) memcpy(text.data() + to[(size_t)i], seq + (direction ? offsets[i] : offsets[i] + len - take), (size_t)take);
    }
    kmer_offsets(to.data(), n, k, ko.data(), nullptr);
    // what no kernel touches: sequences of pieces without a k-mer, rows past a result's length
    for (int64_t i = 0; i < n; ++i) ex_blank<PE>(recs[i], d);
    memset(out_bases, 0, (size_t)(n * stride));
    if (out_count) memset(out_count, 0, (size_t)(n * stride) * 4);
    if (ko[(size_t)n] == 0) return;
    RB_HIP(hipSetDevice(g->p.device));
    HostPin pin_b(out_bases, (size_t)(n * stride)), pin_c(out_count, out_count ? (size_t)(n * stride) * 4 : 0), pin_r(recs, (size_t)n * sizeof(Rec));
    QueryLease q(g);
    hipStream_t s = q.c->st;
    const bool lds = d <= EX_LDS_D;
    const size_t row_bytes = ex_row_bytes(lds ? EX_LDS_D : d);
    // piece by piece (rb_pieces.hpp): b0 the piece's k-mer offsets, b1 / b2 the getKmers hashes, b3 counts, floors, records, results and — for a
    // distance past the LDS row — the wavefronts' walk rows; with profiling on the kernels of every piece are timed: entry "extend_se" / "extend_pe"
    for_each_host_piece(g, s, text.data(), to.data(), ko.data(), n, PE ? "extend_pe" : "extend_se", [&](HostPiece &pc) {
        const int64_t ra = pc.ra, pn = pc.pn, pt = pc.pt;
        const int64_t slots = lds ? pn : std::min<int64_t>(pn, EX_SCRATCH_SLOTS);
        const unsigned blocks = blocks_for(slots, EX_WAVES);
        const size_t o_fl = up16((size_t)pt * 4), o_rec = up16(o_fl + (size_t)pn * 4), o_b = o_rec + (size_t)pn * sizeof(Rec),
                     o_c = up16(o_b + (size_t)(pn * stride)), o_row = up16(o_c + (out_count ? (size_t)(pn * stride) * 4 : 0));
        q.c->b3.reserve(o_row + (lds ? 0 : (size_t)blocks * EX_WAVES * row_bytes) + 16);
        uint8_t *base3 = q.c->b3.as<uint8_t>();
        ExArgsT<PE> a;
        a.fv = g->view(0, 0);
        a.pf = PairView{g->rpk.bits, g->rpk.mod, g->rpk.num_hash, kmul_of(k)};
        a.stranded = (int)g->stranded; a.k = k; a.d = d; a.direction = direction; a.D = lds ? EX_LDS_D : d;
        a.floors = reinterpret_cast<float *>(base3 + o_fl);
        Rec *d_recs = reinterpret_cast<Rec *>(base3 + o_rec);
        if constexpr (PE) {
            a.recs = nullptr; a.recs_pe = d_recs;
            a.ff = PairView{g->fpk.bits, g->fpk.mod, g->fpk.num_hash, kmul_of(k)};
            a.d_r = d_r;
            // isRepeat keeps its counters in signed bytes: a threshold above 127 is never reached (t1 from k = 142 on; t2, t3 stay below for k <= RB_MAX_K)
            const int t1 = (int)java_round((float)k * 0.9f);
            a.t1 = t1 > 127 ? INT32_MAX : t1; a.t2 = (int)java_round((float)(k / 2) * 0.9f); a.t3 = (int)java_round((float)(k / 3) * 0.9f);
        } else a.recs = d_recs;
        a.out_b = base3 + o_b;
        a.out_c = out_count ? reinterpret_cast<float *>(base3 + o_c) : nullptr;
        RB_HIP(hipMemcpyAsync(base3 + o_fl, min_kmer_cov + ra, (size_t)pn * 4, hipMemcpyHostToDevice, s));
        RB_HIP(hipMemsetAsync(base3 + o_b, 0, o_row - o_b, s));        // (what no wavefront writes comes back as zeros, whatever the cuts)
        PieceRows(g, *q.c, pc).into(a);
        if (lds) hipLaunchKernelGGL((k_extend<PE, true>), dim3(blocks), dim3(EX_TPB), 0, s, a, (uint8_t *)nullptr, row_bytes);
        else hipLaunchKernelGGL((k_extend<PE, false>), dim3(blocks), dim3(EX_TPB), 0, s, a, base3 + o_row, row_bytes);
        RB_HIP(hipGetLastError());
        pc.kernels_end();
        RB_HIP(hipMemcpyAsync(recs + ra, d_recs, (size_t)pn * sizeof(Rec), hipMemcpyDeviceToHost, s));
        RB_HIP(hipMemcpyAsync(out_bases + ra * stride, a.out_b, (size_t)(pn * stride), hipMemcpyDeviceToHost, s));
        if (out_count) RB_HIP(hipMemcpyAsync(out_count + ra * stride, a.out_c, (size_t)(pn * stride) * 4, hipMemcpyDeviceToHost, s));
    });
}

}  // namespace

extern "C" {
int rb_graph_extend_se(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, int direction, const float *min_kmer_cov, char *out_bases,
                       float *out_count, rb_extend_rec *recs) {
    return guarded([&] { extend_call<false>(g, seq, offsets, n, direction, min_kmer_cov, out_bases, out_count, recs); });
}
int rb_graph_extend_pe(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, int direction, const float *min_kmer_cov, char *out_bases,
                       float *out_count, rb_extend_pe_rec *recs) {
    return guarded([&] { extend_call<true>(g, seq, offsets, n, direction, min_kmer_cov, out_bases, out_count, recs); });
}
}  // extern "C"
