// rb_pair_correct.hip — error correction of read pairs with all rounds inside the call (rb_graph_correct_pairs): GraphUtils.correctErrorsPE
// (R/util/GraphUtils.java:4051-4182), what the FragmentAssembler runs on every pair behind connect (R/RNABloom.java:2086-2235), and with no right
// mates correctErrorsSE (:3998-4049), the single-end worker's (R/RNABloom.java:1980-2001).  A round is the threshold search over both mates' sorted
// counts (:4071-4126), the combining rule (:4129-4143) and correctErrorHelper on both mates (:4145-4177); the helper is rb_correct.hip's body
// (rb_correct.hpp), run on text, hash rows and counts that never leave the device between rounds.
//   Per piece (rb_pieces.hpp; a pair is never split): the text goes up once and k_text_kmers profiles it.  Then, per round: k_pair_threshold — a
// wavefront per pair, the 129-bin histograms of both mates in LDS, the two downward walks of rb_covwalk.hpp, the combining rule and the
// min_cov_threshold test — names the pairs that run; k_pair_gather packs their rows densely (the round's capacity is corr_capacity of the actual
// lengths) and sends the finished pairs' texts to the staging buffer; the body runs; k_pair_commit adds the round to the pairs' records and decides
// which pairs live on; k_pair_threshold of the next round runs on the body's output where it lies.  The host sees lengths and live flags between
// rounds, builds the gather table from them, and gets the records and the final texts at the end.  (DESIGN.md §5 "Pair correction".)
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rb_correct.hpp"
#include "rb_covwalk.hpp"
#include "rb_wave.hpp"

using namespace rb;

// Java float arithmetic: n * covFPR and threshold * maxCovGradient are single float32 operations
#pragma clang fp contract(off)

namespace {

constexpr int PC_TPB = 256;
constexpr int PC_WAVES = PC_TPB / 64;            // pairs per workgroup: a wavefront each
enum { PC_DONE = 0, PC_LIVE = 1, PC_LOST = 2 };  // live[]: the pair is finished / enters the next round / lost a mate's k-mers

static_assert(sizeof(rb_pairc_rec) == 64, "rb_pairc_rec is 64 bytes");

__device__ __forceinline__ uint32_t float_bits(float x) { return __float_as_uint(x); }

// ---- the threshold of a round (:4071-4145; single form :4007-4036): a wavefront per pair of the current state.  Mate `side` of pair j is sequence
// j + side * half with nks[] k-mers whose counts lie at cnt + kof[].  Pairs with live[j] != PC_LIVE are passed over.  thr[seq] gets the round's
// threshold for both mates, or 0 — "no count is below it" — where the helper is not to run, and then the pair ends: END_LOW, live = PC_DONE.
__global__ void __launch_bounds__(PC_TPB) k_pair_threshold(int pe, int round, float gradient, float fpr, float min_thr, int64_t m, int64_t half,
                                                           const int64_t *__restrict__ kof, const int32_t *__restrict__ nks,
                                                           const float *__restrict__ cnt, const int32_t *__restrict__ pid, int32_t *__restrict__ live,
                                                           float *__restrict__ thr, rb_pairc_rec *__restrict__ recs) {
    __shared__ uint32_t hist[PC_WAVES][2][COV_BINS + 1];      // bin counts, then cum (exclusive prefix; [COV_BINS] = n)
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t j = (int64_t)blockIdx.x * PC_WAVES + wv;
    const bool mine = j < m && live[j] == PC_LIVE;
    const int sides = pe ? 2 : 1;
    for (int i = (int)lane; i < 2 * (COV_BINS + 1); i += 64) (&hist[wv][0][0])[i] = 0u;
    __syncthreads();
    if (mine)
        for (int side = 0; side < sides; ++side) {
            const int64_t sq = j + side * half;
            const float *c = cnt + kof[sq];
            const int32_t n = nks[sq];
            for (int32_t i = (int32_t)lane; i < n; i += 64) atomicAdd(&hist[wv][side][count_code_of(c[i])], 1u);
        }
    __syncthreads();
    // exclusive prefix of the bins over the wavefront: lane l holds bins 2l, 2l+1 (and 128); a lane reads and writes its own bins only
    for (int side = 0; side < sides; ++side) {
        uint32_t *h = hist[wv][side];
        const uint32_t x0 = h[2 * lane], x1 = h[2 * lane + 1], x2 = lane == 63u ? h[128] : 0u;
        uint32_t inc = x0 + x1 + x2;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(inc, d, 64);
            if ((int)lane >= d) inc += y;
        }
        const uint32_t exc = inc - (x0 + x1 + x2);
        h[2 * lane] = exc; h[2 * lane + 1] = exc + x0;
        if (lane == 63u) { h[128] = exc + x0 + x1; h[129] = inc; }
    }
    __syncthreads();
    if (!mine || lane != 0) return;
    float t = -1.0f;
    int found_bits = 0;
    const int32_t nl = nks[j];
    if (pe) {
        const int32_t nr = nks[j + half];
        const int64_t nfp = java_round((float)(nl > nr ? nl : nr) * fpr);      // Math.max(numLeftKmers, numRightKmers) * covFPR (:4071)
        float tv[2];
        bool fv[2];
        for (int side = 0; side < 2; ++side) {
            int64_t start = (side ? nr : nl) - 1;
            if (start > nfp) start -= nfp;                                      // (:4084-4087)
            fv[side] = false;
            tv[side] = cov_walk(hist[wv][side], start, gradient, false, fv[side]);
        }
        if (fv[0] && fv[1]) t = tv[0] < tv[1] ? tv[0] : tv[1];                  // (:4131-4143)
        else if (fv[0]) { if (tv[0] <= tv[1]) t = tv[0]; }
        else if (fv[1]) { if (tv[1] <= tv[0]) t = tv[1]; }
        found_bits = (fv[0] ? 1 : 0) | (fv[1] ? 2 : 0);
    } else {
        const int64_t start = (int64_t)nl - 1 - java_round((float)nl * fpr);   // (:4019-4020)
        bool f = false;
        if (start >= 0) { const float v = cov_walk(hist[wv][0], start, gradient, true, f); if (f) t = v; }
        found_bits = f ? 1 : 0;
    }
    const bool run = pe ? t >= min_thr : found_bits != 0;                       // (:4145; :4037)
    thr[j] = run ? t : 0.0f;
    if (pe) thr[j + half] = run ? t : 0.0f;
    rb_pairc_rec *rc = recs + (pid ? pid[j] : (int32_t)j);
    if (round == 0) { rc->thr_first = float_bits(t); rc->found_first = found_bits; }
    rc->thr_last = float_bits(t);
    if (!run) { rc->end = RB_PAIRC_END_LOW; live[j] = PC_DONE; }
}

// ---- the end of a round (:4155-4176): a thread per pair of the state adds what the helper did to the pair's record and decides whether the pair
// lives on.  flags / nf / clen / cnk and the gap records are the body's output for the state's sequences.
__global__ void k_pair_commit(int pe, int round, int rounds, int64_t m, const uint32_t *__restrict__ flags, const int32_t *__restrict__ nf,
                              const int32_t *__restrict__ clen, const int32_t *__restrict__ cnk, const int64_t *__restrict__ gof,
                              const rb_corr_gap *__restrict__ gaps, const int32_t *__restrict__ pid, int32_t *__restrict__ live,
                              rb_pairc_rec *__restrict__ recs) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    rb_pairc_rec rc = recs[pid[j]];
    bool changed[2] = {false, false}, lost = false;
    for (int side = 0; side < (pe ? 2 : 1); ++side) {
        const int64_t sq = j + side * m;
        changed[side] = flags[sq] != 0u || nf[sq] > 0;                          // RB_CORR_CORRECTED: the helper returned non-null
        for (int64_t gi = gof[sq]; gi < gof[sq + 1]; ++gi) {
            const uint8_t o = gaps[gi].outcome;
            if (o == RB_GAP_REPLACED) ++rc.gaps_replaced; else if (o == RB_GAP_TRIMMED) ++rc.gaps_trimmed; else ++rc.gaps_kept;
        }
        rc.mismatches += nf[sq];
        lost = lost || cnk[sq] == 0;
    }
    ++rc.rounds_run;
    if (changed[0]) { ++rc.left_changed; rc.flags |= (int32_t)RB_PAIRC_LEFT; }
    if (changed[1]) { ++rc.right_changed; rc.flags |= (int32_t)RB_PAIRC_RIGHT; }
    rc.left_len = clen[j];
    if (pe) rc.right_len = clen[j + m];
    int32_t lv = PC_DONE;
    if (!changed[0] && !changed[1]) rc.end = RB_PAIRC_END_NO_CHANGE;            // (:4174)
    else if (lost) { rc.status = RB_PAIRC_NOT_JUDGED; rc.end = RB_PAIRC_END_LOST_KMERS; lv = PC_LOST; }
    else if (round + 1 >= rounds) rc.end = RB_PAIRC_END_ALL;
    else lv = PC_LIVE;
    recs[pid[j]] = rc;
    live[j] = lv;
}

struct GatherSide {                      // rows of sequences: text, getKmers hashes, counts, thresholds
    uint8_t *txt;
    uint64_t *F, *R;
    float *cnt, *thr;
};
// ---- compaction: a wavefront per item copies a sequence of `len` letters from the source layout into the next round's dense layout — text, both
// hash rows, counts, threshold — or, where dst_k < 0, its text alone into the staging buffer of the finished texts.  tab: seven columns of n items
// (src_t, src_k, dst_t, dst_k, len, src_seq, dst_seq).
__global__ void __launch_bounds__(PC_TPB) k_pair_gather(int k, int64_t n, const int64_t *__restrict__ tab, GatherSide src, GatherSide dst,
                                                        uint8_t *__restrict__ stage) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const int64_t it = (int64_t)blockIdx.x * PC_WAVES + wv;
    if (it >= n) return;
    const int64_t st = tab[it], sk = tab[n + it], dt = tab[2 * n + it], dk = tab[3 * n + it], len = tab[4 * n + it];
    const uint8_t *tx = src.txt + st;
    uint8_t *out = (dk < 0 ? stage : dst.txt) + dt;
    for (int64_t x = lane; x < len; x += 64) out[x] = tx[x];
    if (dk < 0) return;
    const int64_t nk = len >= k ? len - k + 1 : 0;
    for (int64_t x = lane; x < nk; x += 64) {
        dst.F[dk + x] = src.F[sk + x];
        dst.R[dk + x] = src.R[sk + x];
        dst.cnt[dk + x] = src.cnt[sk + x];
    }
    if (lane == 0) dst.thr[tab[6 * n + it]] = src.thr[tab[5 * n + it]];
}

struct Carry {                           // the state between rounds: the live pairs' rows, dense
    DevBuf txt, F, R, cnt, thr;
    GatherSide side() const { return GatherSide{txt.as<uint8_t>(), F.as<uint64_t>(), R.as<uint64_t>(), cnt.as<float>(), thr.as<float>()}; }
};

}  // namespace

extern "C" {
int rb_graph_correct_pairs(rb_graph *g, const char *lseq, const int64_t *loffsets, const char *rseq, const int64_t *roffsets, int64_t n,
                           const rb_pairc_params *p, const int64_t *lout_offsets, char *lout, const int64_t *rout_offsets, char *rout,
                           rb_pairc_rec *recs) {
    return guarded([&] {
        const char *who = "rb_graph_correct_pairs";
        RB_REQUIRE(g && loffsets && p && lout_offsets && n >= 0, "%s: null argument", who);
        const bool pe = roffsets != nullptr;
        RB_REQUIRE(pe ? rout_offsets != nullptr : (!rseq && !rout_offsets && !rout), "%s: the right mates need roffsets and rout_offsets; the single form takes neither rseq nor rout_offsets nor rout", who);
        RB_REQUIRE(n == 0 || (recs && lout && (!pe || rout)), "%s: null argument", who);
        RB_REQUIRE(!g->shard, "%s: not available on a shard handle", who);
        RB_REQUIRE(g->dbg.bits && g->cbf, "%s: dbgbf or the counting filter has been destroyed", who);
        RB_REQUIRE(g->k >= 2, "%s: k = %d (the mismatch pass's median of k - 1 counts needs k >= 2)", who, g->k);
        RB_REQUIRE(std::isfinite(p->max_cov_gradient) && std::isfinite(p->cov_fpr) && std::isfinite(p->min_cov_threshold) &&
                   std::isfinite(p->percent_identity) && std::isfinite(p->min_kmer_cov), "%s: the float parameters must be finite", who);
        RB_REQUIRE(p->max_cov_gradient >= 0.0f, "%s: max_cov_gradient must be >= 0", who);
        RB_REQUIRE(p->cov_fpr >= 0.0f && p->cov_fpr <= 1.0f, "%s: cov_fpr must be in [0, 1]", who);
        RB_REQUIRE(p->lookahead >= 1 && p->lookahead <= 16, "%s: lookahead out of range [1, 16]", who);
        RB_REQUIRE(p->max_indel_size >= 0 && p->max_indel_size <= CE_MAX_INDEL, "%s: max_indel_size out of range [0, %d]", who, CE_MAX_INDEL);
        RB_REQUIRE(p->iterations >= 0, "%s: iterations must be >= 0", who);
        const int k = g->k, max_indel = p->max_indel_size;
        const int sides = pe ? 2 : 1;
        const int rounds = pe ? p->iterations : std::min(p->iterations, 1);        // correctErrorsSE has no loop
        std::vector<int64_t> ko[2];
        ko[0].resize((size_t)n + 1);
        kmer_offsets(loffsets, n, k, ko[0].data(), who);
        if (pe) { ko[1].resize((size_t)n + 1); kmer_offsets(roffsets, n, k, ko[1].data(), who); }
        for (int64_t i = 0; i < n; ++i)
            RB_REQUIRE(lout_offsets[i + 1] >= lout_offsets[i] && (!pe || rout_offsets[i + 1] >= rout_offsets[i]), "%s: decreasing output offsets at %lld", who, (long long)i);
        const int64_t textL = n ? loffsets[n] - loffsets[0] : 0, textR = pe && n ? roffsets[n] - roffsets[0] : 0;
        RB_REQUIRE((textL == 0 || lseq) && (textR == 0 || rseq), "%s: null sequence text", who);
        if (n == 0) return;
        const char *in_seq[2] = {lseq, rseq};
        const int64_t *in_off[2] = {loffsets, roffsets}, *out_off[2] = {lout_offsets, rout_offsets};
        char *out_seq[2] = {lout, rout};
        auto in_len = [&](int side, int64_t i) { return in_off[side][i + 1] - in_off[side][i]; };
        // a final text goes out if it fits; else the overflow bit and nothing written
        auto emit = [&](int64_t i, int side, const char *src, int64_t len) {
            (side ? recs[i].right_len : recs[i].left_len) = (int32_t)len;
            if (len <= out_off[side][i + 1] - out_off[side][i]) { if (len) memmove(out_seq[side] + out_off[side][i], src, (size_t)len); }
            else recs[i].flags |= (int32_t)(side ? RB_PAIRC_RIGHT_OVERFLOW : RB_PAIRC_LEFT_OVERFLOW);
        };
        auto emit_input = [&](int64_t i) { for (int sd = 0; sd < sides; ++sd) emit(i, sd, in_seq[sd] + in_off[sd][i], in_len(sd, i)); };
        const float none = -1.0f;
        uint32_t none_bits;
        memcpy(&none_bits, &none, 4);
        for (int64_t i = 0; i < n; ++i) {
            rb_pairc_rec &rc = recs[i];
            memset(&rc, 0, sizeof(rc));
            rc.status = RB_PAIRC_UNCHANGED; rc.end = RB_PAIRC_END_ALL;
            rc.thr_first = rc.thr_last = none_bits;
        }
        if (rounds == 0) { for (int64_t i = 0; i < n; ++i) emit_input(i); return; }
        // pairs that are over before anything runs: a mate without a k-mer (:4088 throws; the single form returns null, :4007)
        auto no_kmer = [&](int64_t i) {
            for (int sd = 0; sd < sides; ++sd) if (ko[sd][(size_t)i + 1] == ko[sd][(size_t)i]) return true;
            return false;
        };
        std::vector<int64_t> cost((size_t)n + 1, 0);
        for (int64_t i = 0; i < n; ++i) {
            cost[(size_t)i + 1] = cost[(size_t)i];
            if (no_kmer(i)) { recs[i].status = pe ? RB_PAIRC_NOT_JUDGED : RB_PAIRC_UNCHANGED; recs[i].end = RB_PAIRC_END_NO_KMER; }
            else for (int sd = 0; sd < sides; ++sd) cost[(size_t)i + 1] += ko[sd][(size_t)i + 1] - ko[sd][(size_t)i];
        }
        if (cost[(size_t)n] == 0) { for (int64_t i = 0; i < n; ++i) emit_input(i); return; }
        RB_HIP(hipSetDevice(g->p.device));
        HostPin pin_l(lseq + loffsets[0], (size_t)textL), pin_r(pe ? rseq + roffsets[0] : nullptr, (size_t)textR);
        QueryLease q(g);
        hipStream_t s = q.c->st;
        rb_query_ctx &c = *q.c;
        CorrPhaseTimer ph;                                   // (off: the call has one profile entry)
        ph.s = s;
        DevBuf gbuf, wbuf, fixed, gtab, stage;               // the body's gap arrays and walks; records / live / pid / next thresholds; gather table; finished texts
        Carry carry;
        CorrBody body;
        body.g = g; body.c = &c; body.s = s; body.ph = &ph; body.gbuf = &gbuf; body.wbuf = &wbuf; body.who = who;
        body.p = rb_corr_params{p->lookahead, p->max_indel_size, p->percent_identity, p->min_kmer_cov};
        body.own_input = false; body.write_counts = 1;
        std::vector<int64_t> tab, gt, st_kof, st_tof, st_ctof;
        std::vector<uint32_t> woff;
        std::vector<int32_t> len0, live, pid, npid, clen, slen, nslen;
        std::vector<char> fin;                               // the finished texts of the piece, in finishing order
        struct Fin { int64_t pair; int side; int64_t at, len; };
        std::vector<Fin> fins;
        const int64_t piece_dflt = std::max<int64_t>(1, ((int64_t)16 << 20) / (1 + (max_indel + 1) / 2));
        for_each_piece(g, s, [&](int64_t i) { return cost[(size_t)i]; }, n, piece_dflt, "correct_pairs", [&](Piece &pc) {
            const int64_t ra = pc.ra, pn = pc.pn, ns = sides * pn;
            if (cost[(size_t)pc.rb] == cost[(size_t)ra]) { for (int64_t i = ra; i < pc.rb; ++i) emit_input(i); return; }
            // ---- the piece's text and its getKmers rows: sequences [0, pn) the left mates, [pn, 2 pn) the right ones
            tab.assign((size_t)(2 * ns + 2), 0);             // tof [ns + 1], kof [ns + 1]
            woff.assign((size_t)ns + 1, 0);
            len0.assign((size_t)ns, 0);
            int64_t *t_tof = tab.data(), *t_kof = t_tof + ns + 1;
            for (int sd = 0; sd < sides; ++sd)
                for (int64_t i = 0; i < pn; ++i) {
                    const int64_t q_ = sd * pn + i, l = in_len(sd, ra + i);
                    RB_REQUIRE(l <= INT32_MAX, "%s: sequence too long", who);
                    len0[(size_t)q_] = (int32_t)l;
                    t_tof[q_ + 1] = t_tof[q_] + l;
                    t_kof[q_ + 1] = t_kof[q_] + (ko[sd][(size_t)(ra + i) + 1] - ko[sd][(size_t)(ra + i)]);
                    woff[(size_t)q_ + 1] = woff[(size_t)q_] + (uint32_t)((l + 31) / 32);
                }
            const int64_t tb = t_tof[ns], pt = t_kof[ns];
            RB_REQUIRE(pt < ((int64_t)1 << 40) && (int64_t)woff[(size_t)ns] * 32 < ((int64_t)1 << 36), "%s: piece too large", who);
            const size_t tab_bytes = up16(tab.size() * 8);
            c.b0.reserve(tab_bytes + woff.size() * 4 + 16);
            c.b1.reserve((size_t)pt * 8 + 16);
            c.b2.reserve((size_t)pt * 8 + 16);
            uint8_t *i_txt; float *i_cnt, *i_thr; int32_t *i_len, *i_nk; uint32_t *i_valid;
            auto lay0 = [&](Arena &a) {
                i_txt = a.take<uint8_t>((size_t)tb); i_cnt = a.take<float>((size_t)pt); i_thr = a.take<float>((size_t)ns);
                i_len = a.take<int32_t>((size_t)ns); i_nk = a.take<int32_t>((size_t)ns); i_valid = a.take<uint32_t>((size_t)woff[(size_t)ns] + 1);
            };
            Arena a0;
            lay0(a0);
            c.b3.reserve(a0.at + 64);
            a0.base = c.b3.as<uint8_t>(); a0.at = 0;
            lay0(a0);
            // the call's own arrays of the piece: records, live flags, the state's pair ids [pn each], the next round's thresholds [ns]
            rb_pairc_rec *d_recs; int32_t *d_live, *d_pid; float *d_thr_next;
            auto layf = [&](Arena &a) {
                d_recs = a.take<rb_pairc_rec>((size_t)pn); d_live = a.take<int32_t>((size_t)pn); d_pid = a.take<int32_t>((size_t)pn);
                d_thr_next = a.take<float>((size_t)ns);
            };
            Arena af;
            layf(af);
            fixed.reserve(af.at + 64);
            af.base = fixed.as<uint8_t>(); af.at = 0;
            layf(af);
            uint8_t *b0 = c.b0.as<uint8_t>();
            const int64_t *d_tof = reinterpret_cast<const int64_t *>(b0), *d_kof = d_tof + ns + 1;
            const uint32_t *d_woff = reinterpret_cast<const uint32_t *>(b0 + tab_bytes);
            std::vector<int32_t> nk0((size_t)ns);
            for (int64_t q_ = 0; q_ < ns; ++q_) nk0[(size_t)q_] = (int32_t)(t_kof[q_ + 1] - t_kof[q_]);
            live.assign((size_t)pn, PC_LIVE);
            pid.resize((size_t)pn);
            for (int64_t i = 0; i < pn; ++i) { pid[(size_t)i] = (int32_t)i; if (no_kmer(ra + i)) live[(size_t)i] = PC_DONE; }
            RB_HIP(hipMemcpyAsync(b0, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
            RB_HIP(hipMemcpyAsync(b0 + tab_bytes, woff.data(), woff.size() * 4, hipMemcpyHostToDevice, s));
            for (int sd = 0; sd < sides; ++sd) {
                const int64_t l = in_off[sd][pc.rb] - in_off[sd][ra];
                if (l) RB_HIP(hipMemcpyAsync(i_txt + t_tof[sd * pn], in_seq[sd] + in_off[sd][ra], (size_t)l, hipMemcpyHostToDevice, s));
            }
            RB_HIP(hipMemcpyAsync(i_len, len0.data(), (size_t)ns * 4, hipMemcpyHostToDevice, s));
            RB_HIP(hipMemcpyAsync(i_nk, nk0.data(), (size_t)ns * 4, hipMemcpyHostToDevice, s));
            RB_HIP(hipMemcpyAsync(d_recs, recs + ra, (size_t)pn * sizeof(rb_pairc_rec), hipMemcpyHostToDevice, s));
            RB_HIP(hipMemcpyAsync(d_live, live.data(), (size_t)pn * 4, hipMemcpyHostToDevice, s));
            RB_HIP(hipMemcpyAsync(d_pid, pid.data(), (size_t)pn * 4, hipMemcpyHostToDevice, s));
            pc.kernels_begin();
            launch_text_kmers(g, ns, d_tof, d_kof, d_woff, i_txt, i_len, i_valid, c.b1.as<uint64_t>(), c.b2.as<uint64_t>(), i_cnt, s);
            hipLaunchKernelGGL(k_pair_threshold, dim3(blocks_for(pn, PC_WAVES)), dim3(PC_TPB), 0, s, pe ? 1 : 0, 0, p->max_cov_gradient, p->cov_fpr,
                               p->min_cov_threshold, pn, pn, d_kof, i_nk, i_cnt, (const int32_t *)nullptr, d_live, i_thr, d_recs);
            RB_HIP(hipGetLastError());
            // ---- the rounds.  The source of a gather is the initial profile, then the body's output; m pairs are in the state
            GatherSide src{i_txt, c.b1.as<uint64_t>(), c.b2.as<uint64_t>(), i_cnt, i_thr};
            std::vector<int64_t> src_tof(t_tof, t_tof + ns), src_kof(t_kof, t_kof + ns);   // (tab is the body's to overwrite)
            slen = len0;
            int64_t m = pn;
            fin.clear(); fins.clear();
            for (int round = 0;; ++round) {
                RB_HIP(hipMemcpyAsync(live.data(), d_live, (size_t)m * 4, hipMemcpyDeviceToHost, s));
                RB_HIP(hipStreamSynchronize(s));
                // the next state: the pairs that enter round `round`; behind round 0, the finished pairs' texts go to the staging buffer
                int64_t m2 = 0;
                for (int64_t j = 0; j < m; ++j) if (live[(size_t)j] == PC_LIVE) ++m2;
                std::vector<int64_t> items;                  // (state sequence, destination sequence or -1)
                npid.assign((size_t)m2, 0);
                nslen.assign((size_t)(sides * m2), 0);
                int64_t stage_bytes = 0;
                const size_t fin_at = fin.size();
                {
                    int64_t d = 0;
                    for (int64_t j = 0; j < m; ++j) {
                        const int32_t lv = live[(size_t)j];
                        if (lv == PC_LIVE) {
                            npid[(size_t)d] = pid[(size_t)j];
                            for (int sd = 0; sd < sides; ++sd) { nslen[(size_t)(sd * m2 + d)] = slen[(size_t)(sd * m + j)]; items.push_back(sd * m + j); items.push_back(sd * m2 + d); }
                            ++d;
                        } else if (round > 0 && lv == PC_DONE) {
                            for (int sd = 0; sd < sides; ++sd) {
                                items.push_back(sd * m + j); items.push_back(-1);
                                fins.push_back(Fin{ra + pid[(size_t)j], sd, (int64_t)fin_at + stage_bytes, slen[(size_t)(sd * m + j)]});
                                stage_bytes += slen[(size_t)(sd * m + j)];
                            }
                        }
                    }
                }
                const int64_t ns2 = sides * m2, ni = (int64_t)items.size() / 2;
                st_tof.assign((size_t)ns2 + 1, 0); st_kof.assign((size_t)ns2 + 1, 0); st_ctof.assign((size_t)ns2 + 1, 0);
                for (int64_t q_ = 0; q_ < ns2; ++q_) {
                    const int64_t l = nslen[(size_t)q_];
                    st_tof[(size_t)q_ + 1] = st_tof[(size_t)q_] + l;
                    st_kof[(size_t)q_ + 1] = st_kof[(size_t)q_] + (l >= k ? l - k + 1 : 0);
                    st_ctof[(size_t)q_ + 1] = st_ctof[(size_t)q_] + corr_capacity(l, k, max_indel);
                }
                if (ni > 0) {
                    gt.assign((size_t)(7 * ni), 0);
                    int64_t so = 0;
                    for (int64_t it = 0; it < ni; ++it) {
                        const int64_t sq = items[(size_t)(2 * it)], dq = items[(size_t)(2 * it + 1)], l = slen[(size_t)sq];
                        gt[(size_t)it] = src_tof[(size_t)sq]; gt[(size_t)(ni + it)] = src_kof[(size_t)sq];
                        gt[(size_t)(2 * ni + it)] = dq >= 0 ? st_tof[(size_t)dq] : so;
                        gt[(size_t)(3 * ni + it)] = dq >= 0 ? st_kof[(size_t)dq] : -1;
                        gt[(size_t)(4 * ni + it)] = l; gt[(size_t)(5 * ni + it)] = sq; gt[(size_t)(6 * ni + it)] = dq >= 0 ? dq : 0;
                        if (dq < 0) so += l;
                    }
                    gtab.reserve(gt.size() * 8 + 16);
                    stage.reserve((size_t)stage_bytes + 16);
                    // (the state of the last round is dead: the body that read it has run, and reserve() waits for the device before it frees)
                    carry.txt.reserve((size_t)st_tof[(size_t)ns2] + 16);
                    carry.F.reserve((size_t)st_kof[(size_t)ns2] * 8 + 16); carry.R.reserve((size_t)st_kof[(size_t)ns2] * 8 + 16);
                    carry.cnt.reserve((size_t)st_kof[(size_t)ns2] * 4 + 16); carry.thr.reserve((size_t)ns2 * 4 + 16);
                    RB_HIP(hipMemcpyAsync(gtab.p, gt.data(), gt.size() * 8, hipMemcpyHostToDevice, s));
                    hipLaunchKernelGGL(k_pair_gather, dim3(blocks_for(ni, PC_WAVES)), dim3(PC_TPB), 0, s, k, ni, gtab.as<int64_t>(), src, carry.side(),
                                       stage.as<uint8_t>());
                    RB_HIP(hipGetLastError());
                    if (stage_bytes) {
                        fin.resize(fin_at + (size_t)stage_bytes);
                        RB_HIP(hipMemcpyAsync(fin.data() + fin_at, stage.p, (size_t)stage_bytes, hipMemcpyDeviceToHost, s));
                        RB_HIP(hipStreamSynchronize(s));     // (fin may move when it grows again)
                    }
                }
                if (m2 == 0) break;
                m = m2; pid.swap(npid); slen.swap(nslen);
                RB_HIP(hipMemcpyAsync(d_pid, pid.data(), (size_t)m * 4, hipMemcpyHostToDevice, s));
                // ---- the helper on the state
                body.prepare(sides * m, st_kof.data(), st_tof.data(), st_ctof.data());
                const GatherSide in = carry.side();
                body.dtxt = in.txt; body.dFin = in.F; body.dRin = in.R; body.dcnt = in.cnt; body.dthr = in.thr;
                body.run();
                hipLaunchKernelGGL(k_pair_commit, dim3(blocks_for(m)), dim3(TPB), 0, s, pe ? 1 : 0, round, rounds, m, body.dflags, body.dnf, body.dclen, body.dcnk,
                                   body.dgof, body.drecs, d_pid, d_live, d_recs);
                RB_HIP(hipGetLastError());
                if (round + 1 < rounds) {
                    hipLaunchKernelGGL(k_pair_threshold, dim3(blocks_for(m, PC_WAVES)), dim3(PC_TPB), 0, s, pe ? 1 : 0, round + 1, p->max_cov_gradient, p->cov_fpr,
                                       p->min_cov_threshold, m, m, body.dckof, body.dcnk, body.dcnt2, d_pid, d_live, d_thr_next, d_recs);
                    RB_HIP(hipGetLastError());
                }
                clen.resize((size_t)(sides * m));
                uint32_t over = 0;
                RB_HIP(hipMemcpyAsync(clen.data(), body.dclen, (size_t)(sides * m) * 4, hipMemcpyDeviceToHost, s));
                RB_HIP(hipMemcpyAsync(&over, body.dover, 4, hipMemcpyDeviceToHost, s));
                RB_HIP(hipStreamSynchronize(s));
                if (over) {
                    set_error("%s: %u sequences of pairs [%lld, %lld) outgrew their slots (internal error)", who, over, (long long)ra, (long long)pc.rb);
                    throw HipError{RB_ERR_STATE};
                }
                slen = clen;
                src = GatherSide{body.dctxt, body.dF, body.dR, body.dcnt2, d_thr_next};
                src_tof.assign(body.h_ctof(), body.h_ctof() + sides * m);
                src_kof.assign(body.h_ckof(), body.h_ckof() + sides * m);
            }
            pc.kernels_end();
            RB_HIP(hipMemcpyAsync(recs + ra, d_recs, (size_t)pn * sizeof(rb_pairc_rec), hipMemcpyDeviceToHost, s));
            pc.finish();
            // ---- the final texts: staged ones where a round ran and the pair was judged, the input everywhere else
            std::vector<uint8_t> staged((size_t)pn, 0);
            for (const Fin &f : fins)
                if (recs[f.pair].status != RB_PAIRC_NOT_JUDGED) { staged[(size_t)(f.pair - ra)] = 1; emit(f.pair, f.side, fin.data() + f.at, f.len); }
            for (int64_t i = ra; i < pc.rb; ++i) {
                rb_pairc_rec &rc = recs[i];
                if (!staged[(size_t)(i - ra)]) emit_input(i);
                if (rc.status != RB_PAIRC_NOT_JUDGED)
                    rc.status = (rc.flags & (int32_t)(RB_PAIRC_LEFT | RB_PAIRC_RIGHT)) ? RB_PAIRC_CORRECTED : RB_PAIRC_UNCHANGED;
            }
        });
    });
}
}  // extern "C"
