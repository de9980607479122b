// rb_long_prepare.hip — what LongReadCorrectionWorker.run does to a raw read before it makes a segment (rb_long_prepare; R/RNABloom.java:3700-3779):
// the reverse complement where asked, PolyATailFinder.findPolyATail / findPolyTHead (R/util/PolyATailFinder.java:201-277, 319-338, 355-432,
// 476-495), the five-way rule that cuts and turns the read, SeqUtils.trimLowComplexityRegions (R/util/SeqUtils.java:839-902) over
// isLowComplexityLong (:585-659) and isLowComplexityLongWindowed (:661-682), and hasPolyA.  Text work on the raw bytes, no graph: a wavefront
// per read (DESIGN.md §5 "Preparation of long reads").
//   The finder's scans are wave_first / wave_last over the positions of a search range: a lane decides its position from the letters of the
// seed window that starts there, so the sliding count of the reference and its early break become three scans (the highest position where a
// region opens, the first position below it where the identity fails, the lowest letter in between that is an A).  The poly-T head is the
// same code on the mirrored read; the two places where the reference's two forms are NOT mirror images are kept (LpEnd::MIR).
//   The complexity pass has the lanes across a window's letters: lane l takes letters l, l + 64, ... of the window and adds its letter, pair and
// triple to the window's 84 counters in LDS (ds_add); 84 lanes' worth of comparisons on the final counts decide (the counters only grow, so the
// reference's early return sees nothing the final counts do not).  Nothing of the read is staged, so a read of any length works; a read's windows
// are taken one after the other, and the segments come out of the run of window verdicts as they are made.
#include "rb_wave.hpp"
#include "rb_pieces.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

constexpr int LP_TPB = 256;
constexpr int LP_WAVES = LP_TPB / 64;       // reads a workgroup works on at a time: a wavefront each
constexpr int LP_NCTR = 4 + 16 + 64;        // nf1, nf2, nf3 of isLowComplexityLong
constexpr unsigned LP_MAX_BLOCKS = 1u << 16;

struct LpArgs {
    const uint8_t *txt;          // the piece's letters
    const int64_t *tab;          // toff[pn + 1], then soff[pn + 1]: letter and segment-slot offsets inside the piece
    int64_t pn;
    int32_t *recs;               // 16 ints a read
    int32_t *segs;               // 2 ints a slot
    uint8_t *out;                // the transformed reads at toff, or nullptr
    int min_len, rc, stranded, polya, seed, thr, max_gap, window, lc_window, lc_min_length;
    float min_identity;
};

// SeqUtils.reverseComplement's letter map (:1130-1148): lower case and everything else is N
__device__ __forceinline__ uint8_t lp_comp(uint8_t c) {
    return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : (c == 'T' || c == 'U') ? 'A' : 'N';
}
// nucleotideArrayIndex (:315-330)
__device__ __forceinline__ int lp_idx(uint8_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : (c == 'T' || c == 'U') ? 3 : -1; }

// the read as the finder sees it: the raw letters, or their reverse complement where the call asks for it
struct LpRead {
    const uint8_t *x;
    int len, rc;
    __device__ __forceinline__ uint8_t at(int j) const { return rc ? lp_comp(x[len - 1 - j]) : x[j]; }
};
// the transformed read: letters [a, b) of the finder's read, reverse-complemented (once more) where the head rule turned it
struct LpText {
    LpRead r;
    int a, b, turned;
    __device__ __forceinline__ int size() const { return b - a; }
    __device__ __forceinline__ uint8_t at(int i) const { return turned ? lp_comp(r.at(b - 1 - i)) : r.at(a + i); }
};

// One end of the finder's read in the coordinates of findPolyASeed: the read itself and the letters A a for the tail; for the head (MIR) the
// mirrored read — position p is letter len - 1 - p — and the letters T t, so that findPolyTSeed's scan to the right is the same scan downwards.
template <bool MIR> struct LpEnd {
    LpRead r;
    __device__ __forceinline__ bool hit(int p) const {
        const uint8_t c = r.at(MIR ? r.len - 1 - p : p);
        return MIR ? (c == 'T' || c == 't') : (c == 'A' || c == 'a');
    }
};

// findPolyASeed / findPolyTSeed over [s, e): true and the region [rs, re), or false (null).  thr: the smallest count of a seed window that
// passes `count / (float) seedLength >= minIdentity`.  All lanes call, all get the result.
template <bool MIR> __device__ bool lp_seed(const LpEnd<MIR> &en, int s, int e, int seed, int thr, int &rs, int &re, uint32_t lane) {
    if (!(s < e && s >= 0 && e - s >= seed)) return false;
    const int i0 = e - seed;
    auto pass = [&](int i) { int c = 0; for (int q = 0; q < seed; ++q) c += en.hit(i + q) ? 1 : 0; return c >= thr; };
    // the region opens at the first window of the scan that passes and, below the topmost one, starts with the letter
    const int ic = wave_last(s, i0 + 1, [&](int i) { return (i == i0 || en.hit(i)) && pass(i); }, lane);
    if (ic < s) return false;
    // the scan stops at the first window below it that fails; the region starts at the lowest letter above that stop
    const int stop = wave_last(s, ic, [&](int i) { return !pass(i); }, lane);
    int start = wave_first(stop + 1, ic, [&](int i) { return en.hit(i); }, lane);
    int end = ic + seed + (MIR && ic != i0 ? 1 : 0);            // (findPolyTSeed opens its region one letter longer: Interval(i - seedLength, i + 1))
    // refine: other letters leave the far end while the region is longer than the seed ...
    end = wave_last(start + seed, end, [&](int i) { return en.hit(i); }, lane) + 1;
    // ... and a region that starts where the search did walks on: the tail's start while seq[start] is an A (it ends ON the other letter, or at
    // 0), the head's end while the letter behind it is a T
    if (start == s) {
        if (MIR) start = wave_last(0, start, [&](int i) { return !en.hit(i); }, lane) + 1;
        else start = wave_last(1, start + 1, [&](int i) { return !en.hit(i); }, lane);
    }
    rs = start; re = end;
    return true;
}

// findPolyATail / findPolyTHead: the chain of seed searches towards the inside of the read
template <bool MIR> __device__ bool lp_chain(const LpEnd<MIR> &en, const LpArgs &a, int &bs, int &be, int &searches, uint32_t lane) {
    int s_end = en.r.len, s_start = max(0, s_end - a.window);
    searches = 1;
    const bool have = lp_seed(en, s_start, s_end, a.seed, a.thr, bs, be, lane);
    while (have && s_start > 0) {
        s_end = bs; s_start = max(0, s_end - a.window);
        int ps = 0, pe = 0;
        ++searches;
        if (!lp_seed(en, s_start, s_end, a.seed, a.thr, ps, pe, lane)) break;
        bool join = pe + a.max_gap >= bs;
        if (!join) {                                            // percentA / percentT of the letters between them (pe < bs here)
            int c = 0;
            for (int p = pe + (int)lane; p < bs; p += 64) c += en.hit(p) ? 1 : 0;
            for (int sh = 32; sh > 0; sh >>= 1) c += __shfl_xor(c, sh, 64);
            join = (float)c / (float)(bs - pe) >= a.min_identity;
        }
        if (!join) break;
        bs = ps;
    }
    return have;
}

// isLowComplexityLong of letters [start, start + len) of the transformed read, on the final counts.  cnt: the wavefront's 84 counters in LDS.
__device__ bool lp_is_low(const LpText &t, int start, int len, uint32_t *cnt, uint32_t lane) {
    if (len <= 6) return false;
    const float f = (float)len * 0.89f;
    const uint32_t t1 = (uint32_t)java_round(f), t2 = (uint32_t)java_round(f / 2.0f), t3 = (uint32_t)java_round(f / 3.0f);
    for (int c = (int)lane; c < LP_NCTR; c += 64) cnt[c] = 0;
    wave_fence();
    for (int p = (int)lane; p < len; p += 64) {
        const int c1 = lp_idx(t.at(start + p));
        if (c1 >= 0) atomicAdd(&cnt[c1], 1u);
        if (p < 2) continue;
        const int c2 = lp_idx(t.at(start + p - 1)), c3 = lp_idx(t.at(start + p - 2));
        if (c3 == c2 && c2 == c1) continue;                     // three equal letters (or three that are none) count no pair and no triple
        if (c2 >= 0 && c1 >= 0) atomicAdd(&cnt[4 + c2 * 4 + c1], 1u);
        if (p == 2 && c3 >= 0 && c2 >= 0) atomicAdd(&cnt[4 + c3 * 4 + c2], 1u);      // the first pair goes with the first triple
        if (c3 >= 0 && c2 >= 0 && c1 >= 0) atomicAdd(&cnt[20 + c3 * 16 + c2 * 4 + c1], 1u);
    }
    wave_fence();
    bool low = false;
    for (int c = (int)lane; c < LP_NCTR; c += 64) low = low || cnt[c] >= (c < 4 ? t1 : c < 20 ? t2 : t3);
    if (lane < 16) {
        const int i = (int)lane >> 2, j = (int)lane & 3;
        if (i < j) low = low || cnt[i] + cnt[j] >= t1;          // the six pairs of letters
        const uint32_t count = cnt[4 + lane];                    // two dinucleotides (:645-656)
        for (int k = i; k < 4; ++k)
            for (int l = j; l < 4; ++l) low = low || ((i != k || j != l) && count + cnt[4 + k * 4 + l] >= t2);
    }
    const bool res = __ballot(low) != 0ull;
    wave_fence();                                               // (the next window clears the counters)
    return res;
}

__global__ void __launch_bounds__(LP_TPB) k_long_prepare(LpArgs a) {
    __shared__ uint32_t s_cnt[LP_WAVES][LP_NCTR + 12];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t *cnt = s_cnt[wave];
    const int64_t *toff = a.tab, *soff = a.tab + a.pn + 1;
    for (int64_t rd = (int64_t)blockIdx.x * LP_WAVES + wave; rd < a.pn; rd += (int64_t)gridDim.x * LP_WAVES) {
        const int len = (int)(toff[rd + 1] - toff[rd]);
        const int64_t slots = soff[rd + 1] - soff[rd];
        const int room = slots > INT32_MAX ? INT32_MAX : (int)slots;
        int32_t *rec = a.recs + rd * 16, *seg = a.segs + 2 * soff[rd];
        int status = RB_PREP_SHORT, flags = 0, kb = 0, ke = 0, ts = -1, te = -1, hs = -1, he = -1, nwin = 0, nlow = 0, off = 0, nseg = 0, tsearch = 0, hsearch = 0;
        if (len >= a.min_len) {
            const LpRead r{a.txt + toff[rd], len, a.rc};
            // ---- the tail, the head and the five-way rule (:3715-3766) ----
            LpText t{r, 0, len, 0};
            bool polya = false;
            if (a.polya) {
                const bool tail = lp_chain(LpEnd<false>{r}, a, ts, te, tsearch, lane);
                if (!tail) ts = te = -1;
                if (a.stranded) {
                    if (tail && te < len) { t.b = te; polya = true; }
                } else {
                    int ms = 0, me = 0;
                    const bool head = lp_chain(LpEnd<true>{r}, a, ms, me, hsearch, lane);
                    if (head) { hs = len - me; he = len - ms; }
                    if (tail && !head) { if (te < len) t.b = te; polya = true; }
                    else if (!tail && head) { t.a = hs; t.turned = 1; polya = true; }
                    else if (tail && head && he < ts) { t.a = he; t.b = ts; }
                }
                flags |= (ts >= 0 ? RB_PREP_TAIL_FOUND : 0) | (hs >= 0 ? RB_PREP_HEAD_FOUND : 0);
            }
            const int n = t.size();
            kb = a.rc ? len - t.b : t.a; ke = a.rc ? len - t.a : t.b;
            if ((a.rc != 0) != (t.turned != 0)) flags |= RB_PREP_REVCOMP;
            if (a.rc && t.turned) flags |= RB_PREP_MAPPED_TWICE;
            if (a.out) for (int i = (int)lane; i < n; i += 64) a.out[toff[rd] + i] = t.at(i);
            // ---- trimLowComplexityRegions(seq, lc_window, lc_min_length) ----
            const int ws = a.lc_window;
            if (n / ws >= 5) {
                flags |= RB_PREP_ROUTE_WINDOWS;
                nwin = n / ws; off = (n % ws) / 2;
                int run = -1, run_end = -1;
                auto put = [&](int b, int e) { if (lane == 0 && nseg < room) { seg[2 * nseg] = b; seg[2 * nseg + 1] = e; } ++nseg; };
                for (int w = 0; w < nwin; ++w) {
                    if (!lp_is_low(t, w * ws + off, ws, cnt, lane)) { if (run < 0) run = w; run_end = w; }
                    else {
                        ++nlow;
                        if (run >= 0) put(run == 0 ? 0 : off + run * ws, off + (run_end + 1) * ws);
                        run = -1;
                    }
                }
                if (run >= 0) put(run == 0 ? 0 : off + run * ws, n);
                if ((int64_t)nlow * ws >= (int64_t)a.lc_min_length) flags |= RB_PREP_CUT_FIRED;
                else { nseg = 0; put(0, n); }                   // the cut does not fire: the read is one segment
            } else {
                bool low;
                if (n / 50 >= 4) {                              // isLowComplexityLongWindowed
                    flags |= RB_PREP_ROUTE_WINDOWED;
                    nwin = n / 50; off = (n % 50) / 2;
                    for (int w = 0; w < nwin; ++w) nlow += lp_is_low(t, w * 50 + off, 50, cnt, lane) ? 1 : 0;
                    low = nlow >= (3 * nwin) / 4;               // floor(0.75 * numWindows)
                } else {
                    flags |= RB_PREP_ROUTE_WHOLE;
                    low = lp_is_low(t, 0, n, cnt, lane);
                    nlow = low ? 1 : 0;
                }
                if (!low) { if (lane == 0 && room > 0) { seg[0] = 0; seg[1] = n; } nseg = 1; }
            }
            status = nseg ? RB_PREP_SEGMENTS : RB_PREP_LOW_COMPLEXITY;
            if (polya && nseg <= 1) flags |= RB_PREP_HAS_POLYA;    // several segments clear it (:3777-3779)
        }
        if (lane == 0) {
            rec[0] = status; rec[1] = flags; rec[2] = kb; rec[3] = ke; rec[4] = ts; rec[5] = te; rec[6] = hs; rec[7] = he;
            rec[8] = nwin; rec[9] = nlow; rec[10] = off; rec[11] = nseg; rec[12] = tsearch; rec[13] = hsearch; rec[14] = 0; rec[15] = 0;
        }
    }
}

// the smallest count c of a seed window with c / (float) seedLength >= minIdentity (findPolyASeed's test, once a call instead of once a letter)
int seed_threshold(int seed, float min_identity) {
    int lo = 0, hi = seed;                                      // (seed / seed = 1 >= min_identity; the quotient grows with c)
    while (lo < hi) { const int mid = lo + (hi - lo) / 2; if ((float)mid / (float)seed >= min_identity) hi = mid; else lo = mid + 1; }
    return lo;
}

int64_t prep_room(int64_t len, int lc_window) { return std::max<int64_t>(1, (len / lc_window + 1) / 2); }

void prepare_call(int device, const char *seq, const int64_t *offsets, int64_t n, const rb_prep_params *p, const int64_t *seg_offsets, rb_prep_rec *recs,
                  int32_t *out_segs, char *out_seq, double *kernel_ms) {
    const char *who = "rb_long_prepare";
    RB_REQUIRE(p, "%s: null params", who);
    RB_REQUIRE(n >= 0, "%s: n = %lld", who, (long long)n);
    RB_REQUIRE(p->min_len >= 0, "%s: min_len = %d", who, p->min_len);
    RB_REQUIRE(p->seed_length >= 1, "%s: seed_length = %d (>= 1)", who, p->seed_length);
    RB_REQUIRE(p->min_identity > 0.0f && p->min_identity <= 1.0f, "%s: min_identity = %g (0 < min_identity <= 1)", who, (double)p->min_identity);
    RB_REQUIRE(p->max_gap >= 0 && p->max_gap <= (1 << 30), "%s: max_gap = %d (0 .. 2^30)", who, p->max_gap);
    RB_REQUIRE(p->window >= 0, "%s: window = %d", who, p->window);
    RB_REQUIRE(p->lc_window >= 1 && p->lc_window <= RB_PREP_MAX_LC_WINDOW, "%s: lc_window = %d (1 .. %d)", who, p->lc_window, RB_PREP_MAX_LC_WINDOW);
    RB_REQUIRE(p->lc_min_length >= 0, "%s: lc_min_length = %d", who, p->lc_min_length);
    if (n == 0) { if (kernel_ms) *kernel_ms = 0; return; }
    RB_REQUIRE(offsets && seg_offsets && recs && out_segs, "%s: null argument (offsets, seg_offsets, recs and out_segs are needed for n > 0)", who);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t l = offsets[i + 1] - offsets[i];
        RB_REQUIRE(l >= 0, "%s: offsets[%lld] > offsets[%lld]", who, (long long)i, (long long)i + 1);
        RB_REQUIRE(l <= (1 << 30), "%s: read %lld has %lld letters, more than 2^30", who, (long long)i, (long long)l);
    }
    for (int64_t i = 0; i < n; ++i) {
        const int64_t l = offsets[i + 1] - offsets[i], room = seg_offsets[i + 1] - seg_offsets[i];
        RB_REQUIRE(room >= prep_room(l, p->lc_window), "%s: seg_offsets gives read %lld (%lld letters) room for %lld segments, it may have %lld", who,
                   (long long)i, (long long)l, (long long)room, (long long)prep_room(l, p->lc_window));
    }
    RB_REQUIRE(offsets[n] == offsets[0] || seq, "%s: null sequence text", who);
    if (kernel_ms) *kernel_ms = 0;
    RB_HIP(hipSetDevice(device));
    LpArgs a{};
    a.min_len = p->min_len; a.rc = p->reverse_complement != 0; a.stranded = p->strand_specific != 0; a.polya = p->polya != 0;
    a.seed = p->seed_length; a.thr = seed_threshold(p->seed_length, p->min_identity); a.max_gap = p->max_gap;
    a.window = std::max(p->seed_length, p->window);             // PolyATailFinder.setWindow
    a.lc_window = p->lc_window; a.lc_min_length = p->lc_min_length; a.min_identity = p->min_identity;
    Stream st;
    RB_HIP(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    Event ev[2];
    if (kernel_ms) for (Event &e : ev) RB_HIP(hipEventCreate(&e.e));
    HostPin pin_in(seq ? seq + offsets[0] : nullptr, (size_t)(offsets[n] - offsets[0]));
    DevBuf b_txt, b_tab, b_rec, b_seg, b_out;
    std::vector<int64_t> tab;
    std::vector<int32_t> segs_host;
    HostBuf<uint8_t> out_host;                                  // pinned: the texts come back at link speed, then go read by read to the caller
    // piece by piece, cut by letters (RB_QUERY_PIECE counts letters here): 64 M letters a piece
    const std::vector<int64_t> cut = piece_cuts_by_cost([&](int64_t i) { return offsets[i + 1] - offsets[i]; }, n, query_piece_max((int64_t)64 << 20));
    if (out_seq) {
        int64_t most = 0;
        for (size_t c = 0; c + 1 < cut.size(); ++c) most = std::max(most, offsets[cut[c + 1]] - offsets[cut[c]]);
        if (most) out_host.alloc((size_t)most);
    }
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        const int64_t ra = cut[c], rb_ = cut[c + 1], pn = rb_ - ra, tb = offsets[rb_] - offsets[ra], sb = seg_offsets[rb_] - seg_offsets[ra];
        tab.resize(2 * (size_t)pn + 2);
        for (int64_t i = 0; i <= pn; ++i) { tab[(size_t)i] = offsets[ra + i] - offsets[ra]; tab[(size_t)(pn + 1 + i)] = seg_offsets[ra + i] - seg_offsets[ra]; }
        b_txt.reserve((size_t)tb + 16); b_tab.reserve(tab.size() * 8); b_rec.reserve((size_t)pn * sizeof(rb_prep_rec)); b_seg.reserve((size_t)sb * 8 + 16);
        if (out_seq) b_out.reserve((size_t)tb + 16);
        if (tb) RB_HIP(hipMemcpyAsync(b_txt.p, seq + offsets[ra], (size_t)tb, hipMemcpyHostToDevice, st));
        RB_HIP(hipMemcpyAsync(b_tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, st));
        a.txt = b_txt.as<uint8_t>(); a.tab = b_tab.as<int64_t>(); a.pn = pn;
        a.recs = b_rec.as<int32_t>(); a.segs = b_seg.as<int32_t>(); a.out = out_seq ? b_out.as<uint8_t>() : nullptr;
        if (kernel_ms) RB_HIP(hipEventRecord(ev[0], st));
        hipLaunchKernelGGL(k_long_prepare, dim3(std::min(blocks_for(pn, LP_WAVES), LP_MAX_BLOCKS)), dim3(LP_TPB), 0, st, a);
        RB_HIP(hipGetLastError());
        if (kernel_ms) RB_HIP(hipEventRecord(ev[1], st));
        segs_host.resize(2 * (size_t)sb);
        RB_HIP(hipMemcpyAsync(recs + ra, b_rec.p, (size_t)pn * sizeof(rb_prep_rec), hipMemcpyDeviceToHost, st));
        RB_HIP(hipMemcpyAsync(segs_host.data(), b_seg.p, (size_t)sb * 8, hipMemcpyDeviceToHost, st));
        if (out_seq && tb) RB_HIP(hipMemcpyAsync(out_host.p, b_out.p, (size_t)tb, hipMemcpyDeviceToHost, st));
        RB_HIP(hipStreamSynchronize(st));
        if (kernel_ms) { float ms = 0; RB_HIP(hipEventElapsedTime(&ms, ev[0], ev[1])); *kernel_ms += ms; }
        // only what a read has comes back to the caller's arrays: its segments, and the letters of its transformed text
        for (int64_t i = 0; i < pn; ++i) {
            const rb_prep_rec &rc = recs[ra + i];
            const int64_t room = seg_offsets[ra + i + 1] - seg_offsets[ra + i];
            if (rc.n_segments > room) {
                set_error("%s: read %lld has %d segments, more than its %lld slots (internal error)", who, (long long)(ra + i), rc.n_segments, (long long)room);
                throw HipError{RB_ERR_STATE};
            }
            if (rc.n_segments) memcpy(out_segs + 2 * seg_offsets[ra + i], segs_host.data() + 2 * tab[(size_t)(pn + 1 + i)], (size_t)rc.n_segments * 8);
            if (out_seq && rc.status != RB_PREP_SHORT && rc.kept_end > rc.kept_begin)
                memcpy(out_seq + offsets[ra + i], out_host.p + tab[(size_t)i], (size_t)(rc.kept_end - rc.kept_begin));
        }
    }
}

}  // namespace
}  // namespace rb

extern "C" {
int rb_long_prepare(int device, const char *seq, const int64_t *offsets, int64_t n, const rb_prep_params *p, const int64_t *seg_offsets,
                    rb_prep_rec *recs, int32_t *out_segs, char *out_seq, double *kernel_ms) {
    return rb::guarded([&] { rb::prepare_call(device, seq, offsets, n, p, seg_offsets, recs, out_segs, out_seq, kernel_ms); });
}
}  // extern "C"
