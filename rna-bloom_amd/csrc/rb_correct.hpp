// rb_correct.hpp — correctErrorHelper (R/util/GraphUtils.java:3711-3912) on the sequences of a piece, as a body that both rb_graph_correct_errors
// (rb_correct.hip: host text, one run) and rb_graph_correct_pairs (rb_pair_correct.hip: text that stays on the device from round to round) run.
// Host code only; the kernels are rb_correct.hip's.
#pragma once
#include <vector>

#include "rb_pieces.hpp"
#include "rb_wave.hpp"

namespace rb {

constexpr int CE_MAX_INDEL = 4096;               // the largest max_indel_size taken (the reference's default is 1)

// a bump allocator over one device buffer
struct Arena {
    uint8_t *base = nullptr;
    size_t at = 0;
    template <typename T> T *take(size_t n) { T *p = reinterpret_cast<T *>(base + at); at = up16(at + n * sizeof(T)); return p; }
};

struct CorrPhaseTimer {                   // device time per phase of the call, summed over pieces and chunks (profiling on)
    static constexpr int N = 6;
    const char *names[N] = {"correct_errors.profile", "correct_errors.scan", "correct_errors.walks", "correct_errors.resolve", "correct_errors.stitch",
                            "correct_errors.mismatch"};
    bool on = false;
    hipStream_t s = nullptr;
    struct Span { int phase; Event e0, e1; };
    std::vector<Span> spans;
    double ms[N] = {0, 0, 0, 0, 0, 0};
    int64_t launches[N] = {0, 0, 0, 0, 0, 0};
    void begin(int phase) {
        if (!on) return;
        spans.emplace_back();
        spans.back().phase = phase;
        RB_HIP(hipEventCreate(&spans.back().e0.e));
        RB_HIP(hipEventCreate(&spans.back().e1.e));
        RB_HIP(hipEventRecord(spans.back().e0, s));
    }
    void end() { if (on) RB_HIP(hipEventRecord(spans.back().e1, s)); }
    void collect() {                      // the stream is idle
        for (Span &sp : spans) { float t = 0; RB_HIP(hipEventElapsedTime(&t, sp.e0, sp.e1)); ms[sp.phase] += t; ++launches[sp.phase]; }
        spans.clear();
    }
};

// the most letters a sequence of `len` letters can have after gap repair: see rb_capi.h
inline int64_t corr_capacity(int64_t len, int64_t k, int64_t max_indel) {
    const int64_t nk = len >= k ? len - k + 1 : 0;
    if (nk <= 0) return len;
    return len + ((nk - 1) / 2) * max_indel + ((nk - 1) / (k + 1)) * 2;
}

// One run of the helper over the pn sequences of a piece.  prepare() lays the piece's arrays out in the leased context's four buffers and uploads
// its tables; the caller then puts the input where the `in` pointers point — or, with own_input false, points them at rows it holds itself —;
// run() launches gap scan, walks, resolve, stitch, getKmers of the stitched text and the mismatch pass on the stream and returns with the last
// of them enqueued.  The input is a dense layout (tof / kof), the output a capacity layout (ctof / ckof with the lengths in clen / cnk).
struct CorrBody {
    // set by the caller before prepare()
    rb_graph *g = nullptr;
    rb_query_ctx *c = nullptr;
    hipStream_t s = nullptr;
    CorrPhaseTimer *ph = nullptr;
    DevBuf *gbuf = nullptr, *wbuf = nullptr;  // the gap-level arrays; the walks that run together: the call's, not the context's
    rb_corr_params p{};
    bool own_input = true;                    // the arena holds the input text, its counts and the thresholds; b1 / b2 hold its hash rows (overwritten by run())
    int write_counts = 0;                     // the mismatch pass leaves the counts of the final text in cnt2
    const char *who = "rb_graph_correct_errors";
    // the piece
    int64_t pn = 0, pt = 0, tb = 0, ctb = 0, cpt = 0, nlong = 0, G = 0;
    std::vector<int64_t> tab;                 // host: kof, tof, ctof, ckof [pn + 1 each], the long sequences
    std::vector<uint32_t> cwoff;
    std::vector<int64_t> gof, rof, lof;
    std::vector<int32_t> ngap, lists;
    std::vector<rb_corr_gap> recs;            // as the scan left them (outcomes: drecs)
    const int64_t *dkof = nullptr, *dtof = nullptr, *dctof = nullptr, *dckof = nullptr, *dids = nullptr;
    const uint32_t *dcwoff = nullptr;
    // own_input: the arena's input rows, for the caller to fill between prepare() and run() — text [tb], counts [pt], thresholds [pn]; the
    // hash rows are dF / dR.  prepare() points the `in` pointers at them
    uint8_t *own_txt = nullptr;
    float *own_cnt = nullptr, *own_thr = nullptr;
    // in: text, getKmers rows, thresholds [pn]
    const uint8_t *dtxt = nullptr;
    const uint64_t *dFin = nullptr, *dRin = nullptr;
    const float *dcnt = nullptr, *dthr = nullptr;
    // out (capacity layout): the stitched and mismatch-corrected text, its rows and counts, length and k-mers, RB_CORR_GAP, the mismatch pass's replacements
    uint8_t *dctxt = nullptr, *drow = nullptr;
    uint64_t *dF = nullptr, *dR = nullptr;
    float *dcnt2 = nullptr;
    int32_t *dclen = nullptr, *dcnk = nullptr, *dnf = nullptr, *dng = nullptr;
    uint32_t *dflags = nullptr, *dvalid = nullptr, *dover = nullptr;
    int64_t *dgof = nullptr, *drof = nullptr;
    rb_corr_gap *drecs = nullptr;
    // absolute offset arrays of pn + 1 entries each; only differences to entry 0 are used
    void prepare(int64_t pn_, const int64_t *kof, const int64_t *tof, const int64_t *ctof);
    void run();
    const int64_t *h_ctof() const { return tab.data() + 2 * (pn + 1); }
    const int64_t *h_ckof() const { return tab.data() + 3 * (pn + 1); }
};

// getKmers of device text: hashes, counts and usable-letter bits of pn sequences, sequence r = txt[tof[r] .. tof[r] + len[r]) with its rows at kof[r]
// and its bit words at woff[r] (rb_correct.hip: k_text_kmers)
void launch_text_kmers(rb_graph *g, int64_t pn, const int64_t *tof, const int64_t *kof, const uint32_t *woff, const uint8_t *txt, const int32_t *len,
                       uint32_t *valid, uint64_t *F, uint64_t *R, float *cnt, hipStream_t s);

}  // namespace rb
