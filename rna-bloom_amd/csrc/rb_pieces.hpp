// rb_pieces.hpp — query calls that work piece by piece so that their device scratch stays bounded whatever the caller asks for: how many
// k-mers a piece may hold (RB_QUERY_PIECE), where the pieces are cut, and — for the calls whose sequences are host text (rb_graph_kmers,
// rb_graph_paired_kmer_segments, rb_graph_correct_mismatches) — the loop over the pieces: upload of a piece's text as a packed batch, the
// profile bracket around its kernels, the wait at its end (DESIGN.md §5 "Piece by piece").  Host code only.
#pragma once
#include "rb_pipeline.hpp"

namespace rb {

// RB_QUERY_PIECE=<n>: the most k-mers (counts, windows + reads) a piece of a query call holds, at least 1; dflt where it is not set
inline int64_t query_piece_max(int64_t dflt) {
    const char *e = getenv("RB_QUERY_PIECE");
    return e ? std::max<int64_t>(1, atoll(e)) : dflt;
}

// k-mer prefix sums of n host sequences: ko[i + 1] - ko[i] = windows of k bases in sequence i, ko[0] = 0.  who (the entry point's name, or
// nullptr: unchecked) is what the two argument errors are reported under.
inline void kmer_offsets(const int64_t *offsets, int64_t n, int64_t k, int64_t *ko, const char *who) {
    ko[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t l = offsets[i + 1] - offsets[i], nk = l >= k ? l - k + 1 : 0;
        if (who) {
            RB_REQUIRE(l >= 0, "%s: offsets[%lld] > offsets[%lld]", who, (long long)i, (long long)i + 1);
            RB_REQUIRE(nk <= INT32_MAX, "%s: sequence %lld has more k-mers than an int holds", who, (long long)i);
        }
        ko[i + 1] = ko[i] + nk;
    }
}

// Read boundaries 0 = cut[0] < cut[1] < ... = n of the pieces of reads [0, n): a piece takes as many reads as cost at most piece_max
// together, and one read at the least.  Two forms of the one rule, with the same cuts for the same non-negative costs: by bisection
// where the caller holds the costs' prefix sums (prefix(i) = cost of reads [0, i)) ...
template <typename P> std::vector<int64_t> piece_cuts(P &&prefix, int64_t n, int64_t piece_max) {
    std::vector<int64_t> cut{0};
    while (cut.back() < n) {
        const int64_t a = cut.back();
        int64_t lo = a + 1, hi = n;
        while (lo < hi) { const int64_t mid = (lo + hi + 1) >> 1; if (prefix(mid) - prefix(a) <= piece_max) lo = mid; else hi = mid - 1; }
        cut.push_back(lo);
    }
    return cut;
}
// ... and in one pass over cost(i) where it does not (no prefix array is built for it: 8 bytes a read, first touched inside the call)
template <typename C> std::vector<int64_t> piece_cuts_by_cost(C &&cost, int64_t n, int64_t piece_max) {
    std::vector<int64_t> cut{0};
    for (int64_t i = 0, acc = 0; i < n; ++i) {
        const int64_t c = cost(i);
        if (i > cut.back() && acc + c > piece_max) { cut.push_back(i); acc = 0; }
        acc += c;
    }
    if (n > 0) cut.push_back(n);
    return cut;
}

// reads [first, first + n) of host text as a packed batch with the rnz plane (all-window hashing of raw strings), uploaded and encoded on st
inline BatchPtr upload_text_batch(int device, const char *seq, const int64_t *offsets, int64_t first, int64_t n, hipStream_t st) {
    AsciiUpload up;
    try {
        ascii_batch_begin(up, device, seq, nullptr, offsets, first, n, 0, st, true);
        return BatchPtr(ascii_batch_finish(up));
    } catch (...) { ascii_batch_abort(up); throw; }
}

// The piece for_each_host_piece hands to its body: sequences [ra, rb) of the call, pn of them with pt > 0 k-mers together.
class HostPiece {
public:
    int64_t ra = 0, rb = 0, pn = 0, pt = 0;
    // the piece's text as a packed batch, uploaded at the first call and kept until the piece is over.  A body asks for it BEFORE it
    // enqueues anything on the stream: a body that finds nothing to do for a piece returns without asking, nothing is uploaded, and
    // finish() has nothing to wait for.
    const rb_batch *batch() {
        if (!b) b = upload_text_batch(g->p.device, seq, offsets, ra, pn, s);
        return b.get();
    }
    // around the piece's kernels — after its table and text uploads are enqueued, before its copies back: the interval the profile entry sums
    void kernels_begin() { if (timing) RB_HIP(hipEventRecord(ev[0], s)); }
    void kernels_end() { if (timing) { RB_HIP(hipEventRecord(ev[1], s)); timed = true; } }
    // wait for what a piece that asked for its batch enqueued: its results are on the host, its table and batch may go.  The loop does
    // it after the body; a body that has to look at a result before the next piece calls it itself.
    void finish() {
        if (!b || done) return;
        done = true;
        RB_HIP(hipStreamSynchronize(s));
        if (timed) { float t = 0; RB_HIP(hipEventElapsedTime(&t, ev[0], ev[1])); ms += t; ++launches; }
    }
private:
    template <typename Body>
    friend void for_each_host_piece(rb_graph *, hipStream_t, const char *, const int64_t *, const int64_t *, int64_t, const char *, int64_t, Body &&);
    rb_graph *g = nullptr;
    hipStream_t s = nullptr;
    const char *seq = nullptr;
    const int64_t *offsets = nullptr;
    BatchPtr b;
    Event ev[2];
    bool timing = false, timed = false, done = false;
    double ms = 0;                                      // the call's bracketed intervals so far, one launch a piece
    int64_t launches = 0;
};

// body(piece) for every piece of <= piece_dflt k-mers (RB_QUERY_PIECE overrides it) of n host sequences that has a k-mer at all, in order, on the query
// stream s of a leased context.  ko: kmer_offsets of the sequences.  The body sizes its scratch, uploads its table, launches its kernels
// between kernels_begin() and kernels_end() and enqueues its copies back, all on s.  prof_name: with profiling on
// (rb_graph_profile_enable) the bracketed intervals of the call are summed into this profile entry, one launch a piece; nullptr: not timed.
template <typename Body>
void for_each_host_piece(rb_graph *g, hipStream_t s, const char *seq, const int64_t *offsets, const int64_t *ko, int64_t n, const char *prof_name,
                         int64_t piece_dflt, Body &&body) {
    HostPiece pc;
    pc.g = g; pc.s = s; pc.seq = seq; pc.offsets = offsets;
    pc.timing = prof_name && g->prof_on;
    if (pc.timing) for (Event &e : pc.ev) RB_HIP(hipEventCreate(&e.e));
    const std::vector<int64_t> cut = piece_cuts([&](int64_t i) { return ko[i]; }, n, query_piece_max(piece_dflt));
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        pc.ra = cut[c]; pc.rb = cut[c + 1]; pc.pn = pc.rb - pc.ra; pc.pt = ko[pc.rb] - ko[pc.ra];
        if (pc.pt == 0) continue;
        pc.timed = pc.done = false;
        body(pc);
        pc.finish();
        pc.b.reset();
    }
    if (pc.launches) {
        std::lock_guard<std::mutex> lk(g->qm);              // (queries share the handle: the profile table is written under the context lock)
        g->prof_add(prof_name, pc.ms, pc.launches);
    }
}
// ... with the usual pieces of 16 M k-mers
template <typename Body>
void for_each_host_piece(rb_graph *g, hipStream_t s, const char *seq, const int64_t *offsets, const int64_t *ko, int64_t n, const char *prof_name,
                         Body &&body) {
    for_each_host_piece(g, s, seq, offsets, ko, n, prof_name, (int64_t)16 << 20, std::forward<Body>(body));
}

}  // namespace rb
