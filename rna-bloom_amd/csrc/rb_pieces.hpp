// rb_pieces.hpp — query calls that work piece by piece so that their device scratch stays bounded whatever the caller asks for: how many
// k-mers a piece may hold (RB_QUERY_PIECE), where the pieces are cut, and the loop over the pieces in two layers: for_each_piece — the cut, the
// profile bracket around a piece's kernels, the wait at its end, the profile entry — and on top of it, for the calls whose records are host
// text, for_each_host_piece with the piece's text as a lazily uploaded packed batch and PieceRows, the piece's getKmers rows (DESIGN.md §5
// "Piece by piece").  Host code only.
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

// The piece for_each_piece hands to its body: records [ra, rb) of the call, pn of them.  The body sizes its scratch, uploads what it reads,
// launches its kernels between kernels_begin() and kernels_end() and enqueues its copies back, all on the query stream of a leased context.
class Piece {
public:
    int64_t ra = 0, rb = 0, pn = 0;
    // around the piece's kernels — after its table and text uploads are enqueued, before its copies back: the interval the profile entry sums
    void kernels_begin() { busy = true; if (timing) RB_HIP(hipEventRecord(ev[0], s)); }
    void kernels_end() { if (timing) { RB_HIP(hipEventRecord(ev[1], s)); timed = true; } }
    // wait for what the piece enqueued: its results are on the host, its tables and scratch may go.  The loop does it after the body; a body
    // that has to look at a result before the next piece calls it itself.  A body that found nothing to do — it never came to
    // kernels_begin() — has nothing to wait for.
    void finish() {
        if (!busy || done) return;
        done = true;
        RB_HIP(hipStreamSynchronize(s));
        if (timed) { float t = 0; RB_HIP(hipEventElapsedTime(&t, ev[0], ev[1])); ms += t; ++launches; }
    }
protected:
    template <typename P, typename PC, typename Body>
    friend void for_each_piece(rb_graph *, hipStream_t, P &&, int64_t, int64_t, const char *, PC &, Body &&);
    rb_graph *g = nullptr;
    hipStream_t s = nullptr;
    Event ev[2];
    bool timing = false, timed = false, busy = false, done = false;
    double ms = 0;                                      // the call's bracketed intervals so far, one launch a piece
    int64_t launches = 0;
};

// The lower layer of the piece loop: body(pc) for every piece of n records, in order, on the query stream s of a leased context.  A piece takes
// as many records as cost at most piece_dflt together (RB_QUERY_PIECE overrides it) by the prefix sums prefix(i) = cost of records [0, i), and
// one record at the least.  prof_name: with profiling on (rb_graph_profile_enable) the bracketed intervals of the call are summed into this
// profile entry, one launch a piece; nullptr: not timed.  pc is the caller's piece — a Piece, or what a layer above adds to it; what a piece
// means (text, batches, tables) is that layer's or the body's business.
template <typename P, typename PC, typename Body>
void for_each_piece(rb_graph *g, hipStream_t s, P &&prefix, int64_t n, int64_t piece_dflt, const char *prof_name, PC &pc, Body &&body) {
    Piece &base = pc;
    base.g = g; base.s = s;
    base.timing = prof_name && g->prof_on;
    if (base.timing) for (Event &e : base.ev) RB_HIP(hipEventCreate(&e.e));
    const std::vector<int64_t> cut = piece_cuts(prefix, n, query_piece_max(piece_dflt));
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        base.ra = cut[c]; base.rb = cut[c + 1]; base.pn = base.rb - base.ra;
        base.timed = base.busy = base.done = false;
        body(pc);
        base.finish();
    }
    if (base.launches) {
        std::lock_guard<std::mutex> lk(g->qm);              // (queries share the handle: the profile table is written under the context lock)
        g->prof_add(prof_name, base.ms, base.launches);
    }
}
template <typename P, typename Body>
void for_each_piece(rb_graph *g, hipStream_t s, P &&prefix, int64_t n, int64_t piece_dflt, const char *prof_name, Body &&body) {
    Piece pc;
    for_each_piece(g, s, std::forward<P>(prefix), n, piece_dflt, prof_name, pc, std::forward<Body>(body));
}

// The piece for_each_host_piece hands to its body: records [ra, rb) of the call with `unit` sequences each — sequences [unit ra, unit rb) — that
// have pt > 0 k-mers together.
class HostPiece : public Piece {
public:
    int64_t pt = 0;
    int unit = 1;
    // the piece's text as a packed batch, uploaded at the first call and kept until the piece is over.  A body that finds nothing to do for
    // a piece returns without asking: nothing is uploaded, and finish() has nothing to wait for.
    const rb_batch *batch() {
        if (!b) { busy = true; b = upload_text_batch(g->p.device, seq, offsets, unit * ra, unit * pn, s); }
        return b.get();
    }
private:
    template <typename Body>
    friend void for_each_host_piece(rb_graph *, hipStream_t, const char *, const int64_t *, const int64_t *, int64_t, const char *, int64_t, Body &&, int, const int64_t *);
    friend struct PieceRows;
    const char *seq = nullptr;
    const int64_t *offsets = nullptr, *ko = nullptr;
    BatchPtr b;
    std::vector<int64_t> tab;                           // the piece's table on the host (PieceRows)
};

// The upper layer: body(piece) for every piece of <= piece_dflt k-mers of n records of host text that has a k-mer at all.  A record is `unit`
// sequences (1; a read pair: 2) of seq / offsets; ko: kmer_offsets of the unit * n sequences.  The piece keeps its lazily uploaded batch.
// cost (n + 1 prefix sums, or nullptr): what the pieces are cut by where a record's scratch does not follow its k-mers (a sequence that grows).
template <typename Body>
void for_each_host_piece(rb_graph *g, hipStream_t s, const char *seq, const int64_t *offsets, const int64_t *ko, int64_t n, const char *prof_name,
                         int64_t piece_dflt, Body &&body, int unit, const int64_t *cost) {
    HostPiece pc;
    pc.seq = seq; pc.offsets = offsets; pc.ko = ko; pc.unit = unit;
    for_each_piece(g, s, [&](int64_t i) { return cost ? cost[i] : ko[unit * i]; }, n, piece_dflt, prof_name, pc, [&](HostPiece &hp) {
        hp.pt = ko[unit * hp.rb] - ko[unit * hp.ra];
        if (hp.pt == 0) return;
        body(hp);
        hp.finish();
        hp.b.reset();
    });
}
template <typename Body>
void for_each_host_piece(rb_graph *g, hipStream_t s, const char *seq, const int64_t *offsets, const int64_t *ko, int64_t n, const char *prof_name,
                         int64_t piece_dflt, Body &&body) {
    for_each_host_piece(g, s, seq, offsets, ko, n, prof_name, piece_dflt, std::forward<Body>(body), 1, nullptr);
}
// ... with the usual pieces of 16 M k-mers
template <typename Body>
void for_each_host_piece(rb_graph *g, hipStream_t s, const char *seq, const int64_t *offsets, const int64_t *ko, int64_t n, const char *prof_name,
                         Body &&body, int unit = 1) {
    for_each_host_piece(g, s, seq, offsets, ko, n, prof_name, (int64_t)16 << 20, std::forward<Body>(body), unit, nullptr);
}

// A piece's getKmers rows as its kernel reads them: the k-mer offsets of its unit * pn sequences (kof[0] = 0), both strands' hashes and the
// count of its pt k-mers, and its batch's 2-bit codes, usable-letter bits and word offsets.
struct PieceRows {
    const int64_t *kof;
    const uint64_t *F, *R;
    const float *cnt;
    const uint64_t *codes;
    const uint32_t *valid, *woff;
    int64_t pn, pt;
    // The rows of piece pc in the context's buffers: b0 the table — the k-mer offsets [unit pn + 1], then the caller's n_extra columns, which
    // the kernel finds at kof + unit pn + 1 —, b1 / b2 the hashes, the head of b3 the counts (the caller has reserved b3: pt floats, then what
    // it lays out behind them, and has enqueued its own uploads).  The table goes up, the piece's kernels begin (kernels_begin()) and
    // getKmers is their first.
    PieceRows(rb_graph *g, rb_query_ctx &c, HostPiece &pc, const int64_t *extra = nullptr, size_t n_extra = 0) {
        const int64_t ns = pc.unit * pc.pn, s0 = pc.unit * pc.ra;
        pc.tab.resize((size_t)ns + 1 + n_extra);
        for (int64_t i = 0; i <= ns; ++i) pc.tab[(size_t)i] = pc.ko[s0 + i] - pc.ko[s0];
        std::copy(extra, extra + n_extra, pc.tab.begin() + (ns + 1));
        const rb_batch *b = pc.batch();
        c.b0.reserve(pc.tab.size() * 8);
        c.b1.reserve((size_t)pc.pt * 8);
        c.b2.reserve((size_t)pc.pt * 8);
        kof = c.b0.as<int64_t>();
        F = c.b1.as<uint64_t>(); R = c.b2.as<uint64_t>();
        cnt = c.b3.as<float>();
        codes = b->codes; valid = b->valid; woff = b->woff;
        pn = pc.pn; pt = pc.pt;
        RB_HIP(hipMemcpyAsync(c.b0.p, pc.tab.data(), pc.tab.size() * 8, hipMemcpyHostToDevice, pc.s));
        pc.kernels_begin();
        launch_get_kmers(g, b, kof, c.b1.as<uint64_t>(), c.b2.as<uint64_t>(), c.b3.as<float>(), pc.s);
    }
    // into a kernel's argument struct that names the rows as this does (k_trim_artifacts fills R itself in a stranded graph: its field is not const)
    template <class ARGS> void into(ARGS &a) const {
        a.pn = pn; a.kof = kof; a.F = F; a.R = const_cast<uint64_t *>(R); a.cnt = cnt; a.codes = codes; a.valid = valid; a.woff = woff;
    }
};

// the longest k-mer list among the n sequences of ko
inline int64_t longest_list(const std::vector<int64_t> &ko, int64_t n) {
    int64_t longest = 0;
    for (int64_t i = 0; i < n; ++i) longest = std::max(longest, ko[(size_t)i + 1] - ko[(size_t)i]);
    return longest;
}

}  // namespace rb
