// rb_extend_loop.hip — the extension loop of fragments on the device (rb_graph_extend_loop): GraphUtils.extendSE (R/util/GraphUtils.java:6454-6565)
// and extendPE (:6567-6678) over hasDuplicatedKmerPair (:6416-6452), the sixth step of TranscriptAssemblyWorker.run (R/RNABloom.java:1817-1931).
// ONE kernel, a wavefront per sequence from its first round to its last: the sequence — per k-mer both strands' hashes and the count, per
// letter a 2-bit code in a byte — lies in a row of device scratch with `room` free entries on both sides, so that both directions append in
// place.  A round is the branch step itself — ex_one_on of rb_extend_step.hpp, the body of rb_graph_extend_se / _pe — with the side's last
// min(size, max(d_r, D)) k-mers and their letters where they lie in the row (ExRowText); the floor is a wave_min over the row's counts, the
// usedKmers test and hasDuplicatedKmerPair are sweeps of the row's forward hashes that are confirmed on the bases (rb_wave.hpp).  Nothing is
// written to the graph (DESIGN.md §5 "Extension loop").
//
// The reference, line by line (the two methods differ in D — the read-paired distance for SE, the fragment-paired one for PE — and in the step):
//   :6461-6465  origLen; usedKmers = the list's k-mers; the list is reversed — here the left side works at the row's low end, list index i is
//               position hi - 1 - i, and usedKmers is the row's k-mers [lo, hi) at all times.
//   :6467       while (true), an outer iteration:
//   :6468         covThreshold = getMinimumKmerCoverage of the last min(size, D) k-mers (an added k-mer carries the count its step returned)
//   :6472-6480    do covThreshold = max(minKmerCov, covThreshold * 0.1f); e = step(list, covThreshold) until e is not empty or covThreshold ==
//                 minKmerCov — `steps` counts the steps, `floor_drops` the empty ones above the lowest floor
//   :6482         e empty: the side ends (END_NOTHING)
//   :6486-6495    used = every k-mer of e is in usedKmers
//   :6497-6504    a second loop re-tests list members against usedKmers, which holds every list member: it can never clear the flag and is left out
//   :6506         used && size < D: the side ends (END_USED_SHORT); used && hasDuplicatedKmerPair(list, e.getLast(), D, size - 1 - D + |e|): the
//                 side ends (END_USED_PAIR).  :6416-6452 with cursor = e.getLast(), mate = list[size - 1 - D + |e|] (never negative here: size >=
//                 D): lastIndexOf(cursor) = c2 with c2 - D >= 0 and list[c2 - D] == mate; else indexOf(cursor) = c1 != c2 with c1 - D >= 0 and
//                 list[c1 - D] == mate; else any i in (c1, c2) with list[i] == cursor, i - D >= 0 and list[i - D] == mate.  When c2 - D < 0 no
//                 occurrence has a mate D entries back, so the three tests together are: some i >= D with list[i] == cursor and list[i - D] ==
//                 mate — ONE sweep with a lane per i.
//   :6510-6511    the k-mers are appended to the list and to usedKmers (`used_passed` counts the rounds that were used and went on)
//   :6514-6516    leftExtLen; the list is reversed back; :6518-6562 the same to the right with extendRightSE / extendRightPE.
// What the call adds is `room`: a round whose k-mers do not fit in what is left of the side's room is dropped whole, before the used test, the side
// ends with END_ROOM, and after a left END_ROOM the right side is not run.  The state after any whole round is a state of the reference's loop
// (usedKmers is the list, the floor is recomputed from the list at the top of every outer iteration), so a caller resumes from the returned text.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

#include "rb_pieces.hpp"
#include "rb_extend_step.hpp"

using namespace rb;

// Java float arithmetic: a floor is one float32 product
#pragma clang fp contract(off)

namespace {

// What the branch step reads and writes for ONE sequence, per wavefront of the launch: its k-mer offsets {0, nt}, its floor, its record, its
// result's bases and counts, and for D > EX_LDS_D the rows of its walks.
struct ElSlot {
    size_t o_kof, o_floor, o_rec, o_ob, o_oc, o_walk, bytes;
    __host__ __device__ ElSlot(int D, bool lds) {
        o_kof = 0; o_floor = 16; o_rec = 32; o_ob = o_rec + up16(sizeof(rb_extend_pe_rec));
        o_oc = up16(o_ob + (size_t)D + 2); o_walk = up16(o_oc + ((size_t)D + 2) * 4);
        bytes = up16(o_walk + (lds ? 0 : ex_row_bytes(D)));
    }
};

struct ElArgs {
    FilterView fv;
    PairView pf, ff;
    int stranded, k, d_r, D, room, t1, t2, t3;
    float min_cov;
    int64_t pn;
    const int64_t *kof;                          // the piece's rows (PieceRows): k-mer offsets, getKmers hashes and counts, the batch
    const uint64_t *F, *R;
    const float *cnt;
    const uint64_t *codes;
    const uint32_t *valid, *woff;
    const int64_t *cof, *oof;                    // [pn + 1] each: the sequences' places in the rows' per-k-mer arrays and in the letters' / out
    const uint8_t *phase;
    uint64_t *rF, *rR;                           // the rows: per capacity k-mer both strands' hashes and the count, per capacity letter a code
    float *rC;
    uint8_t *rT, *out;
    rb_extend_loop_rec *recs;
    uint8_t *slots;
    uint32_t *over;                              // rows found outgrown (never: a round that does not fit is dropped)
};

// a sequence as it lies in its row: k-mers [lo, hi) by their start in the text, room for [0, cap)
struct ElRow {
    uint64_t *F, *R;
    float *C;
    uint8_t *T;
    int lo, hi, cap;
};

__device__ __forceinline__ bool el_equal(const uint8_t *x, const uint8_t *y, int k) {
    bool eq = true;
    for (int q = 0; q < k && eq; ++q) eq = x[q] == y[q];
    return eq;
}

// One side of the loop (left: extendLeft*, the list reversed) until it ends; returns how (RB_EXTL_END_*).
template <bool PE>
__device__ __forceinline__ int el_side(const ElArgs &a, ExArgsT<PE> &ea, uint8_t *xrow, uint8_t *srow, const ElSlot &lay, ElRow &w, bool left,
                                       rb_extend_loop_rec &v, int &rounds, float &last_floor, uint32_t lane) {
    const int k = a.k, D = a.D;
    const WaveDir<> dr = wave_dir(a.stranded, k, left ? 1 : 0);
    const uint8_t *eb = srow + lay.o_ob;
    const float *ec = reinterpret_cast<const float *>(srow + lay.o_oc);
    for (;;) {
        const int size = w.hi - w.lo, m = min(size, D);
        const int f0 = left ? w.lo : w.hi - m;
        float thr = wave_min(f0, f0 + m, [&](int j) { return w.C[j]; }, lane);                                  // :6468
        const int nt = min(size, max(a.d_r, D)), tp = left ? w.lo : w.hi - nt;                                // the tail's first position in the text
        ea.direction = left ? 1 : 0;
        ea.F = w.F + tp; ea.R = w.R + tp; ea.cnt = w.C + tp;
        if (lane == 0) reinterpret_cast<int64_t *>(srow + lay.o_kof)[1] = nt;
        int ne = 0;
        for (;;) {                                                                                              // :6472-6480
            thr = fmaxf(a.min_cov, thr * 0.1f);
            if (lane == 0) *reinterpret_cast<float *>(srow + lay.o_floor) = thr;
            wave_fence();
            ex_one_on<PE>(ea, 0, xrow, lane, ExRowText{w.T + tp});
            wave_fence();
            ++v.steps;
            last_floor = thr;
            const int32_t *er = reinterpret_cast<const int32_t *>(srow + lay.o_rec);                          // outcome, why, n_candidates, out_len: both records begin alike
            ne = er[0] == RB_EXT_NONE ? 0 : er[3];
            if (ne > 0 || thr == a.min_cov) break;
            ++v.floor_drops;
        }
        if (ne == 0) return RB_EXTL_END_NOTHING;                                                                // :6482
        if (ne > (left ? w.lo : w.cap - w.hi)) return RB_EXTL_END_ROOM;                                       // only whole rounds
        // the round's k-mers behind the side's end, not yet part of the list: letters first (a lane each), then the hashes, rolled from the last k-mer
        for (int i = (int)lane; i < ne; i += 64) w.T[left ? w.lo - 1 - i : w.hi + k - 1 + i] = (uint8_t)letter_code(eb[i]);
        wave_fence();
        {
            const int lp = left ? w.lo : w.hi - 1;
            uint64_t A = left ? w.R[lp] : w.F[lp], B = left ? w.F[lp] : w.R[lp];
            for (int i = 0; i < ne; ++i) {
                const int np = left ? w.lo - 1 - i : w.hi + i;                                                  // the new k-mer's start; the one before it starts at np -+ 1
                uint64_t nA, nB;
                dr.step(A, B, w.T[left ? np + k : np - 1], w.T[left ? np : np + k - 1], nA, nB);
                A = nA; B = nB;
                if (lane == 0) { w.F[np] = dr.fwd(A, B); w.R[np] = left ? A : B; w.C[np] = ec[i]; }
            }
        }
        wave_fence();
        bool used = true;                                                                                       // :6486-6495
        for (int i = 0; i < ne && used; ++i) {
            const int np = left ? w.lo - 1 - i : w.hi + i;
            used = wave_find(w.lo, w.hi, k, [&](int j) { return w.F[j]; }, w.F[np], [&](int j, int q) { return w.T[j + q]; },
                             [&](int q) { return w.T[np + q]; }, false, lane) != WAVE_NOWHERE;
        }
        if (used) {                                                                                             // :6506
            if (size < D) return RB_EXTL_END_USED_SHORT;
            const int mi = size - 1 - D + ne;                                                                   // the mate's list index
            const int cp = left ? w.lo - ne : w.hi + ne - 1, mp = left ? w.hi - 1 - mi : w.lo + mi;
            const uint64_t cf = w.F[cp], mf = w.F[mp];
            // list index i >= D with list[i] == cursor and list[i - D] == mate, by i's position p: the mate's candidate lies D positions before it (left: behind it)
            const int p0 = left ? w.lo : w.lo + D, p1 = left ? w.hi - D : w.hi, md = left ? D : -D;
            const int hit = wave_first(p0, p1, [&](int p) {
                return w.F[p] == cf && w.F[p + md] == mf && el_equal(w.T + p, w.T + cp, k) && el_equal(w.T + p + md, w.T + mp, k);
            }, lane);
            if (hit < p1) return RB_EXTL_END_USED_PAIR;
            ++v.used_passed;
        }
        if (left) w.lo -= ne; else w.hi += ne;                                                                  // :6510-6511
        ++rounds;
    }
}

// the loop of sequence r of the piece by one wavefront with its slot
template <bool PE>
__device__ __forceinline__ void el_one(const ElArgs &a, ExArgsT<PE> &ea, uint8_t *xrow, uint8_t *srow, const ElSlot &lay, int64_t r, uint32_t lane) {
    const int k = a.k, room = a.room;
    const int64_t k0 = a.kof[r];
    const int nk0 = (int)(a.kof[r + 1] - k0);
    if (nk0 == 0) return;                                     // not judged: the host has written its record and its text
    ElRow w;
    w.F = a.rF + a.cof[r]; w.R = a.rR + a.cof[r]; w.C = a.rC + a.cof[r]; w.T = a.rT + a.oof[r];
    w.lo = room; w.hi = room + nk0; w.cap = nk0 + 2 * room;
    {
        const uint64_t *cw = a.codes + a.woff[r];
        for (int p = (int)lane; p < nk0 + k - 1; p += 64) w.T[room + p] = (uint8_t)((cw[p >> 5] >> (2 * (p & 31))) & 3u);
        for (int j = (int)lane; j < nk0; j += 64) { w.F[room + j] = a.F[k0 + j]; w.R[room + j] = a.R[k0 + j]; w.C[room + j] = a.cnt[k0 + j]; }
    }
    wave_fence();
    rb_extend_loop_rec v;
    v.status = RB_EXTL_DONE; v.why = RB_EXTL_WHY_NONE;
    v.left_end = v.right_end = RB_EXTL_END_NOT_RUN;
    v.left_rounds = v.right_rounds = v.steps = v.floor_drops = v.used_passed = 0;
    v.left_floor = v.right_floor = 0.0f;
    v.pad[0] = v.pad[1] = 0;
    if (a.phase[r] == 0) v.left_end = el_side<PE>(a, ea, xrow, srow, lay, w, true, v, v.left_rounds, v.left_floor, lane);
    if (v.left_end != RB_EXTL_END_ROOM) v.right_end = el_side<PE>(a, ea, xrow, srow, lay, w, false, v, v.right_rounds, v.right_floor, lane);
    if (v.left_end == RB_EXTL_END_ROOM || v.right_end == RB_EXTL_END_ROOM) v.status = RB_EXTL_ROOM;
    v.left_ext = room - w.lo; v.right_ext = w.hi - (room + nk0); v.out_len = w.hi - w.lo + k - 1;
    if (w.lo < 0 || w.hi > w.cap) {                           // (never: see el_side)
        if (lane == 0) atomicAdd(a.over, 1u);
        v.out_len = 0;
    }
    uint8_t *o = a.out + a.oof[r];
    for (int p = (int)lane; p < v.out_len; p += 64) o[p] = code_letter(w.T[w.lo + p]);
    if (lane == 0) a.recs[r] = v;
}

// A wavefront per sequence, taking sequences in turn.  PE: extendPE.  LDS_ROW: the rows of the step's walks are in LDS (D <= EX_LDS_D); else
// in the wavefront's slot.
template <bool PE, bool LDS_ROW>
__global__ void __launch_bounds__(EX_TPB) k_extloop(ElArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_row[EX_WAVES][LDS_ROW ? ex_row_bytes(EX_LDS_D) : 16];
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;     // (one value a wavefront: the slot's addresses stay scalar)
    const int64_t slot = (int64_t)blockIdx.x * EX_WAVES + wv, n_slots = (int64_t)gridDim.x * EX_WAVES;
    const ElSlot lay(a.D, LDS_ROW);
    uint8_t *srow = a.slots + (size_t)slot * lay.bytes;
    uint8_t *xrow;
    if constexpr (LDS_ROW) xrow = s_row[wv]; else xrow = srow + lay.o_walk;
    // the step's view of ONE sequence, r = 0: its tail's rows are set at every round, the rest here; its letters come from the row (ExRowText)
    ExArgsT<PE> ea;
    ea.fv = a.fv; ea.pf = a.pf;
    ea.stranded = a.stranded; ea.k = a.k; ea.d = a.D; ea.direction = 0; ea.D = LDS_ROW ? EX_LDS_D : a.D;
    ea.pn = 1;
    ea.kof = reinterpret_cast<const int64_t *>(srow + lay.o_kof);
    ea.F = ea.R = nullptr; ea.cnt = nullptr;
    ea.codes = nullptr; ea.valid = nullptr; ea.woff = nullptr;
    ea.floors = reinterpret_cast<const float *>(srow + lay.o_floor);
    ea.out_b = srow + lay.o_ob; ea.out_c = reinterpret_cast<float *>(srow + lay.o_oc);
    if constexpr (PE) {
        ea.recs = nullptr; ea.recs_pe = reinterpret_cast<rb_extend_pe_rec *>(srow + lay.o_rec);
        ea.ff = a.ff; ea.d_r = a.d_r; ea.t1 = a.t1; ea.t2 = a.t2; ea.t3 = a.t3;
    } else ea.recs = reinterpret_cast<rb_extend_rec *>(srow + lay.o_rec);
    if (lane == 0) reinterpret_cast<int64_t *>(srow + lay.o_kof)[0] = 0;
    for (int64_t r = slot; r < a.pn; r += n_slots) {
        el_one<PE>(a, ea, xrow, srow, lay, r, lane);
        wave_fence();
    }
}

void extend_loop_call(rb_graph *g, int which, const char *seq, const int64_t *offsets, int64_t n, const uint8_t *phase, float min_cov, int room,
                      int64_t *out_offsets, char *out_seq, rb_extend_loop_rec *recs) {
    const char *who = "rb_graph_extend_loop";
    RB_REQUIRE(g, "%s: null handle", who);
    RB_REQUIRE(!g->shard, "%s: not available on a shard handle", who);
    RB_REQUIRE(g->dbg.bits && g->cbf, "%s: dbgbf or the counting filter has been destroyed", who);
    RB_REQUIRE(g->rpk.bits, "%s: the graph has no read-paired k-mer filter (created without useReadPairedKmers, or destroyed)", who);
    RB_REQUIRE(which == RB_EXTL_SE || which == RB_EXTL_PE, "%s: which must be RB_EXTL_SE or RB_EXTL_PE, not %d", who, which);
    const bool pe = which == RB_EXTL_PE;
    if (pe) RB_REQUIRE(g->fpk.bits, "%s: the graph has no fragment-paired k-mer filter (rb_graph_init_fragment_pairs was not called, or it was destroyed)", who);
    const int d_r = g->read_d, D = pe ? g->frag_d : d_r, k = g->k;
    RB_REQUIRE(d_r >= 2, "%s: the read-paired k-mer distance is %d (the step needs d >= 2)", who, d_r);
    if (pe) RB_REQUIRE(D >= 2, "%s: the fragment-paired k-mer distance is %d (the step needs d >= 2)", who, D);
    RB_REQUIRE(std::isfinite(min_cov) && min_cov >= 0.0f, "%s: min_kmer_cov must be finite and not negative", who);
    RB_REQUIRE(room >= D + 2 && room <= (1 << 24), "%s: room = %d (the loop's distance + 2 = %d .. 2^24)", who, room, D + 2);
    RB_REQUIRE(n >= 0, "%s: n = %lld", who, (long long)n);
    if (n == 0) return;
    RB_REQUIRE(offsets && out_offsets, "%s: null argument", who);
    RB_REQUIRE(recs || !out_seq, "%s: out_seq needs recs", who);
    RB_REQUIRE(offsets[n] == offsets[0] || seq, "%s: null sequence text", who);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        RB_REQUIRE(len >= 0, "%s: offsets[%lld] > offsets[%lld]", who, (long long)i, (long long)i + 1);
        RB_REQUIRE(len <= INT32_MAX / 2, "%s: sequence %lld has more letters than a row holds", who, (long long)i);
        if (phase) RB_REQUIRE(phase[i] <= 1, "%s: phase[%lld] = %d (0: both sides, 1: the right side only)", who, (long long)i, (int)phase[i]);
    }
    // the capacity layout: len + 2 room letters a sequence
    out_offsets[0] = 0;
    for (int64_t i = 0; i < n; ++i) out_offsets[i + 1] = out_offsets[i] + (offsets[i + 1] - offsets[i]) + 2 * (int64_t)room;
    if (!out_seq) return;
    // What the device judges: at least k letters, all of them upper-case A C G T (the reference compares k-mers as bytes and added letters are
    // upper-case).  The rest comes back as it went in and is an empty sequence to the device.  Pieces are cut by capacity k-mers (cp).
    std::vector<int64_t> to((size_t)n + 1, 0), ko((size_t)n + 1), cp((size_t)n + 1, 0);
    std::vector<uint8_t> why((size_t)n, RB_EXTL_WHY_NONE);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        const char *t = seq + offsets[i];
        if (len < k) why[(size_t)i] = RB_EXTL_WHY_NO_KMER;
        else for (int64_t p = 0; p < len; ++p) if (t[p] != 'A' && t[p] != 'C' && t[p] != 'G' && t[p] != 'T') { why[(size_t)i] = RB_EXTL_WHY_LETTER; break; }
        to[(size_t)i + 1] = to[(size_t)i] + (why[(size_t)i] ? 0 : len);
        cp[(size_t)i + 1] = cp[(size_t)i] + std::max<int64_t>(0, len + 2 * (int64_t)room - k + 1);
    }
    std::vector<char> text((size_t)to[(size_t)n]);
    for (int64_t i = 0; i < n; ++i)
        if (!why[(size_t)i]) memcpy(text.data() + to[(size_t)i], seq + offsets[i], (size_t)(offsets[i + 1] - offsets[i]));
    kmer_offsets(to.data(), n, k, ko.data(), nullptr);
    if (ko[(size_t)n] > 0) {
        RB_HIP(hipSetDevice(g->p.device));
        HostPin pin_out(out_seq, (size_t)out_offsets[n]), pin_rec(recs, (size_t)n * sizeof(rb_extend_loop_rec));
        QueryLease q(g);
        hipStream_t s = q.c->st;
        const bool lds = D <= EX_LDS_D;
        const ElSlot lay(D, lds);
        // piece by piece (rb_pieces.hpp), cut by capacity k-mers: b0 the piece's tables, b1 / b2 the getKmers hashes, b3 counts, records, phases, the rows
        // (20 bytes a capacity k-mer, 2 a capacity letter: the codes and the text out) and the wavefronts' slots; profile entry "extend_loop"
        std::vector<int64_t> extra;
        for_each_host_piece(g, s, text.data(), to.data(), ko.data(), n, "extend_loop", (int64_t)16 << 20, [&](HostPiece &pc) {
            const int64_t ra = pc.ra, rb_ = pc.rb, pn = pc.pn, pt = pc.pt;
            const int64_t ck = cp[(size_t)rb_] - cp[(size_t)ra], ot = out_offsets[rb_] - out_offsets[ra];
            extra.resize(2 * ((size_t)pn + 1));
            for (int64_t i = 0; i <= pn; ++i) {
                extra[(size_t)i] = cp[(size_t)(ra + i)] - cp[(size_t)ra];
                extra[(size_t)(pn + 1 + i)] = out_offsets[ra + i] - out_offsets[ra];
            }
            const int64_t slots = std::min<int64_t>(pn, EX_SCRATCH_SLOTS);
            const unsigned blocks = blocks_for(slots, EX_WAVES);
            const size_t o_rec = up16((size_t)pt * 4), o_ph = o_rec + (size_t)pn * sizeof(rb_extend_loop_rec), o_over = up16(o_ph + (size_t)pn),
                         o_f = o_over + 16, o_r = o_f + (size_t)ck * 8, o_c = o_r + (size_t)ck * 8, o_t = up16(o_c + (size_t)ck * 4),
                         o_out = up16(o_t + (size_t)ot), o_slots = up16(o_out + (size_t)ot);
            q.c->b3.reserve(o_slots + (size_t)blocks * EX_WAVES * lay.bytes + 16);
            uint8_t *base3 = q.c->b3.as<uint8_t>();
            ElArgs a;
            a.fv = g->view(0, 0);
            a.pf = PairView{g->rpk.bits, g->rpk.mod, g->rpk.num_hash, kmul_of(k)};
            a.ff = pe ? PairView{g->fpk.bits, g->fpk.mod, g->fpk.num_hash, kmul_of(k)} : a.pf;
            a.stranded = (int)g->stranded; a.k = k; a.d_r = d_r; a.D = D; a.room = room; a.min_cov = min_cov;
            // isRepeat keeps its counters in signed bytes: a threshold above 127 is never reached (rb_extend.hip)
            const int t1 = (int)java_round((float)k * 0.9f);
            a.t1 = t1 > 127 ? INT32_MAX : t1; a.t2 = (int)java_round((float)(k / 2) * 0.9f); a.t3 = (int)java_round((float)(k / 3) * 0.9f);
            a.recs = reinterpret_cast<rb_extend_loop_rec *>(base3 + o_rec);
            a.phase = base3 + o_ph;
            a.over = reinterpret_cast<uint32_t *>(base3 + o_over);
            a.rF = reinterpret_cast<uint64_t *>(base3 + o_f); a.rR = reinterpret_cast<uint64_t *>(base3 + o_r); a.rC = reinterpret_cast<float *>(base3 + o_c);
            a.rT = base3 + o_t; a.out = base3 + o_out; a.slots = base3 + o_slots;
            RB_HIP(hipMemsetAsync(base3 + o_rec, 0, o_f - o_rec, s));                 // (records no wavefront writes, phase 0, the outgrown count)
            RB_HIP(hipMemsetAsync(base3 + o_out, 0, (size_t)ot, s));                  // (zeros behind every text, whatever the cuts)
            if (phase) RB_HIP(hipMemcpyAsync(base3 + o_ph, phase + ra, (size_t)pn, hipMemcpyHostToDevice, s));
            PieceRows(g, *q.c, pc, extra.data(), extra.size()).into(a);
            a.cof = a.kof + pn + 1; a.oof = a.cof + pn + 1;
            if (pe) {
                if (lds) hipLaunchKernelGGL((k_extloop<true, true>), dim3(blocks), dim3(EX_TPB), 0, s, a);
                else hipLaunchKernelGGL((k_extloop<true, false>), dim3(blocks), dim3(EX_TPB), 0, s, a);
            } else {
                if (lds) hipLaunchKernelGGL((k_extloop<false, true>), dim3(blocks), dim3(EX_TPB), 0, s, a);
                else hipLaunchKernelGGL((k_extloop<false, false>), dim3(blocks), dim3(EX_TPB), 0, s, a);
            }
            RB_HIP(hipGetLastError());
            pc.kernels_end();
            uint32_t over = 0;
            RB_HIP(hipMemcpyAsync(recs + ra, a.recs, (size_t)pn * sizeof(rb_extend_loop_rec), hipMemcpyDeviceToHost, s));
            RB_HIP(hipMemcpyAsync(out_seq + out_offsets[ra], a.out, (size_t)ot, hipMemcpyDeviceToHost, s));
            RB_HIP(hipMemcpyAsync(&over, a.over, 4, hipMemcpyDeviceToHost, s));
            pc.finish();
            if (over) {
                set_error("%s: %u sequences of [%lld, %lld) outgrew their rows (internal error)", who, over, (long long)ra, (long long)rb_);
                throw HipError{RB_ERR_STATE};
            }
        }, 1, cp.data());
    }
    // what the device does not judge, after the pieces' copies have landed: the sequence as it went in, every other field 0
    for (int64_t i = 0; i < n; ++i) {
        if (!why[(size_t)i]) continue;
        const int64_t len = offsets[i + 1] - offsets[i];
        rb_extend_loop_rec v;
        memset(&v, 0, sizeof v);
        v.status = RB_EXTL_NOT_JUDGED; v.why = why[(size_t)i]; v.out_len = (int32_t)len;
        recs[i] = v;
        memset(out_seq + out_offsets[i], 0, (size_t)(out_offsets[i + 1] - out_offsets[i]));
        if (len) memcpy(out_seq + out_offsets[i], seq + offsets[i], (size_t)len);
    }
}

}  // namespace

extern "C" {
int rb_graph_extend_loop(rb_graph *g, int which, const char *seq, const int64_t *offsets, int64_t n, const uint8_t *phase, float min_kmer_cov, int room,
                         int64_t *out_offsets, char *out_seq, rb_extend_loop_rec *recs) {
    return guarded([&] { extend_loop_call(g, which, seq, offsets, n, phase, min_kmer_cov, room, out_offsets, out_seq, recs); });
}
}  // extern "C"
