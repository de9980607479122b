// rb_naive_frag.hip — naive extension of fragments on the device (rb_graph_naive_extend_fragments): GraphUtils.naiveExtend(kmers, graph,
// maxTipLength, minKmerCov) (R/util/GraphUtils.java:6935-6957), the list form the FragmentAssembler runs on every connected fragment when
// extendFragments is on (R/RNABloom.java:2214).  ONE kernel, a wavefront per fragment: the left walk (naiveExtendLeft :6959-7012 from kmers[0],
// terminators = the fragment's k-mers), then the right walk (naiveExtendRight :6780-6833 from kmers[last], terminators = the fragment's k-mers
// and the left extension) without a trip to the host between them.  Nothing is written to the graph (DESIGN.md §5 "Naive extension of fragments").
//   The text: a row of 2-bit codes, a byte each, in device scratch with `room` free letters on both sides, so both walks append in place.
//   The terminators: ONE open-addressing table for both walks, linear probing, at most half full.  An entry is 64 bits: the upper half of the
// k-mer's forward hash above the k-mer's start in the row + 1 — never 0, which marks an empty slot, so the hash 0 needs no presence mark of its own
// (rb_trim.hip's TrSet stores whole hashes and keeps one).  The wavefront hashes the fragment's k-mers itself — a lane a stretch of the list, rolling —
// and inserts them with compare-and-swap; every accepted step adds one entry, the left extension's in the same table, so the right walk finds
// it there.  A probe is 64 consecutive slots a time, a lane each, up to the first empty one; a lane whose half hash is equal confirms on the k
// bases (Kmer.equals compares bytes), and the lowest start among the confirmed ones is the hit: equal k-mers of a fragment have an entry each.
// The table is a wavefront's share of LDS while the fragment's k-mers + 2 room are at most NF_LDS_ENTRIES, else a row of device scratch.
//   A step, the body of k_naive_extend mode 0 (rb_query.hip) in its order: the four neighbours and the three variants of the current k-mer in the
// base about to leave are looked up by lanes 0 .. 6 at once (count_value, rb_lookup.hpp) and two ballots decide — no neighbour with count >=
// min_kmer_cov ends the walk first, then a variant with count >= 1, then two or more neighbours, then membership of the only candidate, then room.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rb_pieces.hpp"
#include "rb_wave.hpp"

using namespace rb;

namespace {

constexpr int NF_TPB = 128;
constexpr int NF_WAVES = NF_TPB / 64;         // fragments a workgroup works on at a time: a wavefront each
constexpr int NF_LDS_ENTRIES = 1024;          // the most k-mers + 2 room whose table stays in LDS (rnabloom/_native.py NAIVE_FRAG_LDS_ENTRIES)
constexpr int NF_LDS_SLOTS = 2 * NF_LDS_ENTRIES;
constexpr int NF_MAX_SLOTS = 4096;            // wavefronts of a launch at the most (each takes fragments in turn)
constexpr int NF_MAX_LIST = 1 << 24;          // the longest fragment taken, in k-mers
constexpr size_t NF_TAB_BUDGET = (size_t)1 << 30;   // device scratch all wavefronts' tables may take together (one wavefront runs whatever a table costs)
// 16 KB a wavefront, 32 KB a workgroup: five workgroups share a CU's 160 KB of LDS
static_assert((size_t)NF_LDS_SLOTS * 8 * NF_WAVES * 5 <= 160 * 1024, "five workgroups' tables must fit the CU's 160 KB of LDS");

struct NfArgs {
    FilterView fv;
    int stranded, k, room;
    uint32_t tab_cap;                            // slots of a wavefront's table in device scratch (0: every fragment's fits LDS)
    float min_cov;
    int64_t pn;
    const int64_t *kof, *oof;                    // [pn + 1] each: the fragments' k-mer offsets and their places in the rows' letters / the text out
    const uint64_t *codes;                       // the piece's batch: 2-bit codes of its letters
    const uint32_t *woff;
    const uint8_t *phase;
    uint8_t *rT, *out;
    rb_naive_frag_rec *recs;
    uint64_t *tabs;
};

// the terminators and the walk's own k-mers: see the head of the file.  dev: the table is in device scratch and is read and written past the
// vector cache (the inserts are atomics, which do not update it); in LDS a wavefront's accesses are in order.
struct NfSet {
    uint64_t *tab;
    uint32_t mask;
    bool dev;
    __device__ __forceinline__ static uint32_t home(uint64_t h) { return (uint32_t)((h * 0x9E3779B97F4A7C15ull) >> 32); }
    __device__ __forceinline__ static uint64_t entry(uint64_t h, int pos) { return (h & 0xFFFFFFFF00000000ull) | (uint64_t)(uint32_t)(pos + 1); }
    __device__ __forceinline__ void fence() const {
        if (dev) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent"); else wave_fence();
    }
    __device__ __forceinline__ uint64_t load(uint32_t s) const { return __hip_atomic_load(&tab[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    // by one lane, while the others may insert too (the build)
    __device__ __forceinline__ void insert(uint64_t h, int pos) const {
        const unsigned long long e = entry(h, pos);
        for (uint32_t s = home(h) & mask;; s = (s + 1u) & mask)
            if (atomicCAS(reinterpret_cast<unsigned long long *>(&tab[s]), 0ull, e) == 0ull) break;
    }
};

// the k-mer that starts at `pos` of the row against the candidate: the k-mer that starts at np, whose letter at offset nq is `in` (not in the row yet)
__device__ __forceinline__ bool nf_equal(const uint8_t *T, int pos, int np, int nq, uint32_t in, int k) {
    bool eq = true;
    for (int q = 0; q < k && eq; ++q) eq = (uint32_t)T[pos + q] == (q == nq ? in : (uint32_t)T[np + q]);
    return eq;
}

// One walk until it ends; returns how (RB_NFRAG_END_*).  lo, hi: the text's k-mers by their start in the row.  hit: for END_MEMBER the lowest
// start of a k-mer of the text equal to the candidate.
__device__ __forceinline__ int nf_walk(const NfArgs &a, const NfSet &set, uint8_t *T, int &lo, int &hi, bool left, int &hit, uint32_t lane) {
    const int k = a.k;
    const uint32_t uk = (uint32_t)k;
    const WaveDir<> dr = wave_dir(a.stranded, k, left ? 1 : 0);
    int cur = left ? lo : hi - 1, added = 0;
    uint64_t A, B;
    {
        uint64_t f = 0, r = 0;                                                                                  // the k-mer the walk starts on, both strands
        for (int q = 0; q < k; ++q) {
            const uint32_t c = T[cur + q];
            f = rotl(f, 1) ^ seed_of(c);
            r = rotr(r, 1) ^ rotl(seed_of(3u - c), uk - 1u);
        }
        A = left ? r : f; B = left ? f : r;
    }
    for (;;) {
        const uint32_t oc = T[left ? cur + k - 1 : cur];                                                        // the base about to leave
        // lanes 0 .. 3: the neighbour that takes base `lane`; lanes 4 .. 6: the current k-mer with one of the three other bases where oc stands
        const uint32_t in = lane < 4u ? lane : (oc + 1u + (lane - 4u)) & 3u;
        uint64_t nA, nB;
        if (lane < 4u) dr.step(A, B, oc, in, nA, nB);
        else {
            nA = A ^ rotl(seed_of(oc ^ dr.xm), uk - 1u) ^ rotl(seed_of(in ^ dr.xm), uk - 1u);
            nB = B ^ seed_of(oc ^ dr.ym) ^ seed_of(in ^ dr.ym);
        }
        const float c = lane < 7u ? count_value(a.fv, dr.hash(nA, nB)) : 0.0f;
        const unsigned long long good = __ballot(lane < 4u && c >= a.min_cov), back = __ballot(lane >= 4u && lane < 7u && c >= 1.0f);
        if (!good) return RB_NFRAG_END_NO_NEIGHBOUR;                                                            // :6791 `while (!neighbors.isEmpty())`
        if (back) return RB_NFRAG_END_BACK_BRANCH;                                                              // :6794-6799
        if (good & (good - 1ull)) return RB_NFRAG_END_SEVERAL;                                                  // :6805-6819
        const int bl = (int)__builtin_ctzll(good);
        const uint32_t best = (uint32_t)bl;
        A = wave_shfl64(nA, bl); B = wave_shfl64(nB, bl);                                                       // (kept only if the candidate is added: see the returns)
        const uint64_t hf = dr.fwd(A, B);
        const int np = left ? cur - 1 : cur + 1, nq = left ? 0 : k - 1;                                         // the candidate's start, its new letter's offset
        // terminators.contains(best) || usedKmers.contains(best) (:6821): the probe, 64 slots a time up to the first empty one
        int found = INT32_MAX;
        uint32_t free_slot = 0;
        for (uint32_t s0 = NfSet::home(hf);; s0 += 64u) {
            const uint64_t e = set.load((s0 + lane) & set.mask);
            const unsigned long long empties = __ballot(e == 0ull);
            const uint32_t live = empties ? (uint32_t)__builtin_ctzll(empties) : 64u;
            const int pos = (int)(uint32_t)e - 1;
            bool eq = lane < live && (uint32_t)(e >> 32) == (uint32_t)(hf >> 32);
            if (eq) eq = nf_equal(T, pos, np, nq, best, k);
            for (unsigned long long m = __ballot(eq); m; m &= m - 1ull) found = min(found, __shfl(pos, (int)__builtin_ctzll(m), 64));
            if (empties) { free_slot = (s0 + live) & set.mask; break; }
        }
        if (found != INT32_MAX) { hit = found; return RB_NFRAG_END_MEMBER; }
        if (added >= a.room) return RB_NFRAG_END_ROOM;
        if (lane == 0) {
            T[left ? np : np + k - 1] = (uint8_t)best;
            __hip_atomic_store(&set.tab[free_slot], NfSet::entry(hf, np), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        set.fence();
        wave_fence();
        cur = np; ++added;
        if (left) --lo; else ++hi;
    }
}

// fragment r of the piece by one wavefront; its table is its LDS row or — more than NF_LDS_ENTRIES k-mers + 2 room — its row of device scratch
__device__ __forceinline__ void nf_one(const NfArgs &a, uint64_t *lds_tab, uint64_t *dev_tab, int64_t r, uint32_t lane) {
    const int k = a.k, room = a.room;
    const int nk0 = (int)(a.kof[r + 1] - a.kof[r]);
    if (nk0 == 0) return;                                     // not judged: the host writes its record and its text
    const uint32_t uk = (uint32_t)k;
    uint8_t *T = a.rT + a.oof[r];
    {
        const uint64_t *cw = a.codes + a.woff[r];
        for (int p = (int)lane; p < nk0 + k - 1; p += 64) T[room + p] = (uint8_t)((cw[p >> 5] >> (2 * (p & 31))) & 3u);
    }
    const int entries = nk0 + 2 * room;
    uint32_t slots = 64u;
    while (slots < 2u * (uint32_t)entries) slots <<= 1;
    const bool dev = entries > NF_LDS_ENTRIES;
    const NfSet set{dev ? dev_tab : lds_tab, slots - 1u, dev};
    for (uint32_t s = lane; s < slots; s += 64u) set.tab[s] = 0ull;
    wave_fence();
    set.fence();
    {                                                         // the fragment's k-mers: lane l hashes list entries [l per, (l + 1) per), rolling
        const int per = (nk0 + 63) / 64, j0 = (int)lane * per, j1 = min(nk0, j0 + per);
        uint64_t f = 0;
        for (int j = j0; j < j1; ++j) {
            const uint8_t *t = T + room + j;
            if (j == j0) for (int q = 0; q < k; ++q) f = rotl(f, 1) ^ seed_of(t[q]);
            else f = rotl(f, 1) ^ rotl(seed_of(t[-1]), uk) ^ seed_of(t[k - 1]);
            set.insert(f, room + j);
        }
    }
    set.fence();
    rb_naive_frag_rec v;
    v.status = RB_NFRAG_DONE; v.why = RB_NFRAG_WHY_NONE;
    v.left_end = v.right_end = RB_NFRAG_END_NOT_RUN;
    for (int q = 0; q < 7; ++q) v.pad[q] = 0;
    int lo = room, hi = room + nk0, lhit = -1, rhit = -1;
    if (a.phase[r] == 0) v.left_end = nf_walk(a, set, T, lo, hi, true, lhit, lane);
    if (v.left_end != RB_NFRAG_END_ROOM) v.right_end = nf_walk(a, set, T, lo, hi, false, rhit, lane);
    if (v.left_end == RB_NFRAG_END_ROOM || v.right_end == RB_NFRAG_END_ROOM) v.status = RB_NFRAG_ROOM;
    v.left_ext = room - lo; v.right_ext = hi - (room + nk0); v.out_len = hi - lo + k - 1;
    v.left_hit = v.left_end == RB_NFRAG_END_MEMBER ? lhit - lo : -1;
    v.right_hit = v.right_end == RB_NFRAG_END_MEMBER ? rhit - lo : -1;
    uint8_t *o = a.out + a.oof[r];
    for (int p = (int)lane; p < v.out_len; p += 64) o[p] = code_letter(T[lo + p]);
    if (lane == 0) a.recs[r] = v;
}

// A wavefront per fragment, taking fragments in turn.
__global__ void __launch_bounds__(NF_TPB) k_naive_frag(NfArgs a) {
    __shared__ uint64_t s_tab[NF_WAVES][NF_LDS_SLOTS];
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const int64_t slot = (int64_t)blockIdx.x * NF_WAVES + wv, n_slots = (int64_t)gridDim.x * NF_WAVES;
    uint64_t *dev_tab = a.tabs + (size_t)slot * a.tab_cap;
    for (int64_t r = slot; r < a.pn; r += n_slots) {
        nf_one(a, s_tab[wv], dev_tab, r, lane);
        wave_fence();
    }
}

void naive_frag_call(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, const uint8_t *phase, float min_cov, int room,
                     int64_t *out_offsets, char *out_seq, rb_naive_frag_rec *recs) {
    const char *who = "rb_graph_naive_extend_fragments";
    RB_REQUIRE(g, "%s: null handle", who);
    RB_REQUIRE(!g->shard, "%s: not available on a shard handle", who);
    RB_REQUIRE(g->dbg.bits && g->cbf, "%s: dbgbf or the counting filter has been destroyed", who);
    RB_REQUIRE(std::isfinite(min_cov) && min_cov >= 0.0f, "%s: min_kmer_cov must be finite and not negative", who);
    RB_REQUIRE(room >= 1 && room <= (1 << 24), "%s: room = %d (1 .. 2^24)", who, room);
    RB_REQUIRE(n >= 0, "%s: n = %lld", who, (long long)n);
    if (n == 0) return;
    const int k = g->k;
    RB_REQUIRE(offsets && out_offsets, "%s: null argument", who);
    RB_REQUIRE(recs || !out_seq, "%s: out_seq needs recs", who);
    RB_REQUIRE(offsets[n] == offsets[0] || seq, "%s: null sequence text", who);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        RB_REQUIRE(len >= 0, "%s: offsets[%lld] > offsets[%lld]", who, (long long)i, (long long)i + 1);
        RB_REQUIRE(len - k + 1 <= NF_MAX_LIST, "%s: sequence %lld has more than %d k-mers", who, (long long)i, NF_MAX_LIST);
        if (phase) RB_REQUIRE(phase[i] <= 1, "%s: phase[%lld] = %d (0: both sides, 1: the right side only)", who, (long long)i, (int)phase[i]);
    }
    // the capacity layout: len + 2 room letters a sequence
    out_offsets[0] = 0;
    for (int64_t i = 0; i < n; ++i) out_offsets[i + 1] = out_offsets[i] + (offsets[i + 1] - offsets[i]) + 2 * (int64_t)room;
    if (!out_seq) return;
    // What the device judges: at least k letters, all of them upper-case A C G T (the reference compares k-mers as bytes and added letters are
    // upper-case).  The rest comes back as it went in and is an empty sequence to the device.  Pieces are cut by capacity k-mers (cp).
    std::vector<int64_t> to((size_t)n + 1, 0), ko((size_t)n + 1), cp((size_t)n + 1, 0);
    std::vector<uint8_t> why((size_t)n, RB_NFRAG_WHY_NONE);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        const char *t = seq + offsets[i];
        if (len < k) why[(size_t)i] = RB_NFRAG_WHY_NO_KMER;
        else for (int64_t p = 0; p < len; ++p) if (t[p] != 'A' && t[p] != 'C' && t[p] != 'G' && t[p] != 'T') { why[(size_t)i] = RB_NFRAG_WHY_LETTER; break; }
        to[(size_t)i + 1] = to[(size_t)i] + (why[(size_t)i] ? 0 : len);
        cp[(size_t)i + 1] = cp[(size_t)i] + std::max<int64_t>(0, len + 2 * (int64_t)room - k + 1);
    }
    std::vector<char> text((size_t)to[(size_t)n]);
    for (int64_t i = 0; i < n; ++i)
        if (!why[(size_t)i]) memcpy(text.data() + to[(size_t)i], seq + offsets[i], (size_t)(offsets[i + 1] - offsets[i]));
    kmer_offsets(to.data(), n, k, ko.data(), nullptr);
    if (ko[(size_t)n] > 0) {
        RB_HIP(hipSetDevice(g->p.device));
        HostPin pin_out(out_seq, (size_t)out_offsets[n]), pin_rec(recs, (size_t)n * sizeof(rb_naive_frag_rec));
        QueryLease q(g);
        hipStream_t s = q.c->st;
        // piece by piece (rb_pieces.hpp), cut by capacity k-mers: b0 the piece's table (k-mer offsets, places in the rows), b3 records, phases, the
        // rows (2 bytes a capacity letter: the code and the text out) and the tables of the wavefronts whose fragment's does not fit LDS
        std::vector<int64_t> tab;
        for_each_host_piece(g, s, text.data(), to.data(), ko.data(), n, "naive_extend_fragments", (int64_t)16 << 20, [&](HostPiece &pc) {
            const int64_t ra = pc.ra, rb_ = pc.rb, pn = pc.pn;
            const int64_t ot = out_offsets[rb_] - out_offsets[ra];
            int64_t longest = 0;
            tab.resize(2 * ((size_t)pn + 1));
            for (int64_t i = 0; i <= pn; ++i) {
                tab[(size_t)i] = ko[(size_t)(ra + i)] - ko[(size_t)ra];
                tab[(size_t)(pn + 1 + i)] = out_offsets[ra + i] - out_offsets[ra];
                if (i < pn) longest = std::max(longest, ko[(size_t)(ra + i + 1)] - ko[(size_t)(ra + i)]);
            }
            uint32_t tab_cap = 0;
            if (longest + 2 * (int64_t)room > NF_LDS_ENTRIES) { tab_cap = 64; while ((int64_t)tab_cap < 2 * (longest + 2 * (int64_t)room)) tab_cap <<= 1; }
            const int64_t max_slots = tab_cap ? std::max<int64_t>(1, std::min<int64_t>(NF_MAX_SLOTS, (int64_t)(NF_TAB_BUDGET / ((size_t)tab_cap * 8)))) : NF_MAX_SLOTS;
            const int64_t slots = std::min<int64_t>(pn, max_slots);
            const unsigned blocks = blocks_for(slots, NF_WAVES);
            const size_t o_rec = 0, o_ph = o_rec + (size_t)pn * sizeof(rb_naive_frag_rec), o_t = up16(o_ph + (size_t)pn), o_out = up16(o_t + (size_t)ot),
                         o_tabs = up16(o_out + (size_t)ot);
            q.c->b0.reserve(tab.size() * 8);
            q.c->b3.reserve(o_tabs + (size_t)blocks * NF_WAVES * (size_t)tab_cap * 8 + 16);
            uint8_t *base3 = q.c->b3.as<uint8_t>();
            const rb_batch *b = pc.batch();
            NfArgs a;
            a.fv = g->view(0, 0);
            a.stranded = (int)g->stranded; a.k = k; a.room = room; a.tab_cap = tab_cap; a.min_cov = min_cov;
            a.pn = pn;
            a.kof = q.c->b0.as<int64_t>(); a.oof = a.kof + pn + 1;
            a.codes = b->codes; a.woff = b->woff;
            a.recs = reinterpret_cast<rb_naive_frag_rec *>(base3 + o_rec);
            a.phase = base3 + o_ph;
            a.rT = base3 + o_t; a.out = base3 + o_out;
            a.tabs = reinterpret_cast<uint64_t *>(base3 + o_tabs);
            RB_HIP(hipMemcpyAsync(q.c->b0.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
            RB_HIP(hipMemsetAsync(base3 + o_rec, 0, o_t - o_rec, s));                 // (records no wavefront writes, phase 0)
            RB_HIP(hipMemsetAsync(base3 + o_out, 0, (size_t)ot, s));                  // (zeros behind every text, whatever the cuts)
            if (phase) RB_HIP(hipMemcpyAsync(base3 + o_ph, phase + ra, (size_t)pn, hipMemcpyHostToDevice, s));
            pc.kernels_begin();
            hipLaunchKernelGGL(k_naive_frag, dim3(blocks), dim3(NF_TPB), 0, s, a);
            RB_HIP(hipGetLastError());
            pc.kernels_end();
            RB_HIP(hipMemcpyAsync(recs + ra, a.recs, (size_t)pn * sizeof(rb_naive_frag_rec), hipMemcpyDeviceToHost, s));
            RB_HIP(hipMemcpyAsync(out_seq + out_offsets[ra], a.out, (size_t)ot, hipMemcpyDeviceToHost, s));
        }, 1, cp.data());
    }
    // what the device does not judge, after the pieces' copies have landed: the sequence as it went in, no hit, every other field 0
    for (int64_t i = 0; i < n; ++i) {
        if (!why[(size_t)i]) continue;
        const int64_t len = offsets[i + 1] - offsets[i];
        rb_naive_frag_rec v;
        memset(&v, 0, sizeof v);
        v.status = RB_NFRAG_NOT_JUDGED; v.why = why[(size_t)i]; v.out_len = (int32_t)len;
        v.left_hit = v.right_hit = -1;
        recs[i] = v;
        memset(out_seq + out_offsets[i], 0, (size_t)(out_offsets[i + 1] - out_offsets[i]));
        if (len) memcpy(out_seq + out_offsets[i], seq + offsets[i], (size_t)len);
    }
}

}  // namespace

extern "C" {
int rb_graph_naive_extend_fragments(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, const uint8_t *phase, float min_kmer_cov, int room,
                                    int64_t *out_offsets, char *out_seq, rb_naive_frag_rec *recs) {
    return guarded([&] { naive_frag_call(g, seq, offsets, n, phase, min_kmer_cov, room, out_offsets, out_seq, recs); });
}
}  // extern "C"
