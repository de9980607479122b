// rb_subsample.hip — the accept / reject loop of SeqSubsampler on the device (rb_subsample_reads): strobemerBased (R/util/SeqSubsampler.java:339-481,
// the loop body :374-460) and kmerBased (:120-337; :150-226 stranded, :233-318 canonical).  The loop is sequential ACROSS reads — a read is judged
// against the counting filter as every earlier kept read left it — and wide INSIDE one: thousands of independent look-ups, one scan, thousands
// of increments.  So the hashes of a piece of reads are made by the sketch kernels and stay on the device (rb_sketch.hip), and then ONE
// workgroup walks the piece's reads one after the other in ONE launch (DESIGN.md §5 "Subsampling of long reads"):
//   look-ups   a lane per element: seen[i] = getCount(hash_i) >= maxMultiplicity, the first seen index and the number unseen by LDS atomics;
//   the scan   the left-to-right fold of the reference as a prefix maximum over the elements (strobemers: of `seen ? end : -inf`, which is
//              namInterval.end; pairs: of `seen ? i : -1`, the last seen pair) and a minimum over the indices at which a `break` fires;
//   the set    HashSet<Long>: an open-addressing table keyed by hash that keeps the smallest index of every hash; an element whose index it keeps
//              is a first occurrence, and a prefix count over those gives every distinct hash its place j in the order of first occurrence;
//   increments increment j draws rng31(seed, ordinal + j, 0) whatever lane applies it.  A second table, keyed by counter index, keeps the smallest
//              and the largest j that touch a counter: an increment all of whose counters have smallest == largest shares none with another
//              increment of the read, commutes with all of them and is applied at once by its lane; the others are applied by one lane in
//              ascending j.  Exact, and no sort.
// Both tables live in LDS up to RB_SUB_LDS_ELEMS entries and in device scratch beyond.  The walker reads counters it wrote a moment earlier: every
// counter access below is a relaxed atomic of agent scope (a load that goes past the vector L1, a store that writes through), and a workgroup barrier
// stands between the phases, so no look-up sees a stale line.  One workgroup waits on nobody.
#include "rb_wave.hpp"
#include "rb_pieces.hpp"
#include "rb_kernels.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

constexpr int SUB_MAX_TPB = 1024;
constexpr int SUB_LDS_SLOTS = 2 * RB_SUB_LDS_ELEMS;          // a table is at most half full
constexpr int SUB_NONE = INT32_MAX;
constexpr int SUB_NEG = INT32_MIN / 2;
constexpr int SUB_SHARED = 1 << 30;                          // mark: the increment shares a counter with another one of the read
constexpr int SUB_UNSEEN = -1, SUB_SEEN = -2;                // mark before the set: a candidate for the set / not one

// key ~0: empty.  The set: lo = the smallest element index with this hash.  The counter table: lo / hi = the smallest / largest increment on this counter.
struct SubSlot { unsigned long long key; uint32_t lo, hi; };

struct SubArgs {
    FilterView fv;
    int mode, k, canonical, edge, chain;     // edge: maxEdgeClip (strobemer mode: max(maxEdgeClip, wMax)); chain: missingChainThreshold
    float mult;                              // (float) maxMultiplicity
    const uint64_t *ha;                      // strobemer hashes / forward k-mer hashes
    const uint64_t *hr;                      // reverse k-mer hashes (canonical pairs)
    const int32_t *hend;                     // getInterval's end of every strobemer
    const int64_t *eoff;                     // pn + 1: where a read's strobemers / k-mers start
    const int32_t *len;                      // letters of a read
    int64_t pn;
    uint8_t *keep;
    int32_t *recs;                           // 8 ints a read
    int32_t *mark;                           // an int per candidate of the read at hand
    SubSlot *scratch;                        // (1 << scratch_log2) + 1 slots, or nullptr where LDS holds every read of the piece
    uint32_t scratch_log2;
    unsigned long long *tot;                 // kept, increments, not judged
};

__device__ __forceinline__ uint32_t ctr_load(uint8_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ctr_store(uint8_t *p, uint32_t v) { __hip_atomic_store(p, (uint8_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// a table of 1 << log2cap slots and one more, for the key that looks like an empty slot
__device__ __forceinline__ void sub_clear(SubSlot *t, uint32_t log2cap) {
    for (uint32_t s = threadIdx.x; s <= (1u << log2cap); s += blockDim.x) { t[s].key = ~0ull; t[s].lo = ~0u; t[s].hi = 0u; }
}
__device__ __forceinline__ SubSlot *sub_insert(SubSlot *t, uint32_t log2cap, uint64_t key) {
    if (key == ~0ull) return &t[1u << log2cap];
    const uint64_t mask = (1ull << log2cap) - 1ull;
    uint64_t s = slot_of(key, log2cap);
    for (;;) {
        const unsigned long long cur = __hip_atomic_load(&t[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == key) return &t[s];
        if (cur == ~0ull) {
            const unsigned long long old = atomicCAS(&t[s].key, ~0ull, (unsigned long long)key);
            if (old == ~0ull || old == key) return &t[s];
        }
        s = (s + 1ull) & mask;
    }
}
// ... of a key that was inserted, behind a barrier
__device__ __forceinline__ const SubSlot *sub_find(const SubSlot *t, uint32_t log2cap, uint64_t key) {
    if (key == ~0ull) return &t[1u << log2cap];
    const uint64_t mask = (1ull << log2cap) - 1ull;
    uint64_t s = slot_of(key, log2cap);
    while (t[s].key != key) s = (s + 1ull) & mask;
    return &t[s];
}
// the smallest table that `entries` keys fill to a half at most
__device__ __forceinline__ uint32_t sub_log2cap(int64_t entries) {
    uint32_t l = 6;
    while (((int64_t)1 << l) < 2 * entries) ++l;
    return l;
}

// one read as the walker sees it
struct SubRead {
    const uint64_t *a, *r;
    const int32_t *e;
    int start, m;                            // k-mer mode: the pairs [start, start + m)
};
// HashFunction.combineHashValues of k-mers i and i + shift, or the smaller of that and the reverse strand's (:181, :266-268)
__device__ __forceinline__ uint64_t sub_pair(const SubArgs &A, const SubRead &R, int i, int shift) {
    uint64_t p = combine(R.a[i], R.a[i + shift]);
    if (A.canonical) p = smin(p, combine(R.r[i + shift], R.r[i]));
    return p;
}
// candidate q of the set: strobemer q, or the q-th pair of the gap-1 list, then the gap-2 list, then the gap-0 list (:204-217)
__device__ __forceinline__ uint64_t sub_cand(const SubArgs &A, const SubRead &R, int q) {
    if (A.mode == RB_SUB_STROBEMER) return R.a[q];
    if (q < R.m) return sub_pair(A, R, R.start + q, A.k + 1);
    if (q < 2 * R.m - 1) return sub_pair(A, R, R.start + q - R.m, A.k + 2);
    return sub_pair(A, R, R.start + q - (2 * R.m - 1), A.k);
}

// CountingBloomFilter.getCount(hash) >= maxMultiplicity (:235-251: the smallest counter; its early return of 0 is that minimum too)
__device__ __forceinline__ bool sub_seen(const SubArgs &A, uint64_t h) {
    uint32_t mn = 255u;
    for (int j = 0; j < A.fv.cbf_h; ++j) mn = min(mn, ctr_load(A.fv.cbf + index_of(multi_hash(h, (uint32_t)j, A.fv.kmul), A.fv.cbf_mod)));
    return minifloat_to_float(mn) >= A.mult;
}
// CountingBloomFilter.increment(hash) :170-194 with the draw of op ordinal `ord`
__device__ __forceinline__ void sub_increment(const SubArgs &A, uint64_t h, uint64_t ord) {
    uint64_t idx[RB_MAX_HASH];
    uint32_t c[RB_MAX_HASH], was[RB_MAX_HASH];
    for (int j = 0; j < A.fv.cbf_h; ++j) {
        idx[j] = index_of(multi_hash(h, (uint32_t)j, A.fv.kmul), A.fv.cbf_mod);
        c[j] = was[j] = ctr_load(A.fv.cbf + idx[j]);
    }
    cbf_step(c, A.fv.cbf_h, K_INC, rng31(A.fv.seed, ord, 0u));
    for (int j = 0; j < A.fv.cbf_h; ++j) if (c[j] != was[j]) ctr_store(A.fv.cbf + idx[j], c[j]);
}

// what the workgroup shares
struct SubShared {
    int wave[SUB_MAX_TPB / 64];
    int first_seen, first_break, unseen, at_break, break_seen, n_shared;
};

// One step of a scan over the elements in chunks of a workgroup: `v` is this thread's value, `carry` what all chunks before gave (every thread
// holds it).  Returns the combination of everything BEFORE this thread's element and moves carry past the chunk.  Two barriers.
template <class OP> __device__ __forceinline__ int sub_scan_step(SubShared &S, int v, int identity, int &carry, OP op) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6, nw = (blockDim.x + 63u) >> 6;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d, 64); if ((int)lane >= d) inc = op(inc, o); }
    if (lane == 63u) S.wave[w] = inc;
    int ex = __shfl_up(inc, 1, 64);
    if (lane == 0u) ex = identity;
    __syncthreads();
    int pre = carry, all = carry;
    for (uint32_t x = 0; x < nw; ++x) { if (x < w) pre = op(pre, S.wave[x]); all = op(all, S.wave[x]); }
    carry = all;
    __syncthreads();
    return op(pre, ex);
}

__global__ void __launch_bounds__(SUB_MAX_TPB) k_subsample_walk(SubArgs A) {
    extern __shared__ SubSlot s_tab[];                       // SUB_LDS_SLOTS + 1 slots
    __shared__ SubShared S;
    const int tid = (int)threadIdx.x, T = (int)blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool strobe = A.mode == RB_SUB_STROBEMER;
    const auto imax = [](int a, int b) { return a > b ? a : b; };
    const auto iadd = [](int a, int b) { return a + b; };
    uint64_t ord = A.fv.ordinal0;
    unsigned long long kept = 0, notjudged = 0;
    for (int64_t rd = 0; rd < A.pn; ++rd) {
        const int len = A.len[rd];
        const int64_t eb = A.eoff[rd];
        const int ne = (int)(A.eoff[rd + 1] - eb);
        SubRead R{A.ha + eb, A.hr ? A.hr + eb : nullptr, A.hend ? A.hend + eb : nullptr, 0, 0};
        int status = RB_SUB_DROPPED, line = 0, idx = -1, f3 = -1, f4 = -1, nscan = 0, unseen = 0, distinct = 0;
        bool judge = true;
        if (strobe) {
            if (ne == 0) { status = RB_SUB_KEPT_START_FAILED; line = RB_SUB_LINE_START_FAILED; judge = false; }      // :456-460
            nscan = ne;
        } else {
            if (ne == 0) { line = A.canonical ? RB_SUB_LINE_KMER_START_FAILED_C : RB_SUB_LINE_KMER_START_FAILED; judge = false; }
            else {
                const bool too_short = (int64_t)len < 3 * (int64_t)A.edge;                                         // :155, :167-175
                R.start = too_short ? 0 : A.edge;
                const int64_t m = (int64_t)ne - (too_short ? 0 : A.edge) - (A.k + 1) - R.start;
                f3 = R.start;
                if (m < 0) { status = RB_SUB_NOT_JUDGED; line = A.canonical ? RB_SUB_LINE_KMER_RANGE_C : RB_SUB_LINE_KMER_RANGE; judge = false; ++notjudged; }
                else R.m = nscan = (int)m;
            }
        }
        bool write = false;
        if (judge) {
            // ---- the look-ups ----
            __syncthreads();                                  // (nobody still reads what the read before left in S)
            if (tid == 0) { S.first_seen = SUB_NONE; S.first_break = SUB_NONE; S.unseen = 0; S.at_break = 0; S.break_seen = 0; }
            __syncthreads();
            int mine = 0;
            for (int i = tid; i < nscan; i += T) {
                const bool seen = sub_seen(A, strobe ? R.a[i] : sub_pair(A, R, R.start + i, A.k + 1));
                A.mark[i] = seen ? SUB_SEEN : SUB_UNSEEN;
                if (seen) atomicMin(&S.first_seen, i); else ++mine;
            }
            for (int s = 32; s > 0; s >>= 1) mine += __shfl_xor(mine, s, 64);
            if (lane == 0u && mine) atomicAdd(&S.unseen, mine);
            __syncthreads();
            const int first = S.first_seen;
            unseen = S.unseen;
            // ---- the scan ----
            if (strobe) {
                const int b0 = A.edge + 1;                    // the first start beyond the left edge region: with namInterval null it breaks (:402, :414)
                if (b0 < nscan && b0 <= first) {
                    write = true; status = RB_SUB_KEPT_SCAN; idx = b0;
                    line = b0 == first ? RB_SUB_LINE_SEEN_BEYOND_EDGE : RB_SUB_LINE_UNSEEN_BEYOND_EDGE;
                } else if (first == SUB_NONE) {               // no break, namInterval null: the tail test keeps the read (:429-434)
                    write = true; status = RB_SUB_KEPT_TAIL; line = RB_SUB_LINE_TAIL;
                } else {
                    // namInterval = (first, the largest end of the seen strobemers so far); element i > first breaks when it is seen and
                    // getOverlap = min(namInterval.end, end_i) - i <= 0 (:408), or unseen and i > namInterval.end (:421)
                    int carry = SUB_NEG, brk = SUB_NONE;
                    for (int base = (first / T) * T; base < nscan && brk == SUB_NONE; base += T) {
                        const int i = base + tid;
                        const bool in = i < nscan, seen = in && A.mark[i] == SUB_SEEN;
                        const int e = seen ? R.e[i] : SUB_NEG;
                        const int before = sub_scan_step(S, e, SUB_NEG, carry, imax);
                        if (in && i > first && (seen ? min(before, e) <= i : i > before)) atomicMin(&S.first_break, i);
                        __syncthreads();
                        brk = S.first_break;
                        if (i == brk) { S.at_break = before; S.break_seen = seen ? 1 : 0; }
                    }
                    __syncthreads();
                    f3 = first;
                    if (brk != SUB_NONE) {
                        write = true; status = RB_SUB_KEPT_SCAN; idx = brk; f4 = S.at_break;
                        line = S.break_seen ? RB_SUB_LINE_MERGE_FAILED : RB_SUB_LINE_GAP;
                    } else {
                        f4 = carry; line = RB_SUB_LINE_TAIL;
                        if (f3 > A.edge || (int64_t)f4 < (int64_t)len - A.edge - 1) { write = true; status = RB_SUB_KEPT_TAIL; }
                    }
                }
            } else {
                // missingChainLen at pair i = i - (the last seen pair up to i); the first i where it reaches the threshold breaks (:187-195)
                int carry = -1, brk = SUB_NONE;
                for (int base = 0; base < nscan && brk == SUB_NONE; base += T) {
                    const int i = base + tid;
                    const bool in = i < nscan, seen = in && A.mark[i] == SUB_SEEN;
                    const int before = sub_scan_step(S, seen ? i : -1, -1, carry, imax);
                    if (in && !seen && i - before >= A.chain) atomicMin(&S.first_break, i);
                    __syncthreads();
                    brk = S.first_break;
                }
                if (brk != SUB_NONE) {
                    write = true; status = RB_SUB_KEPT_SCAN; idx = R.start + brk; f4 = A.chain;
                    line = A.canonical ? RB_SUB_LINE_KMER_CHAIN_C : RB_SUB_LINE_KMER_CHAIN;
                } else {
                    f4 = nscan ? nscan - 1 - carry : 0;
                    line = A.canonical ? RB_SUB_LINE_KMER_NO_CHAIN_C : RB_SUB_LINE_KMER_NO_CHAIN;
                }
            }
        }
        if (write) {
            // ---- the set of distinct hashes, in order of first occurrence ----
            const int ncand = strobe ? nscan : 3 * R.m;
            if (!strobe) for (int q = tid; q < ncand; q += T) A.mark[q] = SUB_UNSEEN;       // every pair of the three lists is a candidate
            const int64_t entries = strobe ? unseen : ncand;
            uint32_t lg = sub_log2cap(entries);
            SubSlot *t = (1u << lg) <= (uint32_t)SUB_LDS_SLOTS ? s_tab : A.scratch;
            sub_clear(t, lg);
            __syncthreads();
            for (int q = tid; q < ncand; q += T)
                if (A.mark[q] == SUB_UNSEEN) atomicMin(&sub_insert(t, lg, sub_cand(A, R, q))->lo, (uint32_t)q);
            __syncthreads();
            int rank0 = 0;
            for (int base = 0; base < ncand; base += T) {
                const int q = base + tid;
                const bool is_first = q < ncand && A.mark[q] == SUB_UNSEEN && sub_find(t, lg, sub_cand(A, R, q))->lo == (uint32_t)q;
                const int j = sub_scan_step(S, is_first ? 1 : 0, 0, rank0, iadd);
                if (is_first) A.mark[q] = j;
            }
            distinct = rank0;
            // ---- the increments ----
            const int H = A.fv.cbf_h;
            lg = sub_log2cap((int64_t)distinct * H);
            t = (1u << lg) <= (uint32_t)SUB_LDS_SLOTS ? s_tab : A.scratch;
            sub_clear(t, lg);
            if (tid == 0) S.n_shared = 0;
            __syncthreads();
            for (int q = tid; q < ncand; q += T) {
                const int j = A.mark[q];
                if (j < 0) continue;
                const uint64_t h = sub_cand(A, R, q);
                for (int a = 0; a < H; ++a) {
                    SubSlot *s = sub_insert(t, lg, index_of(multi_hash(h, (uint32_t)a, A.fv.kmul), A.fv.cbf_mod));
                    atomicMin(&s->lo, (uint32_t)j); atomicMax(&s->hi, (uint32_t)j);
                }
            }
            __syncthreads();
            for (int q = tid; q < ncand; q += T) {
                const int j = A.mark[q];
                if (j < 0) continue;
                const uint64_t h = sub_cand(A, R, q);
                bool shared = false;
                for (int a = 0; a < H; ++a) {
                    const SubSlot *s = sub_find(t, lg, index_of(multi_hash(h, (uint32_t)a, A.fv.kmul), A.fv.cbf_mod));
                    shared = shared || s->lo != s->hi;
                }
                if (shared) { A.mark[q] = j | SUB_SHARED; atomicAdd(&S.n_shared, 1); }
                else sub_increment(A, h, ord + (uint64_t)j);
            }
            __syncthreads();
            if (tid < 64 && S.n_shared) {                     // the increments that share a counter (with a filter of a realistic size: rarely any): one lane, ascending j
                for (int base = 0; base < ncand; base += 64) {
                    const int q = base + (int)lane;
                    unsigned long long todo = __ballot(q < ncand && A.mark[q] >= SUB_SHARED);
                    for (; todo; todo &= todo - 1ull) {
                        const int qq = base + (int)__builtin_ctzll(todo);
                        if (lane == 0u) sub_increment(A, sub_cand(A, R, qq), ord + (uint64_t)(A.mark[qq] & ~SUB_SHARED));
                    }
                }
            }
            __syncthreads();
            ord += (uint64_t)distinct;
        }
        const bool keep = write || status == RB_SUB_KEPT_START_FAILED;
        kept += keep ? 1ull : 0ull;
        if (tid == 0) {
            A.keep[rd] = keep ? 1 : 0;
            int32_t *rec = A.recs + rd * 8;
            rec[0] = status; rec[1] = line; rec[2] = idx; rec[3] = f3; rec[4] = f4; rec[5] = nscan; rec[6] = unseen; rec[7] = distinct;
        }
    }
    if (tid == 0) { A.tot[0] = kept; A.tot[1] = ord - A.fv.ordinal0; A.tot[2] = notjudged; }
}

int walker_tpb() {                                           // 256 and 1024 were measured (profiles/subsample_bench.txt): 1024 is the faster; RB_SUB_TPB is the bench's switch
    const char *e = getenv("RB_SUB_TPB");
    const int v = e ? atoi(e) : 0;
    return v >= 64 && v <= SUB_MAX_TPB && v % 64 == 0 ? v : SUB_MAX_TPB;
}

void subsample_call(rb_graph *g, const rb_subsample_params *p, const char *seq, const int64_t *offsets, int64_t n, uint8_t *out_keep, int32_t *out_recs,
                    int64_t *totals) {
    const char *who = "rb_subsample_reads";
    RB_REQUIRE(g && p && (out_keep || n == 0), "%s: null argument", who);
    RB_REQUIRE(!g->shard, "%s: a shard handle (the loop needs the whole counting filter in one place)", who);
    RB_REQUIRE(n >= 0, "%s: n_reads = %lld", who, (long long)n);
    RB_REQUIRE(p->mode == RB_SUB_STROBEMER || p->mode == RB_SUB_KMER, "%s: mode = %d", who, p->mode);
    RB_REQUIRE(p->k == g->k, "%s: k = %d, the handle hashes for k = %d", who, p->k, g->k);
    if (p->mode == RB_SUB_STROBEMER) RB_REQUIRE(p->wmin >= 1 && p->wmax >= p->wmin && p->wmax <= (1 << 20), "%s: wmin = %d, wmax = %d", who, p->wmin, p->wmax);
    RB_REQUIRE(p->max_multiplicity >= 1, "%s: max_multiplicity = %d (>= 1)", who, p->max_multiplicity);
    RB_REQUIRE(p->max_edge_clip >= 0 && p->max_edge_clip <= (1 << 28), "%s: max_edge_clip = %d (0 .. 2^28)", who, p->max_edge_clip);
    if (totals) totals[0] = totals[1] = totals[2] = totals[3] = 0;
    if (n == 0) return;
    RB_REQUIRE(offsets, "%s: null offsets", who);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t l = offsets[i + 1] - offsets[i];
        RB_REQUIRE(l >= 0, "%s: offsets[%lld] > offsets[%lld]", who, (long long)i, (long long)i + 1);
        RB_REQUIRE(l <= (1 << 24), "%s: read %lld has %lld letters, more than 2^24", who, (long long)i, (long long)l);
    }
    RB_REQUIRE(offsets[n] == offsets[0] || seq, "%s: null sequence text", who);
    WriteLock wl(g->rw);
    RB_REQUIRE(g->cbf, "%s: the handle has no counting filter", who);
    RB_HIP(hipSetDevice(g->p.device));
    RB_HIP(hipStreamSynchronize(g->stream));
    const bool strobe = p->mode == RB_SUB_STROBEMER;
    const size_t lds = ((size_t)SUB_LDS_SLOTS + 1) * sizeof(SubSlot);
    RB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_subsample_walk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    SubArgs a{};
    a.mode = p->mode; a.k = p->k; a.canonical = !strobe && p->canonical != 0;
    a.edge = strobe ? std::max(p->max_edge_clip, p->wmax) : p->max_edge_clip;                    // :363
    a.chain = 2 * p->k + 1;                                                                      // :133
    a.mult = (float)p->max_multiplicity;
    Event ev[2];
    for (Event &e : ev) RB_HIP(hipEventCreate(&e.e));
    DevBuf d_a, d_r, d_e, d_eoff, d_len, d_keep, d_rec, d_mark, d_scratch, d_tot;
    d_tot.reserve(3 * 8);
    std::vector<int64_t> eoff;
    std::vector<int32_t> len, recs_host;
    double walker_ms = 0;
    const std::vector<int64_t> cut = piece_cuts_by_cost([&](int64_t i) { return offsets[i + 1] - offsets[i]; }, n, query_piece_max((int64_t)16 << 20));
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        const int64_t ra = cut[c], pn = cut[c + 1] - ra;
        eoff.assign((size_t)pn + 1, 0);
        if (strobe) sketch_strobemers_device(g->p.device, seq, offsets + ra, pn, p->k, 3, p->wmin, p->wmax, eoff.data(), d_a, d_e);
        else sketch_kmer_hashes_device(g->p.device, seq, offsets + ra, pn, p->k, a.canonical != 0, eoff, d_a, d_r);
        len.resize((size_t)pn);
        int64_t most = 1;                                       // candidates of the piece's largest read
        for (int64_t i = 0; i < pn; ++i) {
            len[(size_t)i] = (int32_t)(offsets[ra + i + 1] - offsets[ra + i]);
            most = std::max(most, (strobe ? 1 : 3) * (eoff[(size_t)i + 1] - eoff[(size_t)i]));
        }
        d_eoff.reserve(eoff.size() * 8); d_len.reserve(len.size() * 4 + 4); d_keep.reserve((size_t)pn + 4); d_rec.reserve((size_t)pn * 32);
        d_mark.reserve((size_t)most * 4);
        uint32_t lg = 6;
        while (((int64_t)1 << lg) < 2 * most * g->p.cbf_num_hash) ++lg;
        if ((1u << lg) > (uint32_t)SUB_LDS_SLOTS) d_scratch.reserve((((size_t)1 << lg) + 1) * sizeof(SubSlot));
        RB_HIP(hipMemcpyAsync(d_eoff.p, eoff.data(), eoff.size() * 8, hipMemcpyHostToDevice, g->stream));
        RB_HIP(hipMemcpyAsync(d_len.p, len.data(), len.size() * 4, hipMemcpyHostToDevice, g->stream));
        a.fv = g->view(g->ordinal, 0, false);
        a.ha = d_a.as<uint64_t>(); a.hr = a.canonical ? d_r.as<uint64_t>() : nullptr; a.hend = strobe ? d_e.as<int32_t>() : nullptr;
        a.eoff = d_eoff.as<int64_t>(); a.len = d_len.as<int32_t>(); a.pn = pn;
        a.keep = d_keep.as<uint8_t>(); a.recs = d_rec.as<int32_t>(); a.mark = d_mark.as<int32_t>();
        a.scratch = d_scratch.as<SubSlot>(); a.scratch_log2 = lg;
        a.tot = d_tot.as<unsigned long long>();
        RB_HIP(hipEventRecord(ev[0], g->stream));
        hipLaunchKernelGGL(k_subsample_walk, dim3(1), dim3(walker_tpb()), lds, g->stream, a);
        RB_HIP(hipGetLastError());
        RB_HIP(hipEventRecord(ev[1], g->stream));
        unsigned long long tot[3] = {0, 0, 0};
        recs_host.resize((size_t)pn * 8);
        RB_HIP(hipMemcpyAsync(out_keep + ra, d_keep.p, (size_t)pn, hipMemcpyDeviceToHost, g->stream));
        RB_HIP(hipMemcpyAsync(recs_host.data(), d_rec.p, (size_t)pn * 32, hipMemcpyDeviceToHost, g->stream));
        RB_HIP(hipMemcpyAsync(tot, d_tot.p, sizeof(tot), hipMemcpyDeviceToHost, g->stream));
        RB_HIP(hipStreamSynchronize(g->stream));
        float ms = 0;
        RB_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        walker_ms += ms;
        g->ordinal += tot[1];
        if (out_recs) memcpy(out_recs + ra * 8, recs_host.data(), (size_t)pn * 32);
        if (totals) { totals[0] += (int64_t)tot[0]; totals[1] += (int64_t)tot[1]; totals[2] += (int64_t)tot[2]; }
        // the counters moved: what the prefilter caches assert stays true (counters only grow)
    }
    if (totals) totals[3] = (int64_t)(walker_ms * 1e6);
}

}  // namespace
}  // namespace rb

extern "C" {
int rb_subsample_reads(rb_graph *cbf, const rb_subsample_params *p, const char *seq, const int64_t *offsets, int64_t n_reads, uint8_t *out_keep,
                       int32_t *out_recs, int64_t *totals) {
    return rb::guarded([&] { rb::subsample_call(cbf, p, seq, offsets, n_reads, out_keep, out_recs, totals); });
}
}  // extern "C"
