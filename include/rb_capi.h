/*
 * rb_capi.h — C ABI of librb_hip.so, the MI355X (gfx950) implementation of RNA-Bloom's k-mer
 * hashing / Bloom-filter de Bruijn graph hot path.
 *
 * This is the drop-in boundary: plain C, opaque handles, host pointers + sizes, int status codes
 * (0 = RB_OK; message via rb_last_error()).  The reference (bcgsc/RNA-Bloom v2.0.1, Java) has no
 * FFI seam of its own; the entry points below are what a JNI shim for
 * rnabloom.bloom.{BloomFilter,CountingBloomFilter}, rnabloom.bloom.hash.* and
 * rnabloom.graph.BloomFilterDeBruijnGraph would bind (INTEGRATION.md shows that shim).  Each
 * declaration cites the reference method(s) it replaces; R/ = src/rnabloom/ in the reference tree.
 *
 * Semantics are those of the reference run with ONE worker thread (-t 1): filters end up exactly as
 * if the reads had been processed one after another, k-mers left to right.
 * All entry points are synchronous: when they return, results are visible to the next call.
 */
#ifndef RB_CAPI_H
#define RB_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RB_OK 0
#define RB_ERR_INVALID 1   /* bad argument                    (Java: IllegalArgumentException) */
#define RB_ERR_HIP 2       /* HIP runtime / device failure    (Java: RuntimeException)         */
#define RB_ERR_NOMEM 3     /* device or host allocation failed (Java: OutOfMemoryError)        */
#define RB_ERR_STATE 4     /* filter not initialised etc.     (Java: NullPointerException path) */

typedef struct rb_graph rb_graph; /* BloomFilterDeBruijnGraph + its 4 filters, device resident */
typedef struct rb_batch rb_batch; /* a batch of reads, device resident, 2-bit packed          */

/* which-filter selectors: R/graph/BloomFilterDeBruijnGraph.java:39-43 */
enum { RB_DBGBF = 0, RB_CBF = 1, RB_RPKBF = 2, RB_FPKBF = 3 };

/* BloomFilterDeBruijnGraph(long dbgbfNumBits, long cbfNumBytes, long pkbfNumBits, int dbgbfNumHash,
 *   int cbfNumHash, int pkbfNumHash, int k, boolean stranded, boolean useReadPairedKmers)
 * R/graph/BloomFilterDeBruijnGraph.java:75-104 */
typedef struct rb_graph_params {
    int64_t dbgbf_bits;           /* dbgbfNumBits  (any positive long, not a power of two) */
    int64_t cbf_bytes;            /* cbfNumBytes                                             */
    int64_t pkbf_bits;            /* pkbfNumBits   (rpkbf; fpkbf via rb_graph_init_fragment_pairs) */
    int32_t dbgbf_num_hash;       /* 1..RB_MAX_HASH */
    int32_t cbf_num_hash;
    int32_t pkbf_num_hash;
    int32_t k;                    /* 1..RB_MAX_K */
    int32_t stranded;             /* 0 => CanonicalHashFunction, 1 => HashFunction            */
    int32_t use_read_paired_kmers;
    int32_t device;               /* HIP device ordinal                                       */
    int32_t group_bits;           /* tuning: top hash bits the occurrence sort groups on (0 = default 32,
                                     max 64); any value gives identical results (DESIGN.md "split runs") */
    uint64_t rng_seed;            /* seed of the counter-based generator that replaces the
                                     unseeded Math.random() of R/util/MiniFloat.java:34        */
    int64_t max_batch_kmers;      /* 0 = default; upper bound on k-mers per internal sub-batch */
} rb_graph_params;

#define RB_MAX_HASH 8
#define RB_MAX_K 256

/* flags of rb_graph_add_* : constructor arguments of the stage-1 workers,
 * R/RNABloom.java:535-548 (FastqToGraphWorker) / :655-668 (FastaToGraphWorker) */
#define RB_ADD_REVCOMP 1u          /* reverseComplement: RC iterators (no-op when !stranded,
                                      R/bloom/hash/CanonicalHashFunction.java:188-206)          */
#define RB_ADD_COUNT_IF_PRESENT 2u /* incrementIfPresent: graph::addCountIfPresent             */
#define RB_ADD_STORE_READ_PAIRS 4u /* storeReadPairedKmers: graph.addReadSingleKmerPair        */
#define RB_ADD_PAIRS_IF_PRESENT 8u /* rb_graph_add_pairs: existingKmersOnly (both k-mers in dbgbf) */

typedef struct rb_add_stats {
    int64_t reads;    /* reads consumed (each takes one op ordinal)                 */
    int64_t kmers;    /* graph.add / addCountIfPresent calls performed              */
    int64_t pairs;    /* graph.addReadSingleKmerPair calls performed                */
    int64_t distinct; /* distinct k-mer hashes seen per sub-batch, summed           */
    int64_t conflict_ops; /* ops replayed in order because they shared a counter with another k-mer */
    int64_t sorted_kmers; /* occurrences that survived the no-op prefilter and were grouped (<= kmers) */
} rb_add_stats;

const char *rb_last_error(void); /* thread-local message of the last failing call */
int rb_version(void);
/* 16 hex digits identifying the kernel sources this library was built from (tools/csrc_id.py); no reference counterpart:
 * bench.py uses it to tie committed rocprofv3 counter summaries to the code they profiled */
const char *rb_build_id(void);

/* ---- graph lifetime: ctor :75-104, destroyXxx / clearXxx :332-350 (explicit off-heap lifetime,
 *      R/bloom/buffer/UnsafeByteBuffer.java:44,152-155) ---- */
int rb_graph_create(const rb_graph_params *p, rb_graph **out);
int rb_graph_destroy(rb_graph *g);
int rb_graph_clear(rb_graph *g, unsigned which_mask /* bit i = filter i; also resets the op ordinal when all */);
/* setReadPairedKmerDistance :375-377, setFragPairedKmerDistance :367-369 */
int rb_graph_set_read_paired_kmer_distance(rb_graph *g, int d);
int rb_graph_set_frag_paired_kmer_distance(rb_graph *g, int d);
/* initializePairKmersBloomFilter(long pkbfNumBits, int pkbfNumHash) :352-359 */
int rb_graph_init_fragment_pairs(rb_graph *g, int64_t pkbf_bits, int pkbf_num_hash);
int rb_graph_get_op_ordinal(rb_graph *g, uint64_t *out);
int rb_graph_set_op_ordinal(rb_graph *g, uint64_t v);

/* ---- read batches (the build's counterpart of FastqReader/FastaReader + the per-read regex
 *      segmentation of R/RNABloom.java:572-577, R/util/SeqUtils.java:1432-1438) ----
 * seq: concatenated ASCII bases; qual: concatenated PHRED+33 or NULL (FASTA: no quality pass);
 * offsets[n_reads+1]: read i = seq[offsets[i], offsets[i+1]).  A base is usable iff it is one of
 * ACGTUacgtu and (qual == NULL or '!'+min_base_qual <= qual <= '~').  Encoding to the packed
 * device format (2-bit codes + validity bit per base) runs on the GPU. */
int rb_batch_create_ascii(int device, const char *seq, const char *qual, const int64_t *offsets,
                          int64_t n_reads, int min_base_qual, rb_batch **out);
int rb_batch_destroy(rb_batch *b);
int rb_batch_info(const rb_batch *b, int64_t *n_reads, int64_t *n_bases, int64_t *device_bytes);
/* copy reads [first, first+n) back as ASCII with 'N' at unusable positions (for checkers) */
int rb_batch_download_ascii(const rb_batch *b, int64_t first, int64_t n, char *seq /* len = sum of lens */,
                            int64_t *offsets /* n+1 */);
/* synthetic paired-end reads generated on the device (bench data; SURVEY.md §8(d) model).
 * Produces 2*n_pairs reads: left reads 0..n_pairs-1 then right reads (as sequenced). */
typedef struct rb_synth_params {
    int64_t n_pairs;
    int64_t genome_bases;   /* G */
    int32_t read_len;       /* 150 */
    int32_t frag_mean, frag_sd;
    float sub_rate;         /* substitution errors (error bases are masked unusable, like PHRED 2) */
    float n_rate;
    float expr_sigma;       /* log-normal sigma; 0 => uniform expression */
    uint64_t seed;
    int32_t tx_min, tx_max; /* transcript length range */
    /* a slice of a larger read set (multi-GPU benches): this batch holds pairs
     * [pair_offset, pair_offset + n_pairs) of a set of total_pairs pairs drawn with the same seed,
     * so the ranks' batches together are exactly the single-GPU set.  total_pairs 0 = n_pairs. */
    int64_t pair_offset, total_pairs;
} rb_synth_params;
int rb_batch_create_synthetic(int device, const rb_synth_params *p, rb_batch **out);

/* ---- stage-1 insert: FastqToGraphWorker.run R/RNABloom.java:551-634 /
 *      FastaToGraphWorker.run :672-724, i.e. per k-mer graph.add (BloomFilterDeBruijnGraph.java:405-412)
 *      or addCountIfPresent (:424-428), per paired k-mer addReadSingleKmerPair (:455-457) ---- */
int rb_graph_add_batch(rb_graph *g, const rb_batch *b, unsigned flags, rb_add_stats *stats);
/* PairedKmersToGraphWorker.run (R/RNABloom.java:436-524): the paired k-mers (distance = the read- or fragment-paired
 * k-mer distance of `which` = RB_RPKBF / RB_FPKBF) of reads [first, first+n) into that pair filter — nothing else.
 * flags: RB_ADD_REVCOMP, RB_ADD_PAIRS_IF_PRESENT (existingKmersOnly, :466-482: only pairs whose two k-mers are both
 * in dbgbf).  stats: reads, pairs. */
int rb_graph_add_pairs(rb_graph *g, const rb_batch *b, int64_t first, int64_t n, int which, unsigned flags, rb_add_stats *stats);
/* FragmentsToGraphWorker.run (R/RNABloom.java:1463-1539): for every fragment graph.addDbgOnly of each k-mer; with
 * load_paired_kmers also addReadSingleKmerPair of its read-paired k-mers and, for fragments long enough to have one,
 * addFragmentSingleKmerPair of its fragment-paired k-mers.  Needs rb_graph_init_fragment_pairs + both distances.
 * stats: reads, kmers, pairs (read + fragment pairs). */
int rb_graph_add_fragments(rb_graph *g, const rb_batch *b, int64_t first, int64_t n, int load_paired_kmers, rb_add_stats *stats);
/* reads [first, first+n) of the batch only */
int rb_graph_add_batch_range(rb_graph *g, const rb_batch *b, int64_t first, int64_t n, unsigned flags,
                             rb_add_stats *stats);
/* FastqToGraphWorker.run (R/RNABloom.java:526-643) over host ASCII reads: the result of rb_batch_create_ascii + rb_graph_add_batch + rb_batch_destroy,
 * as a pipeline.  The caller's arrays are registered for the call (best effort, slab by slab ahead of the copies) and handed back when it returns.
 * Input of more than one piece (256 M bases): ONE insert over a device batch sized for the whole call — lengths and word offsets are computed on the
 * GPU from `offsets`, bases and qualities follow piece by piece through two staging buffers and the 2-bit encode kernel on the handle's copy stream,
 * and the insert works on the pieces that have arrived (csrc/rb_packed.hip add_reads_streamed; 17.7 G k-mers/s for 50 M reads of 150 bases = 15 GB
 * over a 57 GB/s link, HISTORY "Round 6").  Smaller input: one chunk.  stats is added to, not cleared. */
int rb_graph_add_reads(rb_graph *g, const char *seq, const char *qual, const int64_t *offsets,
                       int64_t n_reads, int min_base_qual, unsigned flags, rb_add_stats *stats);

/* ---- per-hash mutators (h0 = hashVals[0]; the library expands it with NTM64 using the graph's k,
 *      R/bloom/hash/NTHash.java:518-527).  n ops are applied in array order; each takes one op
 *      ordinal.  op = one of RB_OP_*. ---- */
enum {
    RB_OP_ADD = 0,              /* add(long[])              :405-412 */
    RB_OP_ADD_IF_ABSENT = 1,    /* addIfAbsent              :414-422 */
    RB_OP_ADD_COUNT_IF_PRESENT = 2, /* addCountIfPresent    :424-428 */
    RB_OP_ADD_DBG_ONLY = 3,     /* addDbgOnly               :430-436 */
    RB_OP_ADD_COUNT_ONLY = 4,   /* addCountOnly             :438-440 */
    RB_OP_ADD_READ_PAIR = 5,    /* addReadSingleKmerPair    :455-457 (h0 = pair hash) */
    RB_OP_ADD_FRAG_PAIR = 6     /* addFragmentSingleKmerPair:459-461 */
};
int rb_graph_apply(rb_graph *g, int op, const uint64_t *h0, size_t n);

/* ---- queries ---- */
/* contains(long[]) :538-540 -> dbgbf.lookup R/bloom/BloomFilter.java:170-178 */
int rb_graph_contains(rb_graph *g, const uint64_t *h0, size_t n, uint8_t *out);
/* getCount(long[]) :562-570 = dbgbf.lookup ? cbf.getCount + 1 : 0 */
int rb_graph_count(rb_graph *g, const uint64_t *h0, size_t n, float *out);
/* BloomFilter.lookup(long) on any bit filter / CountingBloomFilter.getCount(long) :231-233 */
int rb_filter_lookup(rb_graph *g, int which, const uint64_t *h0, size_t n, uint8_t *out);
/* BloomFilter.lookupThenAdd (R/bloom/BloomFilter.java:147-155) for an array of base hashes, IN ARRAY ORDER: out[i] = 1 iff
 * every bit of element i was set before element i is added — by the state before the call or by an element earlier in
 * the array — and all bits are set on return.  This is what graph.lookupAndAddAllPairedKmers
 * (R/graph/BloomFilterDeBruijnGraph.java:513-526) and GraphUtils.java:640-650 AND together per sequence. */
int rb_filter_lookup_then_add(rb_graph *g, int which, const uint64_t *h0, size_t n, uint8_t *out);
int rb_filter_get_count(rb_graph *g, const uint64_t *h0, size_t n, float *out);
/* getKmers(String) :1224-1226 -> {Canonical,}HashFunction.getKmers: for every window of every
 * read of the batch: forward hash, reverse hash (0 when stranded), count (0 for windows that
 * contain a non-ACGTU base).  koffsets[n_reads+1] receives the per-read output offsets
 * (read i has max(0,len_i-k+1) windows); pass f=r=count=NULL to query sizes only.  The call works in pieces of 16 M k-mers
 * (320 MB of device scratch whatever the number of reads).  * On a shard handle (rb_graph_create_shard) only the hashes are local: count = 1 for a usable window, 0 otherwise; the counts of a
 * distributed graph come from one rb_shard_query_* exchange (rnabloom/sharded.py::ShardRank.getKmers). */
int rb_graph_kmers(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n_reads,
                   int64_t *koffsets, uint64_t *f, uint64_t *r, float *count);
/* The counts of getKmers for reads that are already resident in HBM (an rb_batch): out[row(i) + p] = graph.getCount of window p of
 * read first + i (0 for a window with a non-ACGTU base) — the per-read count profile stage 2 reads first
 * (R/RNABloom.java:1984, 2097-2114: graph.getKmers(seq) before correctErrors); hashes are not returned (4 bytes per k-mer instead
 * of 20: the call is bound by the copy back).  koffsets (host, n + 1 entries, koffsets[0] = 0): row(i) = koffsets[i], read i must
 * have koffsets[i+1] - koffsets[i] = max(0, len_i - k + 1) windows; koffsets = NULL: rows of *stride_out = max_len - k + 1 counts
 * (the batch's longest read), shorter reads padded with zeros — for uniform reads that is the packed layout.  out_on_device != 0:
 * `out` is device memory of the graph's device and nothing is copied.  Host buffers are pinned for the call (see
 * rb_graph_add_reads).  A window is usable where the batch marks all its bases valid: for getKmers(String) semantics the batch
 * is one created without a quality threshold (min_base_qual 0 / no qualities).  Results equal rb_graph_kmers' counts and the
 * oracle's (tests/test_gpu_queries.py). */
int rb_graph_batch_counts(rb_graph *g, const rb_batch *b, int64_t first, int64_t n, const int64_t *koffsets, float *out,
                          int out_on_device, int64_t *stride_out);

/* Coverage statistics of segments of the count profile of resident reads — what stage 2 reduces every read's sorted getKmers counts
 * to before it decides whether the read needs the corrector (R/RNABloom.java:1980-2015 single-end worker, :2097-2170 FragmentAssembler,
 * :3788-3800 long reads).  The counts are rb_graph_batch_counts' (0 for a window with an unusable base; create the batch without a
 * quality threshold).  A segment is a range of consecutive windows of one read; with covs its n counts sorted ascending:
 *   n_solid          windows with count >= min_kmer_cov                                  (R/util/GraphUtils.java:3099-3108)
 *   min q1 median q3 max, dropoff   getCoverageStats(..., calcDropOff = true)            (GraphUtils.java:1799-1845)
 *   se_threshold, RB_COV_SE_FOUND   the threshold search of correctErrorsSE: nFP = Math.round(n * cov_fpr), start n-1-nFP, strict
 *                    `>`; not found: covs[0], or 0 when start < 0                       (GraphUtils.java:4007-4034)
 *   pe_threshold, RB_COV_PE_FOUND   mates only: first-round threshold search of correctErrorsPE for this mate, nFP from
 *                    max(n, n of the other mate), `>=`; not found: covs[0].  The caller combines the two mates as :4126-4142 do
 *   n_complex        reads mode only: usable windows whose k bases are not SeqUtils.isRepeat (SeqUtils.java:458-497, U as T)
 * An empty segment (n = 0) has every float 0, no flag and n_complex 0.  Arithmetic is the Java float32 arithmetic, ties included.
 * Segmentations: RB_COV_READS, one segment per read (seg_offsets[i] = i); RB_COV_WINDOWS, the first pass of
 * correctLongSequenceWindowed (GraphUtils.java:3110-3140): i = 0; end = min(i + window, n); if end + window/2 >= n then end = n;
 * next i = end.  A window's threshold there is `dropoff > 0 ? max(dropoff, min_kmer_cov) : median`, used only when the window has at
 * least `lookahead` k-mers.  seg_offsets (host, n + 1 entries, required for windows): the records of read first + i are
 * [seg_offsets[i], seg_offsets[i+1]).  out == NULL: only seg_offsets is filled (a size query).  mates != NULL (reads mode only):
 * read mate_first + i of `mates` is read first + i's mate, its record is out[n + i].  out_on_device != 0: `out` is device memory of
 * the graph's device.  The call works in pieces of bounded device scratch; a host `out` is pinned for the call and each piece's
 * copy overlaps the next piece's kernels.  Refused like rb_graph_batch_counts: shard handles, batches on another device, a
 * destroyed counting filter, ranges outside a batch, parameters out of range. */
enum { RB_COV_READS = 0, RB_COV_WINDOWS = 1 };
#define RB_COV_SE_FOUND 1u
#define RB_COV_PE_FOUND 2u
typedef struct rb_cov_params {          /* the reference's worker fields */
    int32_t segments;                   /* RB_COV_READS | RB_COV_WINDOWS */
    int32_t window;                     /* windowSize (RB_COV_WINDOWS), >= 1 */
    int32_t lookahead;                  /* >= 1 */
    float max_cov_gradient, cov_fpr, min_kmer_cov;   /* finite; max_cov_gradient >= 0, 0 <= cov_fpr <= 1 */
} rb_cov_params;
typedef struct rb_cov_stats {           /* 48 bytes, one per segment */
    int32_t n, n_solid, n_complex;
    uint32_t flags;                     /* RB_COV_SE_FOUND | RB_COV_PE_FOUND */
    float min, q1, median, q3, max, dropoff, se_threshold, pe_threshold;
} rb_cov_stats;
int rb_graph_read_coverage(rb_graph *g, const rb_batch *b, int64_t first, int64_t n, const rb_batch *mates, int64_t mate_first,
                           const rb_cov_params *p, int64_t *seg_offsets, rb_cov_stats *out, int out_on_device);

/* Paired-k-mer segmentation of host sequences — GraphUtils.breakWithReadPairedKmers (R/util/GraphUtils.java:4184-4310, the range form and
 * the whole-list form) and breakWithFragPairedKmers (:4312-4405, with and without numPairsRequired), which FragmentAssembler runs on every
 * connected fragment (R/RNABloom.java:2185-2200, 2215-2232) and transcript assembly on every fragment (:1855-1890).
 *   Input: sequence i is seq[offsets[i], offsets[i+1]); its k-mer list is getKmers' (every window, nk = max(0, len - k + 1); a letter
 *   outside ACGTU hashes as seed 0 forward and with the `ch & 7` seed on the reverse strand, as rb_graph_kmers).
 *   Pair key of position p (d = the graph's read- or fragment-paired k-mer distance): Kmer.getKmerPairHashValue (R/graph/Kmer.java:65-67,
 *   CanonicalKmer.java:61-72): stranded combine(f[p], f[p+d]), canonical the signed min(combine(f[p], f[p+d]), combine(r[p+d], r[p]));
 *   support[p] = the pair filter's lookup of that key (lookupReadKmerPair / lookupFragmentKmerPair, BloomFilterDeBruijnGraph.java:526-532).
 *   Segments: the reference's loop with interlockDistance = 0 over p in [rangeStart, lastIndex], lastIndex = rangeEnd - 1 - d.  A run of
 *   num_pairs_required consecutive supported positions ending at p opens a segment at p - num_pairs_required + 1 (if none is open), and
 *   every such p sets end = p + d; any unsupported p resets the run and closes the open segment only when p >= end.  A segment still open
 *   after the loop is emitted too.  Segments are [start, end + 1) in k-mer indices, in the reference's order.  num_pairs_required = 1 is
 *   the reference's first branch; breakWithFragPairedKmers(kmers, graph) is num_pairs_required = 1 on RB_FPKBF.
 *   ranges: NULL = [0, nk) for every sequence (the whole-list forms), else 2n ints [rangeStart, rangeEnd), 0 <= start <= end <= nk.
 *   seg_offsets (host, n + 1): capacity layout from the lengths alone.  Consecutive segment starts are at least d + 1 apart, so sequence i
 *   gets max(0, floor((rangeEnd - 1 - d - rangeStart) / (d + 1)) + 1) slots of 2 ints at segs + 2 * seg_offsets[i]; n_segs[i] = how many
 *   it filled.  koffsets (host, n + 1, optional): getKmers' k-mer offsets.  support (optional, requires koffsets): one byte per k-mer of
 *   sequence i at support[koffsets[i] + p], 1 where position p is supported, 0 where it is not or p + d >= nk (rows of the whole list,
 *   whatever the range).  segs == NULL: only seg_offsets (and koffsets) are filled and nothing is launched (a size query).
 * The call works in pieces of bounded device scratch (RB_QUERY_PIECE k-mers, as rb_graph_kmers); results do not depend on the cuts.  Without
 * `support`, pair positions outside every range are not probed (64 at a time).  With rb_graph_profile_enable on, the kernels' device time
 * is added to the profile entry "pair_segments".  RB_ERR_STATE: a sequence produced more segments than its slots (an internal error; the
 * bound above makes it impossible).
 * Refused (RB_ERR_INVALID, nothing launched): a shard handle; `which` not RB_RPKBF / RB_FPKBF, or a pair filter the graph does not have
 * (useReadPairedKmers off; rb_graph_init_fragment_pairs never called); a distance < 1; num_pairs_required < 1; a range outside [0, nk] or
 * with start > end; null arrays. */
int rb_graph_paired_kmer_segments(rb_graph *g, int which, const char *seq, const int64_t *offsets, int64_t n, int num_pairs_required,
                                  const int32_t *ranges, int64_t *seg_offsets, int32_t *segs, int32_t *n_segs, uint8_t *support,
                                  int64_t *koffsets);
/* Mismatch correction of host sequences — GraphUtils.correctMismatches (R/util/GraphUtils.java:3914-3996, the last step of
 * correctErrorHelper :3904): a low-coverage k-mer between two solid ones is replaced by the substitution whose k windows have the best
 * median coverage.  The two scans run on the device, a wavefront per sequence; the host gets the corrected text back.
 *   Input: sequence i is seq[offsets[i], offsets[i+1]) with threshold T = cov_threshold[i] (the reference's covThreshold: e.g.
 *   rb_cov_stats.se_threshold) and one min_kmer_cov.  Its k-mer list is getKmers(String)'s, as rb_graph_kmers gives it: every window,
 *   nk = max(0, len - k + 1), count 0 for a window with a letter outside ACGTU.  c[p] = count of window p, s = the sequence's bytes.
 *   Forward scan, i = 1 .. nk - k - 1 ascending.  Candidate: c[i] < T, c[i-1] >= T, c[i+k] >= T.  best = median of c[i .. i+k-2] — k - 1
 *   counts, the reference's getMedianKmerCoverage(kmers, i, i+k-1); the median of an even number of counts is (a + b) / 2.0f.  For each
 *   alternative of base s[i+k-1] in the order of SeqUtils.getAltNucleotides (the other three of A C G T; U as T; any other letter, lower
 *   case included: all four) whose variant k-mer is in dbgbf (getRightVariants(String): graph.contains, not getCount): the k windows of
 *   s[i .. i+2k-2] with that base substituted, counted as getKmers counts them; the variant wins if their minimum >= min_kmer_cov and
 *   their median > best (strictly: the first of equal medians stays), and best becomes that median.  A winner replaces s[i+k-1] and
 *   c[i .. i+k-1]; the scan goes on at i + 1 on the changed profile.
 *   Reverse scan over the result, i = nk - 2 .. k descending: c[i] < T, c[i+1] >= T, c[i-k] >= T; best = median of c[i-k+1 .. i-1];
 *   alternatives of s[i] (getLeftVariants(String)); windows i-k+1 .. i; the same acceptance; s[i] and c[i-k+1 .. i] replaced.
 *   Output: out_seq[offsets[i], offsets[i+1]) = the corrected sequence (the layout of seq; out_seq may be seq), n_fixed[i] = the number
 *   of replacements (the reference's `corrected` is n_fixed[i] > 0).  koffsets (host, n + 1, optional): getKmers' k-mer offsets; counts
 *   (optional, requires koffsets): the final c of sequence i at counts[koffsets[i] + p] — rb_graph_kmers' counts of out_seq.
 *   Sequences with nk <= k + 1 or T <= 0 come back unchanged.
 * The call works in pieces of bounded device scratch (RB_QUERY_PIECE k-mers, as rb_graph_kmers); results do not depend on the cuts.  It
 * leases a query context like the other lookups (re-entrant on one handle).  With rb_graph_profile_enable on, the kernels' device time is
 * added to the profile entry "mismatches".
 * Refused (RB_ERR_INVALID, nothing launched): a null handle or a null offsets / cov_threshold / out_seq / n_fixed (or seq, where there is
 * text); a shard handle; a destroyed dbgbf or counting filter; a threshold or min_kmer_cov that is not finite; decreasing offsets; counts
 * without koffsets; k < 2 (the reference's median of k - 1 counts does not exist). */
int rb_graph_correct_mismatches(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, const float *cov_threshold, float min_kmer_cov,
                                char *out_seq, int32_t *n_fixed, int64_t *koffsets, float *counts);
/* Error correction of host sequences — GraphUtils.correctErrorHelper (R/util/GraphUtils.java:3711-3912), what correctErrorsSE (:3998-4049) and
 * correctErrorsPE (:4051-4182) run on every read that passed the coverage screen: every run of k-mers below the threshold (a gap) is repaired,
 * then correctMismatches (:3904) runs on the repaired list.  All of it happens on the device; gaps do not depend on each other (after a gap the
 * reference appends the ORIGINAL good k-mer behind it, :3850, which is the next gap's left anchor, :3820), so all gaps of a call are resolved at once.
 *   Input: sequence i is seq[offsets[i], offsets[i+1]) with T = cov_threshold[i]; its k-mer list is getKmers(String)'s, as rb_graph_kmers gives it
 *   (nk = max(0, len - k + 1); count 0 for a window with a letter outside ACGTU).
 *   Gap scan (:3730-3855): a k-mer is bad if count < T.  A run of nb bad k-mers [g, g + nb) that ends at a good k-mer is a gap; a run still open at
 *   the end is the right edge (:3857-3902) if nb < nk.  A sequence that is bad throughout, has no k-mer, or has T <= 0 has no gap.
 *   Left edge (g = 0, :3736-3781): Kmer.getLeftVariants(k, numHash, graph, min_kmer_cov) (R/graph/Kmer.java:361, CanonicalKmer.java:387) of the LAST
 *   bad k-mer.  None -> kept.  Else nb < lookahead -> trimmed.  Else tipMed = Common.getMedian of the tip's counts (float32; an even number gives
 *   (a + b) / 2f) and ext = greedyExtendLeft(graph, kmers[nb], lookahead, nb) (:1906-1921): if ext has nb k-mers and its median count > tipMed then
 *   getPercentIdentity(assemble(ext), assemble(tip)) >= percent_identity -> replaced by ext; else !kmers[0].hasPredecessors && nb < k -> trimmed (a
 *   blunt end); else kept.  Otherwise kept.  Right edge: the mirror image — getRightVariants of the FIRST bad k-mer, greedyExtendRight from the good
 *   k-mer before it, hasSuccessors of the last k-mer.
 *   getPercentIdentity (R/util/SeqUtils.java:164-175) is (max(|a|, |b|) - d) / max(|a|, |b|) in float32 with d = getDistance (:190-229): the
 *   Levenshtein rows, except that the reference's row copy leaves out the last column, so d = min(D[|a|][|b|-1] + 1, |b| + 1,
 *   D[|a|-1][|b|-1] + (a's last letter != b's last letter)) for the true matrix D — reproduced.  No length limit.
 *   SNV bubble (nb == k, :3782-3818): for n in A C G T the counts of getKmers(kmers[g] + n + kmers[g+k-1]) — 2k + 1 letters, k + 2 windows.  A
 *   candidate wins if its minimum >= min_kmer_cov and its median > best; best starts at Float.MIN_VALUE (the smallest positive float); the winner
 *   needs best >= min_kmer_cov, and its k + 2 k-mers stand for the k bad ones: the sequence grows by two letters (reproduced, not fixed).
 *   Path (every other interior gap, :3819-3845): getMaxCoveragePath(graph, kmers[g-1], kmers[g+nb], nb + max_indel_size, lookahead, min_kmer_cov)
 *   (:1591-1675, with the meeting rule and SeqUtils.isLowComplexityShort :499-543).  A path of len k-mers is accepted if nb - max_indel_size <= len
 *   <= nb + max_indel_size and (len <= k + max_indel_size or getPercentIdentity(assemble(path), assemble(kmers, g, g + nb)) >= percent_identity).
 *   Then correctMismatches(kmers2, graph, T, min_kmer_cov) as rb_graph_correct_mismatches runs it, on the string kmers2 spells.
 *   Letters outside ACGTU follow the existing primitives: such windows count 0; variants and neighbours are hashed as rb_graph_neighbors hashes
 *   them (directions 2 / 3 and 0 / 1, SeqUtils.getAltNucleotides(byte) :130-145 choosing the alternatives); a walk from a seed with such a letter
 *   ends with reason 4 (no path, the gap is kept) — the seeds here are good k-mers, which have none.  k-mers compare as the walk kernels compare
 *   them (upper / lower case alike, U as T), and letters taken from a walk's k-mers come out as upper-case A C G T.
 *   Output: out_offsets (host, n + 1) is a capacity layout from the lengths and max_indel_size alone: cap_i = len_i + floor((nk_i - 1) / 2) *
 *   max_indel_size + 2 * floor((nk_i - 1) / (k + 1)) for nk_i >= 1, else len_i.  (An edge gap never grows.  Every interior gap has a good k-mer
 *   before the first and behind each: p path gaps and s SNV gaps need 1 + 2p + (k + 1)s <= nk k-mers, a path gap grows by at most
 *   max_indel_size, :3830-3832, an SNV gap by exactly 2; p <= (nk-1)/2 and s <= (nk-1)/(k+1) separately.)  out_seq[out_offsets[i] ..] holds the
 *   string the reference's kmers2 spells after correctMismatches, out_len[i] its length.  flags[i]: RB_CORR_GAP a gap was replaced or trimmed,
 *   RB_CORR_MISMATCH the mismatch pass replaced a base, RB_CORR_CORRECTED either (the reference returns non-null); with no bit set the sequence
 *   comes back as it went in.  out_seq == NULL: a size query — out_offsets (and gap_offsets, if given: the capacity layout (nk_i + 1) / 2 per
 *   sequence, whose last entry bounds the number of records) are filled and nothing is launched.
 *   gaps (optional, requires gap_offsets): one record per gap, densely: those of sequence i are gaps[gap_offsets[i] .. gap_offsets[i+1]) in scan
 *   order; `gaps` needs room for the size query's gap_offsets[n] records.  repl_len: the k-mers that stand for the run (kept: run, trimmed: 0).
 * The call works in pieces (RB_QUERY_PIECE input k-mers, as rb_graph_kmers; by default 16 M / (1 + (max_indel_size + 1) / 2), so that a piece has
 * about 16 M CAPACITY k-mers); results do not depend on the cuts.  Device scratch of a piece: 40 bytes per capacity k-mer (cap_i - k + 1 per
 * sequence: two hashes, count, code row, text and bits of the stitched text) + 5 bytes per input letter + 60 bytes per gap + at most 256 MB for
 * the walks that run together (one walk alone may need more: 42 bytes per step of its bound) — bounded by the piece and one sequence, not
 * by the call.  It leases a query context (re-entrant on one handle).  With rb_graph_profile_enable on, the profile entry "correct_errors"
 * gets the time from the first to the last kernel of each piece — the host's work at the piece's two intermediate synchronisations (prefix
 * sums of the gap counts, sorting the gap records into lists) included, so it is an interval on the stream, not pure device time; the
 * kernels alone are in the per-phase entries "correct_errors.profile" / ".scan" / ".walks" / ".resolve" / ".stitch" / ".mismatch".
 * RB_ERR_STATE: a sequence outgrew its slot (an internal error; nothing is truncated silently).
 * Refused (RB_ERR_INVALID, nothing launched): null handle / offsets / cov_threshold / p / out_offsets, out_seq without out_len or flags, seq
 * where there is text; a shard handle; a destroyed dbgbf or counting filter; a threshold, percent_identity or min_kmer_cov that is not finite;
 * lookahead outside 1..16 (the greedy kernel's limit); max_indel_size outside 0..4096; decreasing offsets; gaps without gap_offsets; k < 2. */
enum { RB_GAP_LEFT_EDGE = 0, RB_GAP_RIGHT_EDGE = 1, RB_GAP_SNV = 2, RB_GAP_PATH = 3 };      /* rb_corr_gap.kind */
enum { RB_GAP_KEPT = 0, RB_GAP_REPLACED = 1, RB_GAP_TRIMMED = 2 };                          /* rb_corr_gap.outcome */
#define RB_CORR_CORRECTED 1u
#define RB_CORR_GAP 2u
#define RB_CORR_MISMATCH 4u
typedef struct rb_corr_params { int32_t lookahead, max_indel_size; float percent_identity, min_kmer_cov; } rb_corr_params;
typedef struct rb_corr_gap {            /* 20 bytes */
    int32_t seq, first, run;            /* sequence, first bad k-mer, number of bad k-mers */
    int32_t repl_len;
    uint8_t kind, outcome, pad[2];
} rb_corr_gap;
int rb_graph_correct_errors(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, const float *cov_threshold, const rb_corr_params *p,
                            int64_t *out_offsets, char *out_seq, int32_t *out_len, uint32_t *flags, rb_corr_gap *gaps, int64_t *gap_offsets);
/* Error correction of read pairs, every round inside the call — GraphUtils.correctErrorsPE (R/util/GraphUtils.java:4051-4182), which the
 * FragmentAssembler runs on every pair between connect and overlapAndConnect (R/RNABloom.java:2086-2235), and, with rseq == NULL,
 * GraphUtils.correctErrorsSE (:3998-4049), the single-end worker's (R/RNABloom.java:1980-2001).  Read-only on the graph.  Texts, hash rows and
 * counts stay on the device between rounds; the input goes up once and the final texts come back once.
 *   Pair i is left = lseq[loffsets[i], loffsets[i+1]) and right = rseq[roffsets[i], roffsets[i+1]).  The count profile of a mate is getKmers' of its
 *   current text, as in rb_graph_correct_errors: every window, count 0 where a letter is outside ACGTU.
 *   A round of the pair form (the loop :4066-4179): nFP = (int) Math.round(max(nL, nR) * cov_fpr) from the CURRENT lists (:4071); per mate the
 *   sorted counts are walked down from startIndex = n - 1, lowered by nFP only if startIndex > nFP (:4084-4087): the threshold is covs[startIndex],
 *   then covs[i] for i = startIndex - 1 .. 0 until threshold * max_cov_gradient >= covs[i] (found; float32, one operation) (:4088-4097, :4118-4126).
 *   The pair's threshold (:4129-4143): both found -> the smaller; one found -> that one if it is <= the other mate's (which is its covs[0]); else -1.
 *   If threshold >= min_cov_threshold (:4145), correctErrorHelper runs on both mates with it — exactly what rb_graph_correct_errors computes, its
 *   flag RB_CORR_CORRECTED being the reference's "non-null" — and a non-null result replaces the mate (:4155-4172).  Both null ends the loop (:4174).
 *   A round whose threshold is below min_cov_threshold changes nothing, and the reference repeats it unchanged until the rounds run out: the call
 *   stops the pair there (RB_PAIRC_END_LOW) with the same result.
 *   Single form (rseq, roffsets, rout_offsets, rout all NULL): correctErrorsSE runs once if iterations > 0.  The search is rb_cov_stats.se_threshold's:
 *   startIndex = n - 1 - nFP with nFP = (int) Math.round(n * cov_fpr), strict `>`, not found when startIndex < 0 (:4019-4035); min_cov_threshold
 *   is not read.  The right-hand fields of the record stay 0.
 *   recs[i]: status — RB_PAIRC_CORRECTED exactly when ReadPair.corrected is true (:4181; single form: the helper returned non-null),
 *   RB_PAIRC_UNCHANGED, or RB_PAIRC_NOT_JUDGED; end — why the rounds ended: RB_PAIRC_END_ALL the round count ran out (iterations == 0 included),
 *   END_NO_CHANGE both results null (:4174), END_LOW the threshold was below min_cov_threshold (single form: not found, the reference returns null),
 *   END_NO_KMER, END_LOST_KMERS (below); rounds_run: the rounds in which the helper ran; flags: RB_PAIRC_LEFT / RIGHT leftCorrected /
 *   rightCorrected, and the overflow bits; left_len, right_len: the lengths of the final texts; thr_first / thr_last: the bits of the pair's
 *   threshold of round 0 and of the last round entered, -1.0f where there was none (:4129; single form: not found; no round entered);
 *   found_first: round 0, bit 0 the left threshold was found, bit 1 the right; left_changed / right_changed: the rounds in which the helper
 *   returned non-null for that mate; gaps_replaced / gaps_trimmed / gaps_kept (rb_corr_gap.outcome) and mismatches (replacements of the mismatch
 *   pass), summed over rounds and mates.
 *   Not judged, never guessed: a pair one of whose mates has no k-mer at entry is RB_PAIRC_NOT_JUDGED / END_NO_KMER (the reference throws at :4088);
 *   in the single form an empty list is RB_PAIRC_UNCHANGED / END_NO_KMER (the reference returns null, :4007).  A mate that leaves a round with no
 *   k-mer is NOT_JUDGED / END_LOST_KMERS (the next round would throw).  The texts of a not-judged pair come back as they went in.
 *   iterations == 0: nothing runs; every record is RB_PAIRC_UNCHANGED / END_ALL.
 *   Output: lout_offsets / rout_offsets (n + 1 each) are INPUTS, the caller's capacity layouts, as in rb_graph_correct_long.  A final text is written
 *   at its offset if it fits; else the mate's overflow bit is set and nothing is written for it.  left_len / right_len are the lengths needed either
 *   way; the computation is deterministic, so a second call with room gives the text.  Nothing is ever truncated.
 * The call works in pieces (RB_QUERY_PIECE input k-mers of both mates, by default as rb_graph_correct_errors); a pair is never split and results
 * do not depend on the cuts.  Device scratch of a piece: 21 bytes per input k-mer + 1.2 per letter for the first profile; then per round, for the
 * mates still live, 21 bytes per k-mer + 1 per letter of the round's input and rb_graph_correct_errors' scratch for them (40 bytes per capacity
 * k-mer, 60 per gap, the walks' 256 MB), the capacity being taken from the mates' actual lengths every round; 64 bytes a pair; the finished
 * texts of a round; a gather table of 56 bytes per mate of the round.  Between rounds the host sees 4 bytes a live mate and pair (lengths, live
 * flags) and the gap records, as the corrector does; from them it builds the compaction's gather table (source and destination offsets, 7 int64
 * a mate) and uploads it: the rows are moved on the device, their destinations are computed on the host.  A round costs three stream
 * synchronisations (live flags; the finished texts, where there are any; lengths) besides the corrector's own two, and the call's buffers grow
 * by free and allocate, each a device-wide wait.  None of it is tuned.
 * It leases a query context (re-entrant on one handle).  Profile entry "correct_pairs": the interval from a piece's first to its last kernel,
 * the host's work between the rounds included.  RB_ERR_STATE: a sequence outgrew its slot (an internal error).
 * Refused (RB_ERR_INVALID, nothing launched): a null handle / loffsets / p / lout_offsets, null recs / lout (n > 0), roffsets without rout_offsets
 * or rout, rseq / rout_offsets / rout without roffsets, text missing where there is text; a shard handle; a destroyed dbgbf or counting filter;
 * k < 2; a float parameter that is not finite; max_cov_gradient < 0; cov_fpr outside [0, 1]; lookahead outside 1..16; max_indel_size outside
 * 0..4096; iterations < 0; decreasing offsets (input or capacity).  n == 0 succeeds and touches nothing. */
typedef struct rb_pairc_params {
    int32_t iterations, lookahead, max_indel_size;      /* errorCorrectionIterations >= 0; lookahead / max_indel_size as rb_corr_params */
    float max_cov_gradient, cov_fpr, min_cov_threshold, percent_identity, min_kmer_cov;
} rb_pairc_params;
enum { RB_PAIRC_UNCHANGED = 0, RB_PAIRC_CORRECTED = 1, RB_PAIRC_NOT_JUDGED = 2 };                   /* status */
enum { RB_PAIRC_END_ALL = 0, RB_PAIRC_END_NO_CHANGE = 1, RB_PAIRC_END_LOW = 2,
       RB_PAIRC_END_NO_KMER = 3, RB_PAIRC_END_LOST_KMERS = 4 };                                     /* end */
#define RB_PAIRC_LEFT 1u        /* flags: leftCorrected */
#define RB_PAIRC_RIGHT 2u       /* rightCorrected */
#define RB_PAIRC_LEFT_OVERFLOW 4u
#define RB_PAIRC_RIGHT_OVERFLOW 8u
typedef struct rb_pairc_rec {   /* 64 bytes */
    int32_t status, end, rounds_run, flags, left_len, right_len;
    uint32_t thr_first, thr_last;          /* float bits: the pair's threshold of round 0 and of the last round entered (-1.0f: none) */
    int32_t found_first;                   /* round 0: bit 0 left threshold found, bit 1 right */
    int32_t left_changed, right_changed;   /* rounds in which correctErrorHelper returned non-null for that mate */
    int32_t gaps_replaced, gaps_trimmed, gaps_kept, mismatches;   /* summed over rounds and mates */
    int32_t reserved;                      /* 0 */
} rb_pairc_rec;
int rb_graph_correct_pairs(rb_graph *g, const char *lseq, const int64_t *loffsets, const char *rseq, const int64_t *roffsets, int64_t n,
                           const rb_pairc_params *p, const int64_t *lout_offsets, char *lout, const int64_t *rout_offsets, char *rout,
                           rb_pairc_rec *recs);
/* Overlap of read pairs — GraphUtils.overlap (R/util/GraphUtils.java:4898-5063), the first half of overlapAndConnect (:5065-5090) that the
 * FragmentAssembler runs on every corrected pair (R/RNABloom.java:2148), over SeqUtils.overlapMaximally (R/util/SeqUtils.java:1335-1379).  A wavefront
 * per pair on the device; the call is read-only.  Pair i is left = lseq[loffsets[i], loffsets[i+1]) and right = rseq[roffsets[i], roffsets[i+1]); each
 * read's k-mer list is getKmers(String)'s, as rb_graph_kmers gives it (every window; count 0 for a window with a letter outside ACGTU).
 *   match(a, b, mo): the smallest shift s in [0, |a| - mo] at which b agrees with a over the whole extent they share, a[s, min(s + |b|, |a|)) ==
 *   b[0, ...), bytes compared exactly (case matters) — the first hit of the reference's indexOf(prefix) loop.  s + |b| < |a|: overlapped = a (b is
 *   contained); else overlapped = a + b[|a| - s ..].  No such s, |a| < |b| and b contains a: overlapped = b.
 *   1. match(left, right, min_overlap).  None: mo' = max(min_overlap, min(|left|, |right|) * 3 / 4) (int arithmetic) and match(right, left, mo'); a
 *      hit swaps the roles (dovetail, RB_OVL_SWAPPED: left / right below, LEFT / RIGHT and the text are in swapped terms).  None: NONE, WHY_NO_MATCH.
 *   2. o = |left| + |right| - |overlapped| bases overlap.  o >= k: |overlapped| == max(|left|, |right|) -> LEFT if |left| >= |right| else RIGHT
 *      (the longer read's k-mers are returned).  Else at least one of right's k-mers 0 .. o - k must not be a homopolymer (all k bytes equal), else
 *      NONE, WHY_NO_COMPLEX; the result is left's k-mers and right's from o - k + 1: MERGED.  No graph look-up.
 *   3. o < k: the spanning k-mers are the windows span_first = |left| - k + 1 .. span_first + span_n - 1 of overlapped, span_n = k - 1 - o
 *      (graph.getKmers(overlapped, start, end): [start, end) is a range of bases).  In order: the first with count < min_kmer_cov makes the span
 *      invalid and ends the walk; a k-mer seen before that which is no homopolymer makes the span complex.  Valid: an empty or a complex span gives
 *      SPANNED (left + spanning + right), else NONE, WHY_NO_COMPLEX.  Invalid: the reference rescues the pair (:5018-5056: addDbgOnly of the
 *      spanning k-mers of count 0, correctMismatches with threshold 2, addReadPairedKmers) if some right k-mer i < min(o, nkR) has count == 1
 *      (else WHY_NO_RIGHT_SINGLETON), some left k-mer i >= max(0, nkL - o) has count == 1 (else WHY_NO_LEFT_SINGLETON) and
 *      !SeqUtils.isRepeat(right[0, o)) (:417-456; else WHY_REPEAT), tested in that order: RESCUE.  The call changes nothing: a RESCUE record
 *      describes the pair BEFORE the mutation (the text is overlapped before correctMismatches) and the caller applies those lines.  After them the
 *      reference's no-complex-k-mer test cannot fail: a span of homopolymers forces right[0, o) to be one letter, for which isRepeat is true.
 *      isRepeat(String) indexes its count arrays with -1 at a letter outside ACGTU (upper case only) and throws unless a threshold was reached
 *      before that letter: WHY_REPEAT_THROWS (NONE; the reference's worker dies there).
 *   A pair with a read shorter than max(k, min_overlap) gets NONE, WHY_SHORT (the reference throws in substring, or is never called).
 *   Output: out_offsets (host, n + 1) is the capacity layout |left_i| + |right_i|, from the lengths alone.  out_seq == NULL: a size query — only
 *   out_offsets is filled, nothing is launched.  out_seq[out_offsets[i] ..] holds the string the returned k-mer list spells and recs[i].out_len its
 *   length: the containing read's text (LEFT / RIGHT), overlapped (MERGED / SPANNED / RESCUE), nothing (NONE: out_len 0).  recs[i].overlap = o
 *   and the SWAPPED flag are set whenever a match was found (NONE with another reason than NO_MATCH / SHORT included), span_first / span_n for
 *   SPANNED and RESCUE, else 0.  A NONE is the caller's cue for GraphUtils.join; `why` says which line returned null.
 * Every pair is judged against the graph as it stands when the call starts: a rescue is not applied before the next pair is looked at.  The
 * reference's `-t N` workers give no order between pairs either.
 * The call works in pieces cut by the input letters of both reads (RB_QUERY_PIECE letters, 64 M by default; 2 bytes of device scratch per letter and
 * 48 per pair); results do not depend on the cuts.  It leases a query context (re-entrant on one handle).  With rb_graph_profile_enable on the
 * kernels' device time is added to the profile entry "overlap".
 * Refused (RB_ERR_INVALID, nothing launched): a null handle, loffsets, roffsets, out_offsets (or recs, unless out_seq is NULL too); text missing where
 * offsets say there is some; decreasing offsets; a shard handle; a destroyed dbgbf or counting filter; min_overlap < 1; a min_kmer_cov that is
 * not finite. */
enum { RB_OVL_NONE = 0, RB_OVL_LEFT = 1, RB_OVL_RIGHT = 2, RB_OVL_MERGED = 3, RB_OVL_SPANNED = 4, RB_OVL_RESCUE = 5 };      /* rb_overlap_rec.outcome */
enum { RB_OVL_WHY_FOUND = 0, RB_OVL_WHY_NO_MATCH = 1, RB_OVL_WHY_NO_COMPLEX = 2, RB_OVL_WHY_NO_RIGHT_SINGLETON = 3, RB_OVL_WHY_NO_LEFT_SINGLETON = 4,
       RB_OVL_WHY_REPEAT = 5, RB_OVL_WHY_SHORT = 6, RB_OVL_WHY_REPEAT_THROWS = 7 };                                           /* rb_overlap_rec.why */
#define RB_OVL_SWAPPED 1u
typedef struct rb_overlap_rec {         /* 32 bytes */
    int32_t outcome, why;
    uint32_t flags;
    int32_t overlap, out_len, span_first, span_n, pad;
} rb_overlap_rec;
int rb_graph_overlap_pairs(rb_graph *g, const char *lseq, const int64_t *loffsets, const char *rseq, const int64_t *roffsets, int64_t n,
                           int min_overlap, float min_kmer_cov, int64_t *out_offsets, char *out_seq, rb_overlap_rec *recs);
/* Paired-k-mer branch extension of host sequences — GraphUtils.extendRightSE / extendLeftSE (R/util/GraphUtils.java:6018-6204), the step the
 * transcript assembler's extendSE loop (:6454-6565, R/RNABloom.java:1850) and join (:978, :1106) take across a branch.  A wavefront per sequence
 * on the device; the call is read-only.  Sequence i is seq[offsets[i], offsets[i+1]) in its natural orientation with the floor min_kmer_cov[i];
 * its k-mer list is getKmers(String)'s (a letter outside ACGTU hashes as in rb_graph_kmers).  direction 0: extendRightSE over that list;
 * direction 1: extendLeftSE over the list reversed, as the reference's callers reverse it.  d = the read-paired k-mer distance, n = the
 * number of k-mers; only the last min(n, d) k-mers of the list are read.
 *   Candidates: the successors (direction 1: predecessors) of the last k-mer with graph.getCount >= 1 in the order A C G T (the two-argument
 *   getSuccessors, R/graph/Kmer.java:228-230: not the floor).  None: NONE, WHY_NO_CANDIDATE.  One: SINGLE — the candidate followed by
 *   naiveExtend{Right,Left}NoBackChecks(candidate, bound d - 2, floor) (:6888-6933, :7067-7112: rb_graph_naive_extend mode 2), unscored and
 *   untrimmed (:6030-6035).
 *   First level (:6043-6066): per candidate the same walk, then countKmerPairsSE / countKmerPairsReversedSE (:5718-5790) with gap 0: walked k-mer
 *   i (0 <= i <= min(d - 1, size - 1)) is looked up with the list's k-mer n - d + i where that index is not negative — lookupReadKmerPair of
 *   Kmer.getKmerPairHashValue, the list's k-mer on the left for direction 0 and on the right for direction 1 (rb_graph_paired_kmer_segments'
 *   key).  pairs = supported k-mers, last = the largest supported i.  A supported extension scores Math.min(pathMinCov, median) * pairs /
 *   (last + 1) in float32 (a product, then a quotient), pathMinCov = the minimum count of the last min(n, d) k-mers, median =
 *   getMedianKmerCoverage(Collection) of the whole extension (:229-247).  The best is kept on score > best || (score == best && median >
 *   bestMedian), from 0 / 0, trimmed to last + 1 k-mers.
 *   Second level (:6067-6106): an unsupported first stretch of gap k-mers, gap < d - 1, is extended by every successor (count >= 1) of its last
 *   k-mer and that k-mer's walk with bound d - gap; first stretch + extension is counted and scored the same way and competes for the same best.
 *   A walk's own stop (:6919): the only neighbour equals the k-mer the walk started from or the k-mer added last.  maxTipLength does not
 *   appear (see rb_graph_naive_extend).  A last k-mer with a letter outside ACGTU: NONE, WHY_INVALID_SEED, as the walks treat such a seed.
 *   Output: recs[i]; out_bases[i * (d + 2) ..] the out_len bases the returned k-mers add, in walking order as rb_graph_walk (direction 0: the
 *   last base of each k-mer, direction 1: the first), upper-case A C G T, zeros behind them; out_count (may be NULL) their graph.getCount.
 *   winner: the first-level candidate's base 0..3, for SECOND the second-level candidate's base in bits 4..5; -1 for NONE.  pairs,
 *   last_partnered, score: the winner's (0, -1, 0 for NONE and SINGLE).
 * The call works in pieces through the shared driver (RB_QUERY_PIECE k-mers of the sequences' last d + k - 1 letters); results do not depend
 * on the cuts.  Device scratch of a piece: 20 bytes per such k-mer, 36 + (d + 2) * 5 per sequence, and for d > 256 (the walks' rows do not fit
 * LDS) about 25 d bytes for each of at most 4096 wavefronts.  It leases a query context (re-entrant on one handle).  With rb_graph_profile_enable
 * on the kernels' device time is added to the profile entry "extend_se".
 * Refused (RB_ERR_INVALID, nothing launched): a null handle; a shard handle; a destroyed dbgbf, counting filter or read-pair filter (or a
 * graph made without one); d < 2; a direction other than 0 / 1; n < 0; with n > 0: a null offsets / min_kmer_cov / out_bases / recs, a null seq
 * where there is text, decreasing offsets, a floor that is not finite or is negative.  n == 0 succeeds and touches nothing. */
enum { RB_EXT_NONE = 0, RB_EXT_SINGLE = 1, RB_EXT_FIRST = 2, RB_EXT_SECOND = 3 };                                             /* rb_extend_rec.outcome */
enum { RB_EXT_WHY_FOUND = 0, RB_EXT_WHY_NO_CANDIDATE = 1, RB_EXT_WHY_NO_SUPPORT = 2, RB_EXT_WHY_INVALID_SEED = 3, RB_EXT_WHY_SHORT = 4 };  /* rb_extend_rec.why */
typedef struct rb_extend_rec {          /* 32 bytes */
    int32_t outcome, why;
    int32_t n_candidates, out_len /* k-mers */, pairs, last_partnered, winner;
    float score;
} rb_extend_rec;
int rb_graph_extend_se(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, int direction, const float *min_kmer_cov,
                       char *out_bases /* n * (d + 2) */, float *out_count /* n * (d + 2), may be NULL */, rb_extend_rec *recs);
/* Fragment-paired branch extension of host sequences — GraphUtils.extendRightPE / extendLeftPE (R/util/GraphUtils.java:6206-6414), the step of
 * the transcript assembler's extendPE loop (:6567-6678), which it runs instead of extendSE whenever fragment-paired k-mers exist
 * (R/RNABloom.java:1846-1851).  Arguments, orientation, candidates, walks, output layout, pieces and refusals are rb_graph_extend_se's; what
 * differs, with d_r the read-paired and d_f the fragment-paired k-mer distance (neither is assumed the larger):
 *   Only the last min(n, max(d_r, d_f)) k-mers of the list are read.  The walks' bound is M = d_f - 2.  With two or more candidates M is
 *   lowered by one for every trailing k-mer of the list that graph.isRepeatKmer accepts, from the last k-mer backwards up to the first that
 *   is not one (:6226-6233; SeqUtils.isRepeat(byte[]) :458-497 of the k-mer in its natural orientation, its counters signed bytes: the
 *   homopolymer threshold round(0.9 k) is never reached from k = 142 on).  Every bound <= 0 acts alike, so the scan ends when M reaches 0 and
 *   max_ext = max(M, 0) is reported.  A k-mer inside the scanned stretch with a letter outside ACGTU makes the reference throw (unless a base
 *   count reaches the threshold in front of that letter): NONE, WHY_REPEAT_THROWS.  Such a letter further back than the scan reaches — more
 *   than d_f - 2 k-mers from the end, or behind the first k-mer that is no repeat — is not seen, as in the reference for the second case.
 *   pathMinCov is the minimum count of the last min(n, d_f) k-mers.  countKmerPairsPE / countKmerPairsReversedPE (:5792-5888): walked k-mer i
 *   (0 <= i <= min(d_f - 1, size - 1)) is looked up with the list's k-mer n - d_r + i in the read-pair filter and with k-mer n - d_f + i in
 *   the fragment-pair filter, each where that index lies in [0, n); last_partnered is the largest i either filter supports.  An extension is
 *   scored only with read_pairs > 0 and frag_pairs > 0: Math.min(pathMinCov, median) * (read_pairs + frag_pairs) / (last + 1) in float32.
 *   Else a first stretch of gap k-mers is skipped if (gap >= d_r - 1 and read_pairs == 0) or (gap >= d_f - 1 and frag_pairs == 0), and
 *   otherwise goes to the second level with bound M - gap; the whole chain's pairs are counted, the first stretch's included.
 *   Lower-case letters are read as upper-case ones, as everywhere in this library (the reference's isRepeat would throw on them).
 * out_bases / out_count rows are d_f + 2 long.  Device scratch follows d_f as rb_graph_extend_se's follows d; the profile entry is "extend_pe".
 * Refused as rb_graph_extend_se, and also: no fragment-pair filter (rb_graph_init_fragment_pairs not called, or destroyed); d_f < 2. */
enum { RB_EXT_WHY_REPEAT_THROWS = 5 };                                                                                           /* rb_extend_pe_rec.why, after RB_EXT_WHY_* */
typedef struct rb_extend_pe_rec {       /* 40 bytes */
    int32_t outcome, why;
    int32_t n_candidates, out_len /* k-mers */, read_pairs, frag_pairs, last_partnered, winner;
    float score;
    int32_t max_ext;                    /* the bound the first-level walks ran with, max(M, 0): d_f - 2 where the repeat scan did not run (or threw) */
} rb_extend_pe_rec;
int rb_graph_extend_pe(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, int direction, const float *min_kmer_cov,
                       char *out_bases /* n * (frag_d + 2) */, float *out_count /* n * (frag_d + 2), may be NULL */, rb_extend_pe_rec *recs);
/* The extension loop of fragments — GraphUtils.extendSE (R/util/GraphUtils.java:6454-6565; which = RB_EXTL_SE) and extendPE (:6567-6678; RB_EXTL_PE),
 * the step of TranscriptAssemblyWorker.run that grows a fragment into a transcript (R/RNABloom.java:1846-1851) — for n host sequences in ONE call: a
 * wavefront per sequence keeps it on the device from its first round to its last.  The call is read-only.  Sequence i is seq[offsets[i],
 * offsets[i+1]), kmers = getKmers of it; D is the read-paired k-mer distance for SE and the fragment-paired one for PE; m = min_kmer_cov.
 *   The left side runs first, over the reversed list, with extendLeftSE / extendLeftPE; the right side after it with extendRightSE / PE.  An outer
 *   iteration (:6467-6512): thr = the minimum getCount of the list's last min(size, D) k-mers (an added k-mer carries the count its step returned).
 *   Inner loop: thr = max(m, thr * 0.1f) in float32, then a step with that floor — rb_graph_extend_se's / _pe's step exactly — until the step returns
 *   k-mers or thr == m.  Nothing returned: the side ends (END_NOTHING).  Else used = every returned k-mer is already a k-mer of the list
 *   (Kmer.equals: hashes are compared first, every hit is confirmed on the bases).  The reference's second loop (:6497-6504) re-tests members of the
 *   list against the set made of the list; it can never clear the flag and is not restated.  used and size < D: the side ends (END_USED_SHORT).  used
 *   and hasDuplicatedKmerPair(list, e.getLast(), D, size - 1 - D + |e|) (:6416-6452: lastIndexOf, indexOf and the scan between them, which together
 *   ask whether some list[i] == e.getLast(), i >= D, has list[i - D] == list[size - 1 - D + |e|]): the side ends (END_USED_PAIR).  Else the k-mers are
 *   appended to the list and count as its k-mers from then on.
 *   Letters: the device judges sequences of upper-case A C G T only — the reference compares k-mers as bytes and added letters are upper-case A C G
 *   T, so `acgt`, U and N would need the bytes kept beside the codes.  A sequence with fewer than k letters is NOT_JUDGED / WHY_NO_KMER, any other
 *   with another byte NOT_JUDGED / WHY_LETTER: it comes back as it went in (out_len its length, every other field 0) and the caller's host loop is
 *   its route.  With clean letters RB_EXT_WHY_REPEAT_THROWS and WHY_INVALID_SEED cannot occur in a step.
 *   Room: the reference's loop has no bound; `room` is the most letters (= k-mers) a call may add on EACH side of a sequence.  Only whole rounds are
 *   applied: a round whose k-mers do not fit in what is left of its side's room is dropped (before the used test), the side ends with END_ROOM and the
 *   status is RB_EXTL_ROOM; after a left END_ROOM the right side is not run (END_NOT_RUN).  Nothing is truncated or guessed: the list's k-mers are
 *   the set, thr is recomputed from the list at the top of every outer iteration, so the state after any whole round is a state of the reference's
 *   loop.  Resume with the returned text: phase[i] = 0 (or phase == NULL) runs both sides — after a left END_ROOM; phase[i] = 1 runs the right side
 *   only (left_end = END_NOT_RUN) — after a right END_ROOM.  Chained calls return what one call with ample room returns; left_ext / right_ext add up
 *   over the calls.  A step returns at most D k-mers and room >= D + 2, so every call makes progress.
 *   Output: out_offsets (host, n + 1) is the capacity layout len_i + 2 * room, filled from the lengths alone; out_seq == NULL is a size query: nothing
 *   else is touched, nothing is launched.  Else out_seq[out_offsets[i] ..] holds out_len letters — the original ones as they were, added ones
 *   upper-case A C G T — and zeros behind them.  recs[i]: left_ext / right_ext the k-mers (= letters) added on each side, left_end / right_end how each
 *   side ended, left_rounds / right_rounds the rounds applied, steps the steps taken, floor_drops the steps that returned nothing above the lowest
 *   floor, used_passed the rounds that were `used` and went on, left_floor / right_floor the floor of the LAST step taken on that side (a dropped
 *   round's included; 0 where no step was taken).
 * The call works in pieces cut by capacity k-mers, len_i + 2 * room - k + 1 (RB_QUERY_PIECE, 16 M by default); results do not depend on the cuts.
 * Device scratch of a piece: 20 bytes per capacity k-mer (both hashes, the count) and 2 per capacity letter (the code, the text out) — a sequence's
 * row for as long as the piece lasts —, 20 bytes per k-mer of the text that went in, 64 + 1 per sequence, and for each of at most 4096 wavefronts
 * about 100 + 5 D bytes of the step's own, plus for D > 256 (the walks' rows do not fit LDS) about 25 D.  It leases a query context (re-entrant on
 * one handle).  With rb_graph_profile_enable on the kernels' device time is added to the profile entry "extend_loop".  RB_ERR_STATE: a row was found
 * outgrown (an internal error; nothing is cut silently).
 * Refused (RB_ERR_INVALID, nothing launched): a null handle; a shard handle; a destroyed dbgbf, counting filter or read-pair filter (or a graph made
 * without one), for PE also the fragment-pair filter; a distance below 2; `which` other than 0 / 1; a min_kmer_cov that is not finite or is negative;
 * room < D + 2 or room > 2^24; n < 0; with n > 0: a null offsets / out_offsets (or recs, unless out_seq is NULL too), a null seq where there is text,
 * decreasing offsets, a phase byte above 1.  n == 0 succeeds and touches nothing. */
enum { RB_EXTL_SE = 0, RB_EXTL_PE = 1 };                                                                                         /* which */
enum { RB_EXTL_DONE = 0, RB_EXTL_ROOM = 1, RB_EXTL_NOT_JUDGED = 2 };                                                             /* rb_extend_loop_rec.status */
enum { RB_EXTL_WHY_NONE = 0, RB_EXTL_WHY_NO_KMER = 1, RB_EXTL_WHY_LETTER = 2 };                                                  /* rb_extend_loop_rec.why (NOT_JUDGED) */
enum { RB_EXTL_END_NOT_RUN = 0, RB_EXTL_END_NOTHING = 1, RB_EXTL_END_USED_SHORT = 2, RB_EXTL_END_USED_PAIR = 3, RB_EXTL_END_ROOM = 4 };   /* left_end, right_end */
typedef struct rb_extend_loop_rec {     /* 64 bytes */
    int32_t status, why;
    int32_t left_ext, right_ext, out_len /* letters */;
    int32_t left_end, right_end;
    int32_t left_rounds, right_rounds;
    int32_t steps, floor_drops, used_passed;
    float left_floor, right_floor;
    int32_t pad[2];
} rb_extend_loop_rec;
int rb_graph_extend_loop(rb_graph *g, int which, const char *seq, const int64_t *offsets, int64_t n, const uint8_t *phase /* may be NULL */,
                         float min_kmer_cov, int room, int64_t *out_offsets, char *out_seq, rb_extend_loop_rec *recs);
/* Naive extension of fragments — GraphUtils.naiveExtend(kmers, graph, maxTipLength, minKmerCov) (R/util/GraphUtils.java:6935-6957), which the
 * FragmentAssembler runs on every connected fragment when extendFragments is on (R/RNABloom.java:2214) — for n host sequences in ONE call: a
 * wavefront per sequence runs both walks on the device.  The call is read-only.  Sequence i is seq[offsets[i], offsets[i+1]), kmers = getKmers of
 * it; m = min_kmer_cov.  The conventions are rb_graph_extend_loop's wherever they apply.
 *   First naiveExtendLeft(kmers[0], terminators = the set of kmers) (:6959-7012), then naiveExtendRight(kmers[last], terminators = the set of
 *   kmers and the left extension) (:6780-6833).  A step, with `best` the k-mer the walk stands on — what rb_graph_naive_extend's mode 0 does, in
 *   this order: no neighbour with graph.getCount >= m ends the walk (END_NO_NEIGHBOUR) before the back-branch test; any variant of best in the base
 *   about to leave with count >= 1 ends it (END_BACK_BRANCH); two or more neighbours with count >= m end it (END_SEVERAL); the only candidate a
 *   member of the terminators or added before by this walk ends it, and the candidate is not added (END_MEMBER); else it is added and becomes
 *   best.  maxTipLength is no argument: it only feeds Kmer.hasDepthLeft / hasDepthRight, which never consult the graph (R/graph/Kmer.java:407-486;
 *   see rb_graph_naive_extend).  Membership is Kmer.equals, the k bases: hashes are compared first and every hit is confirmed on the bases.
 *   Letters: the device judges sequences of upper-case A C G T only.  A sequence with fewer than k letters is NOT_JUDGED / WHY_NO_KMER, any other
 *   with another byte NOT_JUDGED / WHY_LETTER: it comes back as it went in (out_len its length, both hits -1, every other field 0).
 *   Room: the reference's walks have no bound; `room` is the most letters (= k-mers) a call may add on EACH side of a sequence.  A walk that has
 *   added `room` k-mers and would add another ends with END_ROOM (after the membership test, so a walk that ends at exactly `room` k-mers for
 *   another reason says that reason) and the status is RB_NFRAG_ROOM; after a left END_ROOM the right side is not run (END_NOT_RUN).  Resume with
 *   the returned text: phase[i] = 0 (or phase == NULL) runs both sides, phase[i] = 1 the right side only (left_end = END_NOT_RUN).  Chained calls
 *   return what one call with ample room returns: the reference tests terminators.contains(best) || usedKmers.contains(best), and the k-mers of
 *   the returned text are exactly that union; a walk restarted from the text's outermost k-mer starts in the state the loop was in.  left_ext /
 *   right_ext add up over the calls.
 *   Output: out_offsets (host, n + 1) is the capacity layout len_i + 2 * room, filled from the lengths alone; out_seq == NULL is a size query: nothing
 *   else is touched, nothing is launched.  Else out_seq[out_offsets[i] ..] holds out_len letters — the original ones as they were, added ones
 *   upper-case A C G T — and zeros behind them.  recs[i]: left_ext / right_ext the k-mers (= letters) added on each side, left_end / right_end how
 *   each walk ended, left_hit / right_hit for END_MEMBER the lowest index in the k-mer list of the RETURNED text of a k-mer equal to the
 *   candidate that ended the walk (below left_ext: the left extension; from left_ext + the fragment's k-mers on: the right extension), else -1.
 *   The counts of the added k-mers are not returned (rb_graph_read_coverage of the text has them).
 * The call works in pieces cut by capacity k-mers, len_i + 2 * room - k + 1 (RB_QUERY_PIECE, 16 M by default); results do not depend on the cuts.
 * Device scratch of a piece: 2 bytes per capacity letter, 64 + 1 + 16 per sequence, and — only where a sequence's k-mers + 2 room exceed 1024, the
 * terminator table a wavefront keeps in LDS — 16 bytes times the next power of two of that number for each of at most 4096 wavefronts (fewer
 * where that would exceed 1 GB).  A sequence of more than 2^24 k-mers is refused.  It leases a query context (re-entrant on one handle).  With
 * rb_graph_profile_enable on the kernel's device time is added to the profile entry "naive_extend_fragments".
 * Refused (RB_ERR_INVALID, nothing launched): a null handle; a shard handle; a destroyed dbgbf or counting filter; a min_kmer_cov that is not finite
 * or is negative; room < 1 or room > 2^24; n < 0; with n > 0: a null offsets / out_offsets (or recs, unless out_seq is NULL too), a null seq where
 * there is text, decreasing offsets, a phase byte above 1.  n == 0 succeeds and touches nothing. */
enum { RB_NFRAG_DONE = 0, RB_NFRAG_ROOM = 1, RB_NFRAG_NOT_JUDGED = 2 };                                                          /* rb_naive_frag_rec.status */
enum { RB_NFRAG_WHY_NONE = 0, RB_NFRAG_WHY_NO_KMER = 1, RB_NFRAG_WHY_LETTER = 2 };                                               /* rb_naive_frag_rec.why (NOT_JUDGED) */
enum { RB_NFRAG_END_NOT_RUN = 0, RB_NFRAG_END_NO_NEIGHBOUR = 1, RB_NFRAG_END_BACK_BRANCH = 2, RB_NFRAG_END_SEVERAL = 3, RB_NFRAG_END_MEMBER = 4,
       RB_NFRAG_END_ROOM = 5 };                                                                                                  /* left_end, right_end */
typedef struct rb_naive_frag_rec {      /* 64 bytes */
    int32_t status, why;
    int32_t left_ext, right_ext, out_len /* letters */;
    int32_t left_end, right_end;
    int32_t left_hit, right_hit;
    int32_t pad[7];
} rb_naive_frag_rec;
int rb_graph_naive_extend_fragments(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, const uint8_t *phase /* may be NULL */,
                                    float min_kmer_cov, int room, int64_t *out_offsets, char *out_seq, rb_naive_frag_rec *recs);
/* Joining of read pairs through the graph — GraphUtils.join (R/util/GraphUtils.java:892-1147), the second half of overlapAndConnect (:5065-5090) that
 * the FragmentAssembler runs on every pair GraphUtils.overlap returned null for (R/RNABloom.java:2148).  A wavefront per pair on the device; the call
 * is read-only.  Pair i is lseq[loffsets[i], loffsets[i+1]) and rseq[roffsets[i], roffsets[i+1]); each read's k-mer list is getKmers(String)'s
 * (lower case and U read as everywhere in this library), nkL and nkR k-mers.  d = the read-paired k-mer distance, g = max_cov_gradient, m =
 * min_kmer_cov.  The reference's lookahead, maxIndelLen and minPercentIdentity are never read by its body and are not part of this call;
 * max_tip_len is passed on to the branch step, which does not read it either (see rb_graph_naive_extend).
 *   Neighbours of a k-mer: its successors (right walk: predecessors) with graph.getCount >= m in the order A C G T (the four-argument
 *   getSuccessors, R/graph/Kmer.java:232-255).  All thresholds are float32, one product each.  Equality of k-mers is Kmer.equals, the k bases:
 *   hashes are compared first and every hit is confirmed on the bases.
 *   Left walk (:912-1030): leftPath = the left list, threshold t = max(m, min(left counts) * g).  While |leftPath| < bound + nkL: no neighbour of
 *   the last k-mer ends the walk.  The only neighbour — or the only one left after dropping those with count < t — is `best`, and t = max(m,
 *   min(t, best.count * g)).  best in the right list: at index 0 the result is leftPath + right list (JOINED, REACHED_RIGHT); at its FIRST index
 *   j > 0 the result is leftPath + right[j ..] (JOINED, INSIDE_RIGHT, index = j) when min count of right[0, j) < min count of leftPath[max(0,
 *   size - j), size), and else the walk goes on to the next test.  best a homopolymer or in leftPath: the walk ends (LOOP).  Else best is added.
 *   No best (a fork): the branch step extendRightSE(leftPath, floor m) — what rb_graph_extend_se computes from the last min(size, d) k-mers; null
 *   or empty ends the walk, else each returned k-mer in turn goes through the two right-list tests above, ends the walk if it is a homopolymer
 *   (EXT_HOMOPOLYMER), and is else added WITHOUT the leftPath test, with c = g * count; if (c < t) t = max(c, m).  The bound is tested at the
 *   top of the loop only: a step's k-mers may overshoot it.
 *   Right walk (:1032-1144), when the left walk did not return: rightPath = the right list reversed, threshold from the right counts, predecessors
 *   and extendLeftSE, bound + nkR.  best in leftPath (as the left walk left it, duplicates included): equal to the left list's last k-mer, the
 *   result is left list + rightPath reversed (JOINED, REACHED_LEFT); else leftPath is cut behind the LAST k-mer equal to best and rightPath reversed
 *   is added (JOINED, PATHS_MEET, index = that k-mer's index).  Else best a homopolymer or in rightPath: null (NONE, RIGHT_LOOP).  A step's k-mer in
 *   leftPath: PATHS_MEET the same way (no REACHED_LEFT test here); a homopolymer: NONE, RIGHT_LOOP; else added without the rightPath test.
 *   Both walks over: NONE, EXHAUSTED.
 *   A pair the reference cannot be asked about is NOT_JUDGED: a read with fewer than k letters (SHORT: the reference throws in get(0)), a letter
 *   outside ACGTU in either read (INVALID_LETTER).
 *   Output: out_offsets (host, n + 1) is a capacity layout from the lengths, bound, d and k alone: pair i has room for nkL + nkR + 2 * (bound + d +
 *   2) k-mers' text, that many + k - 1 bytes (a walk adds at most bound - 1 k-mers one at a time and then one step's, at most d + 1).  out_seq ==
 *   NULL: a size query — only out_offsets is filled, nothing is launched.  out_seq[out_offsets[i] ..] holds the string the returned k-mer list
 *   spells, upper-case A C G T, and recs[i].out_len its length; zeros behind it; NONE / NOT_JUDGED have out_len 0.  recs[i]: l_end / r_end how each
 *   walk ended, l_added / r_added the k-mers it added (before a cut), l_forks / r_forks the branch steps it took, index as above (-1 where there
 *   is none), l_threshold / r_threshold the walks' final thresholds (0 for a walk that did not run).
 * Every pair is judged against the graph as it stands when the call starts.  The call works in pieces cut by the k-mers of both reads
 * (RB_QUERY_PIECE, 16 M by default: 20 bytes of device scratch per k-mer, 72 per pair, and the piece's output text); results do not depend on the
 * cuts.  A pair's paths live in a row of device scratch that a wavefront owns while it works on the pair: 21 bytes for each of the pair's
 * capacity k-mers; a piece has at most 4096 such rows and fewer when they are large — as many as fit 512 MB, but 64 at least.  RB_JOIN_MAX_BOUND
 * is the largest bound accepted: with it 64 rows stay below 0.4 GB plus the reads' share.  It leases a query context (re-entrant on one handle).
 * With rb_graph_profile_enable on the kernels' device time is added to the profile entry "join".
 * Refused (RB_ERR_INVALID, nothing launched): a null handle; a shard handle; a destroyed dbgbf, counting filter or read-pair filter (or a graph
 * made without one); d < 2; bound < 0 or above RB_JOIN_MAX_BOUND; a max_cov_gradient or min_kmer_cov that is not finite or is negative; n < 0;
 * with n > 0: a null loffsets / roffsets / out_offsets (or recs, unless out_seq is NULL too), text missing where offsets say there is some,
 * decreasing offsets.  n == 0 succeeds and touches nothing. */
enum { RB_JOIN_NONE = 0, RB_JOIN_JOINED = 1, RB_JOIN_NOT_JUDGED = 2 };                                                         /* rb_join_rec.outcome */
enum { RB_JOIN_WHY_REACHED_RIGHT = 0, RB_JOIN_WHY_INSIDE_RIGHT = 1, RB_JOIN_WHY_REACHED_LEFT = 2, RB_JOIN_WHY_PATHS_MEET = 3, RB_JOIN_WHY_RIGHT_LOOP = 4,
       RB_JOIN_WHY_EXHAUSTED = 5, RB_JOIN_WHY_SHORT = 6, RB_JOIN_WHY_INVALID_LETTER = 7 };                                     /* rb_join_rec.why */
enum { RB_JOIN_END_NOT_RUN = 0, RB_JOIN_END_NO_NEIGHBOR = 1, RB_JOIN_END_LOOP = 2, RB_JOIN_END_STEP_NONE = 3, RB_JOIN_END_EXT_HOMOPOLYMER = 4,
       RB_JOIN_END_BOUND = 5, RB_JOIN_END_RETURNED = 6 };                                                                      /* rb_join_rec.l_end, r_end */
#define RB_JOIN_MAX_BOUND 65536
typedef struct rb_join_rec {            /* 48 bytes */
    int32_t outcome, why, l_end, r_end;
    int32_t l_added, r_added, l_forks, r_forks;
    int32_t index, out_len /* letters */;
    float l_threshold, r_threshold;
} rb_join_rec;
int rb_graph_join_pairs(rb_graph *g, const char *lseq, const int64_t *loffsets, const char *rseq, const int64_t *roffsets, int64_t n, int bound,
                        float max_cov_gradient, int max_tip_len, float min_kmer_cov, int64_t *out_offsets, char *out_seq, rb_join_rec *recs);
/* Connection of read segments through the graph — GraphUtils.connect(ArrayList<String>, graph, lookahead) (R/util/GraphUtils.java:4836-4872) over the
 * two-string connect (:4874-4896) and the six-argument getMaxCoveragePath (:1591-1675): the first thing the fragment, single-end and long-read workers
 * do with a read (R/RNABloom.java:1980, 2092, 2106, 4781-4829).  A wavefront per gap and then a wavefront per read on the device; the call is read-only.
 * Read i owns list entries [read_segs[i], read_segs[i+1]); entry j is seq[seg_offsets[j], seg_offsets[j+1]).  The list is SeqUtils.filterFastq's /
 * filterFasta's (R/util/SeqUtils.java:1833-1934): entries with an even index within the read are runs of ACGTU (lower case and U read as everywhere in
 * this library), entries with an odd index are placeholders of which only the LENGTH is read.  m = min_kmer_cov; the reference passes 1.  lookahead is
 * accepted and not read: the six-argument getMaxCoveragePath never reads it (as max_tip_len of rb_graph_naive_extend).
 *   By list size (:4838-4843): no entry, the result is "" (EMPTY); one entry, that entry, copied byte for byte whatever its letters (SINGLE).  More:
 *   last = longest = entry 0, and for i = 1, 3, 5, ...: connected = connect(last, entry i+1, bound = length of entry i + k).  Not empty, it becomes
 *   last, and longest when STRICTLY longer; empty, entry i+1 becomes last, and longest when strictly longer: of two runs of equal length the earlier
 *   one is returned (CHAINED).  A connected string ends with the whole of its right segment, so the left k-mer of every gap is the last k-mer of the
 *   segment before it: the gaps are independent of each other, only this choice is sequential.
 *   connect(left, right, bound) (:4874-4896): path = getMaxCoveragePath(last k-mer of left, first k-mer of right, bound, m); "" when the path is null,
 *   is EMPTY (the right k-mer follows the left one directly) or has more than bound k-mers; else left[0, len-k+1) + assemble(path) + right[k-1 ..),
 *   which is left + the last letter of every path k-mer + right[k-1 ..): a path of fewer than k-1 k-mers lets right overlap left.
 *   getMaxCoveragePath: a neighbour is Kmer.getMaxCovSuccessor / Predecessor (R/graph/Kmer.java:301-355), the first strictly largest graph.getCount
 *   >= m among A C G T; equality of k-mers is Kmer.equals, the k bases: forward hashes are compared first and every hit is confirmed on the bases.
 *   Left walk, up to bound times: no neighbour ends it (NO_NEIGHBOR); the neighbour equal to right returns the left path (how = LEFT_ARRIVED, l_end =
 *   ARRIVED); one already in the left path ends it (LOOP); else it is added (BOUND after bound of them).  Right walk, up to bound times from right:
 *   the neighbour equal to left returns the right path (RIGHT_ARRIVED); one in the right path returns null (RIGHT_LOOP, r_end = LOOP); one in the left
 *   path (r_end = MET, index = the LAST left-path entry equal to it) returns null when SeqUtils.isLowComplexityShort of it holds
 *   (MEET_LOW_COMPLEXITY), else left path [0, index] + the right path (PATHS_MEET).  Both walks over: null (EXHAUSTED).
 *   A read the reference cannot be asked about is NOT_JUDGED, with why: a list of 2, 4, ... entries (EVEN_COUNT: the reference throws in get(i+1)); an
 *   even entry under k letters in a list of more than one (SHORT); a letter outside ACGTU in such an entry (INVALID_LETTER), tested in this order.
 *   Output: out_offsets (host, n + 1) is a capacity layout from the lengths alone: the sum of the read's even entries' lengths plus, per odd entry, its
 *   length + 1 (a connected gap adds path_len - k + 1 <= gap length + 1 letters).  out_seq == NULL: a size query — only out_offsets is filled,
 *   nothing is launched.  out_seq[out_offsets[i] ..] holds the returned string and recs[i].out_len its length; zeros behind it.  A SINGLE read's text
 *   is the entry's bytes; a CHAINED read's text is upper-case A C G T also where the run is one segment; EMPTY / NOT_JUDGED have out_len 0.
 *   recs[i]: gaps = the read's odd entries (list size / 2), connected = how many of them connected, first_seg / last_seg the list indices of the
 *   returned run's first and last segment (-1 for EMPTY / NOT_JUDGED).  gaps (may be NULL), one record per odd entry in list order over all reads:
 *   connected; how = the line that returned (NOT_RUN for the gaps of a NOT_JUDGED read); l_end / r_end how each walk ended; l_added / r_added the
 *   k-mers it added; index as above, else -1; path_len the k-mers of the path returned, 0 for null.  connected is 0 for a path that is empty or
 *   longer than bound: how still says which line returned it.
 * Every gap is judged against the graph as it stands when the call starts.  The call works in pieces of whole reads cut by letters + bounds
 * (RB_QUERY_PIECE, 16 M by default); results do not depend on the cuts.  A gap's two path rows — a forward hash per k-mer and the walk's text, 9 bytes
 * per k-mer of bound and 2 k — live in LDS when bound <= 128 (2592 bytes a wavefront) and else in a row of device scratch that a wavefront owns, laid
 * out for the piece's largest bound: at most 4096 rows a launch and fewer when they are large — as many as fit 512 MB, but 64 at least.
 * RB_CONNECT_MAX_BOUND is the largest bound accepted.  It leases a query context (re-entrant on one handle).  With rb_graph_profile_enable on the
 * kernels' device time is added to the profile entry "connect".
 * Refused (RB_ERR_INVALID, nothing launched): a null handle; a shard handle; a destroyed dbgbf or counting filter; a min_kmer_cov that is not finite
 * or is negative; n < 0; with n > 0: a null seg_offsets / read_segs / out_offsets (or recs, unless out_seq is NULL too), decreasing read_segs or
 * seg_offsets, text missing where offsets say there is some, a gap whose bound exceeds RB_CONNECT_MAX_BOUND.  n == 0 succeeds and touches nothing. */
enum { RB_CONNECT_EMPTY = 0, RB_CONNECT_SINGLE = 1, RB_CONNECT_CHAINED = 2, RB_CONNECT_NOT_JUDGED = 3 };                        /* rb_connect_rec.outcome */
enum { RB_CONNECT_WHY_NONE = 0, RB_CONNECT_WHY_EVEN_COUNT = 1, RB_CONNECT_WHY_SHORT = 2, RB_CONNECT_WHY_INVALID_LETTER = 3 };     /* rb_connect_rec.why */
enum { RB_CONNECT_HOW_NOT_RUN = 0, RB_CONNECT_HOW_LEFT_ARRIVED = 1, RB_CONNECT_HOW_RIGHT_ARRIVED = 2, RB_CONNECT_HOW_PATHS_MEET = 3,
       RB_CONNECT_HOW_MEET_LOW_COMPLEXITY = 4, RB_CONNECT_HOW_RIGHT_LOOP = 5, RB_CONNECT_HOW_EXHAUSTED = 6 };                     /* rb_connect_gap_rec.how */
enum { RB_CONNECT_END_NOT_RUN = 0, RB_CONNECT_END_NO_NEIGHBOR = 1, RB_CONNECT_END_LOOP = 2, RB_CONNECT_END_BOUND = 3, RB_CONNECT_END_ARRIVED = 4,
       RB_CONNECT_END_MET = 5 };                                                                                                 /* rb_connect_gap_rec.l_end, r_end */
#define RB_CONNECT_MAX_BOUND 65536
typedef struct rb_connect_rec {         /* 32 bytes */
    int32_t outcome, why, gaps, connected;
    int32_t first_seg, last_seg, out_len /* letters */, pad;
} rb_connect_rec;
typedef struct rb_connect_gap_rec {     /* 32 bytes */
    int32_t connected, how, l_end, r_end;
    int32_t l_added, r_added, index, path_len /* k-mers */;
} rb_connect_gap_rec;
int rb_graph_connect_segments(rb_graph *g, const char *seq, const int64_t *seg_offsets, const int64_t *read_segs, int64_t n, int lookahead,
                              float min_kmer_cov, int64_t *out_offsets, char *out_seq, rb_connect_rec *recs, rb_connect_gap_rec *gaps /* may be NULL */);
/* The fragment screens of the transcript assembler's worker (TranscriptAssemblyWorker.run, R/RNABloom.java:1816-1927) for n host sequences:
 * GraphUtils.isBranchFree (R/util/GraphUtils.java:7651-7672), isChimera (:7674-7760) and isBluntEndArtifact (:8535-8586), with what they
 * call: the gated getMaxCoveragePath (:1677-1776), the gated greedyExtendRight / Left (:1978-1997, :1940-1959) and the four static
 * hasDepthRight / hasDepthLeft (:6680-6778).  A wavefront per sequence on the device; the call is read-only on both handles, and every
 * sequence is judged against the filters as they stood when the call began.  Sequence i is seq[offsets[i], offsets[i+1]); its k-mer list is
 * getKmers(String)'s.  Lower-case letters are read as upper-case ones and U as T, as everywhere in this library.
 *   gate: the `BloomFilter assembledKmers` (the worker's screeningBf) — another handle on the same device with the same k whose dbgbf is
 *   that filter, exactly as rb_graph_greedy_extend's gate.  Required when `what` asks for the chimera or the blunt-end screen; may be NULL
 *   for the branch-free screen alone.
 *   what: RB_SCREEN_BRANCH_FREE | RB_SCREEN_CHIMERA | RB_SCREEN_BLUNT_END.  The three predicates are pure: computing them independently
 *   equals the reference's short-circuit chain, and the caller combines them.  The fields of a screen that was not asked keep 0 / -1.
 *   isBranchFree calls the MEMBER Kmer.hasDepthRight / hasDepthLeft (R/graph/Kmer.java:407-486), which never consult the graph and always
 *   answer true (see rb_graph_naive_extend): branch-free = no k-mer has a right or a left variant (Kmer.getRightVariants / getLeftVariants,
 *   :357-405) with graph.getCount >= 1.
 *   isChimera: both end k-mers in the gate, else chim_why 0.  The forward scan (:7682-7706) and the backward scan (:7714-7738) over the
 *   k-mers' gate bits, a gap of d <= 2k k-mers bridged where the gated getMaxCoveragePath(left, right, d, lookahead, gate) is not null: up
 *   to d steps to the right from `left` — the gated successors (gate.lookup, then graph.getCount > 0), one taken as is, several through the
 *   gated greedyExtendRightOnce (:535-562 over getMaxMedianCoverageRight :312-373) — ending with a path when the step's k-mer equals
 *   `right`, and with the right-hand search when it is one the walk has added before; then up to d steps to the left from `right` ending with
 *   a path at `left` or at a k-mer of the left-hand walk, with null at one the right-hand walk has added before (:1745-1771).  No
 *   low-complexity test.  Kmer.equals is equality of the bases: the device compares forward hashes and confirms on the bases.
 *   chim_why 1: the forward scan reached the last k-mer (:7708); 2: j - i > 2k at :7742; else the two gated greedy walks of at most 1000
 *   k-mers, to the right from k-mer i and to the left from k-mer j: 3 if they share a k-mer, 4 if not (the chimera).
 *   isBluntEndArtifact: max_depth (the worker's maxEdgeClipLength) <= 0 answers false (:8536).  Minima and medians are the reference's
 *   float32 values (getMinimumKmerCoverage(kmers, start, end) :133-145, getMedianKmerCoverage(kmers, start, end) :208-217); d is the graph's
 *   read-paired k-mer distance.  blunt_why 0: neither arm entered; 1 / 2: the left / right arm returned at its range test (:8555, :8574);
 *   3 / 4: the arm's three-clause test (:8559-8561, :8578-8580) failed; 5 / 6: it held (the artifact).  The clauses are evaluated in the
 *   reference's order and not past the first that fails.  The static hasDepth* are depth-first searches over getSuccessors /
 *   getPredecessors (count >= 1; the gated form: gate.lookup, then count > 0) whose test `frontier.size() >= depth` follows every push and
 *   every removal of an empty level.
 *   max_visits: the budget of ONE hasDepth* search, counted in getSuccessors / getPredecessors calls (the first one, of the source, counts).
 *   The reference's search is unbounded and exponential on a tangled graph; the device stops a search that would make call number
 *   max_visits + 1 and reports the sequence as not judged (RB_SCREEN_OVER_BUDGET: the blunt-end bit is clear, blunt_why is 0, boundary is
 *   the arm's; the other two screens are reported as usual).  0 selects RB_SCREEN_DEFAULT_VISITS.
 *   out[8 i ..]: rb_screen_rec.  A sequence without a k-mer is flagged RB_SCREEN_NO_KMER, one with a k-mer and a letter outside ACGTU
 *   RB_SCREEN_BAD_LETTER; neither is judged (every other field 0 / -1) — they stay with the caller.
 * The call works in pieces through the shared driver (RB_QUERY_PIECE k-mers); results do not depend on the cuts.  Device scratch of a piece:
 * 21 bytes per k-mer, 40 per sequence, and 19 P + 2 k bytes of walk rows for each of at most 2048 wavefronts (fewer, down to 16, where
 * that would pass 512 MB), P = max(1000, min(max(max_depth, the longest sequence's k-mers), max_visits)).  With rb_graph_profile_enable on
 * the kernels' device time is added to the profile entry "screen_fragments".
 * Refused (RB_ERR_INVALID, nothing launched): a null handle; a shard handle; a destroyed dbgbf or counting filter; `what` 0 or with other
 * bits; no gate where bit 1 or 2 is asked; a gate that is a shard handle, on another device, with another k or without its dbgbf;
 * lookahead outside [0, 16]; max_depth above 2^20; max_visits < 0; n < 0; with n > 0: a null offsets / out, a null seq where there is text, decreasing offsets.
 * n == 0 succeeds and touches nothing. */
enum { RB_SCREEN_BRANCH_FREE = 1, RB_SCREEN_CHIMERA = 2, RB_SCREEN_BLUNT_END = 4,                                                /* `what`, and rb_screen_rec.flags */
       RB_SCREEN_BAD_LETTER = 8, RB_SCREEN_NO_KMER = 16, RB_SCREEN_OVER_BUDGET = 32 };                                            /* rb_screen_rec.flags: not judged */
enum { RB_CHIM_WHY_ENDS = 0, RB_CHIM_WHY_ASSEMBLED = 1, RB_CHIM_WHY_WIDE_GAP = 2, RB_CHIM_WHY_PATHS_MEET = 3, RB_CHIM_WHY_DISJOINT = 4 };   /* rb_screen_rec.chim_why */
enum { RB_BLUNT_WHY_NO_ARM = 0, RB_BLUNT_WHY_LEFT_RANGE = 1, RB_BLUNT_WHY_RIGHT_RANGE = 2, RB_BLUNT_WHY_LEFT_FAILED = 3, RB_BLUNT_WHY_RIGHT_FAILED = 4,
       RB_BLUNT_WHY_LEFT_ARTIFACT = 5, RB_BLUNT_WHY_RIGHT_ARTIFACT = 6 };                                                         /* rb_screen_rec.blunt_why */
#define RB_SCREEN_DEFAULT_VISITS 65536
typedef struct rb_screen_rec {          /* 32 bytes */
    int32_t flags, chim_why;
    int32_t break_i, break_j;           /* isChimera's i and j as they stand at :7742, or -1 (chim_why 0 or 1, or the screen not asked) */
    int32_t right_len, left_len;        /* k-mers of the two gated greedy walks (:7746-7748), or 0 */
    int32_t blunt_why;
    int32_t boundary;                   /* the entered arm's boundary index (left arm: i, right arm: j + 1), or -1 */
} rb_screen_rec;
int rb_graph_screen_fragments(rb_graph *g, const rb_graph *gate, const char *seq, const int64_t *offsets, int64_t n, int what, int lookahead,
                              int max_depth, int64_t max_visits, rb_screen_rec *out);
/* GraphUtils.represented(kmers, graph, bf, lookahead, maxIndelSize, maxEdgeClipLength, percentIdentity) (R/util/GraphUtils.java:711-824) for
 * n host sequences: the worker's screen between isBranchFree and isChimera.  A wavefront per sequence on the device; read-only on both
 * handles, every sequence judged against the filters as they stood when the call began.  Sequences, letters and the gate (required here) are
 * rb_graph_screen_fragments'; the graph's read-paired k-mer distance d gives maxNumBubbleKmers = d + k.
 *   The scan (:726-804) takes every run of k-mers in the gate; a run shorter than `lookahead` is skipped over and changes nothing.  The first
 *   run that counts, if it starts at k-mer startIndex > 0, tests the left edge (:745-753): where startIndex >= max_edge_clip or the ungated
 *   static hasDepthLeft(kmers[0], max_edge_clip - startIndex) holds, the gated greedyExtendLeft from k-mer startIndex, bound startIndex, must
 *   add exactly startIndex k-mers whose assembled text has getPercentIdentity >= percent_identity against the sequence's first
 *   startIndex + k - 1 letters; otherwise the edge is excused.  Every later run tests the gap behind the last run that counted (:756-796):
 *   wider than d + k k-mers fails; one narrower than k is widened by up to k - width k-mers on each side (:768-782: the index moves BEFORE
 *   the lookup, so a widening that stops on a k-mer outside the gate stays on it); the gated getMaxCoveragePath(left, right, width +
 *   max_indel) must give a path of width - max_indel .. width + max_indel k-mers whose assembled text passes the identity test against the
 *   letters of k-mers left + 1 .. right - 1.  The right edge (:806-818) mirrors the left one.  No run that counts: false (:820).
 *   getPercentIdentity is SeqUtils' (R/util/SeqUtils.java:164-229), stale last column of getDistance included, with the reference's operands
 *   in its order: s the assembled walk or path read left to right, t the sequence's letters; the comparison is one in float32.
 *   max_visits: as rb_graph_screen_fragments' — a hasDepth* search that would pass it leaves the sequence not judged (RB_SCREEN_OVER_BUDGET).
 *   out[12 i ..]: rb_repr_rec.  flags: RB_REPR_REPRESENTED, or one of RB_SCREEN_BAD_LETTER / RB_SCREEN_NO_KMER / RB_SCREEN_OVER_BUDGET for a
 *   sequence that is not judged: nothing is guessed for it, every other field is the blank record's (why -1, the five test fields -1, the
 *   rest 0).  why: the line that returned (RB_REPR_WHY_*).  left, right, expected_len, found_len, distance describe the deciding test — left
 *   edge: 0 and startIndex; gap: left and right after the widening; right edge: lastRepresentedKmerFoundIndex and numKmers - 1; the expected
 *   length; the walk's or path's length (-1: no path); the getDistance value where an alignment was made, else -1 — and are all -1 for why
 *   0, 1 and 4.  tests_passed counts the edge and gap tests that passed before the deciding line, distance_sum adds up their distances,
 *   tips_skipped counts the edges hasDepth* excused: a true record says how it came to be true.  path_form is the form of the last
 *   getMaxCoveragePath result: 0 none (or none asked), 1 the left walk arrived, 2 the right walk arrived, 3 spliced (:1748-1763).
 * Pieces, scratch per k-mer and per sequence as rb_graph_screen_fragments (48 bytes a record); a wavefront's walk rows hold
 * P = max(the longest sequence's k-mers, max(2 k, d + k) + max_indel, min(max_edge_clip, max_visits)) entries, and 4 bytes per letter of
 * the longest sequence where that is more than 1024 letters (the alignment row leaves LDS).  Profile entry "represented".
 * Refused (RB_ERR_INVALID, nothing launched): a null handle or gate; a shard handle; a destroyed dbgbf or counting filter; a gate that is a
 * shard handle, on another device, with another k or without its dbgbf; lookahead outside [0, 16]; max_indel outside [0, 4096];
 * max_edge_clip outside [0, 2^20]; a percent_identity that is not finite; a sequence of more than 2^24 k-mers; max_visits < 0; n < 0; with n > 0: a null offsets / out, a null seq
 * where there is text, decreasing offsets.  n == 0 succeeds and touches nothing. */
enum { RB_REPR_REPRESENTED = 1 };                                                                                                /* rb_repr_rec.flags, beside the not-judged bits of rb_screen_rec */
enum { RB_REPR_WHY_TRUE = 0, RB_REPR_WHY_NO_RUN = 1, RB_REPR_WHY_LEFT_LENGTH = 2, RB_REPR_WHY_LEFT_IDENTITY = 3, RB_REPR_WHY_WIDE_GAP = 4,
       RB_REPR_WHY_NO_PATH = 5, RB_REPR_WHY_PATH_LENGTH = 6, RB_REPR_WHY_PATH_IDENTITY = 7, RB_REPR_WHY_RIGHT_LENGTH = 8,
       RB_REPR_WHY_RIGHT_IDENTITY = 9 };                                                                                         /* rb_repr_rec.why */
enum { RB_REPR_PATH_NONE = 0, RB_REPR_PATH_LEFT = 1, RB_REPR_PATH_RIGHT = 2, RB_REPR_PATH_SPLICED = 3 };                         /* rb_repr_rec.path_form */
typedef struct rb_repr_rec {            /* 48 bytes */
    int32_t flags, why;
    int32_t left, right, expected_len, found_len, distance;     /* the deciding test, or -1 */
    int32_t tests_passed, distance_sum, tips_skipped;
    int32_t path_form;
    int32_t reserved;                   /* 0 */
} rb_repr_rec;
int rb_graph_represented(rb_graph *g, const rb_graph *gate, const char *seq, const int64_t *offsets, int64_t n, int lookahead, int max_indel,
                         int max_edge_clip, float percent_identity, int64_t max_visits, rb_repr_rec *out);
/* The in-order represented-then-add loop of the transcript stage for n host sequences: TranscriptWriter.write (R/RNABloom.java:1639-1720) —
 * `if (!represented(transcriptKmers, graph, screeningBf, …)) { for (Kmer kmer : transcriptKmers) screeningBf.add(kmer.getHash()); … }` — and
 * GraphUtils.reduceRedundancy (R/util/GraphUtils.java:652-699), the same loop over a FASTA sorted by length.  For i = 0 .. n - 1 in list order
 * sequence i is judged exactly as rb_graph_represented judges it, but against the gate AS IT STANDS THEN: the gate at the start of the call
 * plus the k-mers of every earlier kept sequence of this call.  Sequential across sequences, wide inside one: per piece the getKmers rows of
 * all sequences are made side by side, then ONE workgroup walks the piece's sequences in order in ONE launch — all its lanes fill the
 * sequence's gate bits, one wavefront runs the represented body, all lanes add a kept sequence's k-mers (DESIGN.md §5 "Represented, then add").
 *   out[12 i ..]: rb_repr_rec, the same 12 ints as rb_graph_represented writes.  A record that is judged and false (flags == 0) keeps the
 *   sequence: keep[i] = 1, and getHash() of every k-mer of it (the forward hash on a stranded graph, else the signed minimum of the two
 *   strands') is added to the gate's dbgbf through the gate's own num_hash functions (BloomFilter.add, R/bloom/BloomFilter.java:133-141);
 *   median[i] (where median is given) = getMedianKmerCoverage of its counts (R/util/GraphUtils.java:229-247: the float32 mean of the two middle
 *   values for an even number), the writer's `c=` value.  Otherwise keep[i] = 0, nothing is added and median[i] = 0.  Sequences flagged
 *   RB_SCREEN_NO_KMER or RB_SCREEN_BAD_LETTER add nothing and the walk goes on (the reference's worker never hands the writer an empty list;
 *   odd letters are the caller's business, as everywhere).
 *   The stop rule: the walk STOPS at the first RB_SCREEN_OVER_BUDGET sequence, since every later answer would depend on a decision the
 *   library refuses to guess.  That sequence's record says over budget, *n_done is its index, and every later record is the blank record
 *   with RB_SCREEN_NOT_REACHED, keep 0, median 0.  Without such a stop *n_done == n.  The caller decides the stopped sequence itself and
 *   calls again on the rest: the gate carries the state, so one call, three calls and any cut of the list leave the same records, keep
 *   flags and gate bytes — as do the pieces (RB_QUERY_PIECE), whatever their size.
 * g is read-only (shared lock); the gate is WRITTEN (unique lock), the two taken in address order as rb_graph_screen_fragments takes its
 * two.  Scratch as rb_graph_represented with the walk rows of ONE wavefront, and 5 more bytes per sequence.  Profile entry
 * "represented_then_add" (getKmers and the walker of every piece).
 * Refused (RB_ERR_INVALID, no output byte written, no filter changed): everything rb_graph_represented refuses; gate == g; with n > 0 a null
 * keep or n_done.  n == 0 succeeds and touches nothing. */
enum { RB_SCREEN_NOT_REACHED = 64 };                                                                                             /* rb_repr_rec.flags: not judged, behind an over-budget stop */
int rb_graph_represented_then_add(rb_graph *g, rb_graph *gate, const char *seq, const int64_t *offsets, int64_t n, int lookahead, int max_indel,
                                  int max_edge_clip, float percent_identity, int64_t max_visits, rb_repr_rec *out, uint8_t *keep,
                                  float *median /* may be NULL */, int64_t *n_done);
/* GraphUtils.trimReverseComplementArtifact for n host sequences, the last per-sequence step of the transcript worker (R/RNABloom.java:1914), of
 * the fragment worker (:2206) and of the long-read corrector (:3806).  Each of the three overloads is pure and returns a contiguous sub-list of
 * the k-mers it was given, so the answer is a range [begin, end) of the sequence's k-mers (the trimmed text is the letters begin .. end + k - 2,
 * or nothing where the range is empty).  A wavefront per sequence on the device; read-only; the handle's own `stranded` flag is the
 * reference's argument.  Sequences and letters are rb_graph_screen_fragments'.
 *   mode RB_TRIM_HASHES: trimReverseComplementArtifact(kmers, graph, stranded) (R/util/GraphUtils.java:8588-8661).  The HashSet of the
 *   reverse-strand hashes of k-mers 0 .. n/2 - 1; numMatch = the k-mers n/2 .. n - 1 whose forward hash is in it — hashes alone, bases are
 *   never compared; numMatch >= k returns subList(start, n), after the adjustment loop (:8616-8621, down to index 0 without a break) where
 *   start == n/2; else null.  The stranded branch reads getHash() / getReverseComplementHash() (the k-mer's own NTP64RC) and the canonical
 *   one getFHash() / getRHash(): both are the forward and the reverse-strand hash of the k-mer.
 *   mode RB_TRIM_EDGE: trimReverseComplementArtifact(seqKmers, maxEdgeClip, maxIndelSize, minPercentIdentity, graph) (:7918-8057), two passes,
 *   the second on the list the first one left.  A pass finds, for a seed among the first (last) max_edge_clip k-mers (the right-to-left pass
 *   takes max_edge_clip + 1 seeds, :7994), the nearest k-mer whose getHash() equals the seed's getReverseComplementHash() and whose bases are
 *   the seed's reverse complement; the left-to-right scan stops only at a seed index > 0, so a match of seed 0 is kept and trims nothing
 *   unless a later seed overwrites it.  cutIndex then runs inward in strides of k and in single steps, is held at the midpoint, and one of
 *   three lines cuts, two of them chosen by getMinimumKmerCoverage of two windows of k k-mers.
 *   mode RB_TRIM_LONG: the seven-argument overload (:7762-7916): the same anchor scan, the nested extension of anchor and partner up to the
 *   midpoint, the test that both are 2 k k-mers long, and the unstranded return or one of four stranded ones chosen by
 *   getMedianKmerCoverage (float32; an even count is one sum and one quotient) of anchor, middle and partner and by max_cov_gradient.
 *   maxIndelSize and minPercentIdentity are read by neither body and are no parameters here.  max_edge_clip is read by EDGE and LONG,
 *   max_cov_gradient by LONG in a stranded graph; the other modes ignore their values (which are checked all the same).
 *   out[i]: rb_trim_rec, 16 ints.  flags: RB_TRIM_FOUND — a line other than the final fall-through produced the range (HASHES: the result
 *   is not null; EDGE: a pass cut; LONG: a return inside a pass); RB_TRIM_TRIMMED — begin > 0 or end < the number of k-mers; or
 *   RB_SCREEN_NO_KMER / RB_SCREEN_BAD_LETTER for a sequence that is not judged (begin 0, end = its k-mers, both passes blank).
 *   RB_TRIM_NOT_JUDGED is reserved for an input on which the reference throws; the three bodies throw on no list of one or more k-mers,
 *   so no record carries it.  begin, end: the range kept, in the input's numbering; it may be empty (LONG's unstranded return).  mode: the
 *   call's.  pass[p]: why and four ints, blank (all -1) for pass[1] of HASHES and of a LONG call whose first pass returned.
 *     HASHES pass[0]: why 0 null (:8660), 1 :8612, 2 :8622; i0 start (-1: none) and i1 numMatch as they stand at :8610; i2 the start
 *     returned or -1; i3 -1.
 *     EDGE pass[p]: why 0 the :7945 / :8012 test is false, 1 2 3 the lines :7978 :7981 :7985 (pass 0) and :8045 :8048 :8052 (pass 1);
 *     i0, i1 leftIndex and rightIndex as the scan left them; i2 cutIndex after the min / max, i3 cutLength, each -1 where it is not
 *     computed.  Pass 1's indices are in the numbering of the list pass 0 left.
 *     LONG pass[p]: why 0 no anchor, 1 the match-length test failed, 2 the unstranded return, 3 .. 6 the four stranded returns in source
 *     order; i0 .. i3 anchorStart, anchorEnd, partnerStart, partnerEnd as they stand at the :7810 / :7883 test, before the ++ (why 0: as the
 *     scan left them).
 * Pieces as rb_graph_kmers (RB_QUERY_PIECE; results do not depend on the cuts).  Device scratch: 20 bytes per k-mer of a piece (two hashes
 * and a count), 8 per sequence for the k-mer offsets and 64 per sequence for the records; where the call's longest sequence has more than 512
 * k-mers the wavefronts' hash tables leave LDS: 8 bytes x the next power of two >= twice that sequence's k-mers for each wavefront of the
 * launch (at most 2048 wavefronts and 512 MB together, never fewer than 4 wavefronts).  Profile entry "trim_artifacts".
 * Refused (RB_ERR_INVALID, nothing launched): a null or shard handle; a destroyed dbgbf or counting filter; an unknown mode; max_edge_clip
 * outside [0, 2^20]; a max_cov_gradient that is not finite; a sequence of more than 2^24 k-mers; n < 0; with n > 0: a null offsets / out,
 * a null seq where there is text, decreasing offsets.  n == 0 succeeds and touches nothing. */
enum { RB_TRIM_HASHES = 0, RB_TRIM_EDGE = 1, RB_TRIM_LONG = 2 };                 /* mode */
enum { RB_TRIM_FOUND = 1, RB_TRIM_TRIMMED = 2, RB_TRIM_NOT_JUDGED = 32 };        /* rb_trim_rec.flags, beside RB_SCREEN_BAD_LETTER (8) and RB_SCREEN_NO_KMER (16) */
typedef struct rb_trim_pass { int32_t why, i0, i1, i2, i3; } rb_trim_pass;
typedef struct rb_trim_rec {            /* 64 bytes */
    int32_t flags, begin, end, mode;    /* the k-mers kept: [begin, end) of the INPUT list */
    rb_trim_pass pass[2];
    int32_t reserved[2];                /* 0 */
} rb_trim_rec;
int rb_graph_trim_rc_artifacts(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, int mode, int max_edge_clip,
                               float max_cov_gradient, rb_trim_rec *out);
/* Windowed correction of long reads — GraphUtils.correctLongSequenceWindowed (R/util/GraphUtils.java:3087-3185), the second step of
 * LongReadCorrectionWorker.run (R/RNABloom.java:3788-3840), with what it calls: getCoverageStats (:1799-1848), correctInternalErrors
 * (:3402-3602), the six-argument getMaxCoveragePath (:1591-1675), getMedianKmerCoverage (:208-247) and trimLowCoverageEdgeKmers (:3187-3241).
 * On the device, a wavefront per window and pass; the call is read-only on the graph.
 *   Input: sequence i is seq[offsets[i], offsets[i+1]); its k-mer list is getKmers(String)'s, as rb_graph_kmers gives it (nk = max(0, len - k
 *   + 1); count 0 for a window with a letter outside ACGTU).  Every list the reference builds is a chain of k-mers that overlap by k - 1
 *   letters (below), so a list is the text it spells and the counts of a pass are getKmers' of that text.
 *   Solid-k-mer screen (:3099-3110): with min_num_solid > 0 a sequence with fewer than min_num_solid k-mers of count >= min_kmer_cov gives null
 *   (status RB_LONG_NULL, the text comes back as it went in); min_num_solid <= 0 skips the screen.
 *   Passes (:3118-3171): up to max_itr.  shift = window_size / 2; toShift starts false and flips after every pass that corrected something.
 *   Windows [i, end) of k-mers: end = min(i + window_size, nk), for i == 0 of a pass with toShift min(i + shift + window_size, nk); then
 *   end + shift >= nk makes end = nk.  A window of fewer than lookahead k-mers is copied.  The first pass that corrects nothing ends the loop.
 *   Threshold of a window (getCoverageStats with calcDropOff, :1799-1848): the sorted counts c; median = c[len/2], for an even len (c[len/2-1] +
 *   c[len/2]) / 2f; dropoff: last = c[len - lookahead], then for j = len - lookahead - 1 down to 0: c[j] < last * max_cov_gradient (one float32
 *   product) -> dropoff = last, stop; else last = c[j].  T = median, or max(dropoff, min_kmer_cov) where dropoff > 0.
 *   correctInternalErrors(window, T) (:3402-3602): a k-mer is bad if count < T.  kmers2 is the output list.  At a good k-mer that ends a run of
 *   `run` bad ones, in this order:
 *     kmers2 is empty (the run starts the window): the run is copied.
 *     run == k - 1, an SNV bubble (:3432-3467): for every Kmer.getLeftVariants(k, numHash, graph, min_kmer_cov) `var` of the LAST bad k-mer
 *     (the alternatives SeqUtils.getAltNucleotides gives for its first letter, in the order A C G T, whose count >= min_kmer_cov) the counts of
 *     getKmers(first bad k-mer[0, k-1) + var): 2k - 1 letters, k windows.  A variant wins if its minimum >= min_kmer_cov and its median > best;
 *     best starts at Float.MIN_VALUE; the winner needs best >= min_kmer_cov.  Its k k-mers stand for the k - 1 bad ones: the text grows by one
 *     letter (reproduced, not fixed).  Else the run is copied.
 *     run < k - 1 - max_indel_size (:3468-3471): the run is not closed: the good k-mer counts as one more bad k-mer of it and the scan goes on.
 *     Else a path (:3472-3571).  maxLengthDifference D = max_indel_size if percent_identity < 1.0f, else 0.  Left anchor: kmers2's last entry,
 *     then entries last - 2 down to max(0, last - lookahead) (last - 1 is skipped, as in the source), a strictly greater count taking over.
 *     Right anchor: the good k-mer i, then window k-mers i + 1 .. min(i + lookahead, len - 1), a strictly greater count taking over.
 *     path = getMaxCoveragePath(graph, L, R, run + D, lookahead, min_kmer_cov) (:1591-1675: the walk to the right of at most run + D maximum-
 *     coverage successors — the first strictly largest count >= min_kmer_cov among A C G T — that returns when it reaches R and stops at a k-mer
 *     it has added; then the walk back from R, which returns when it reaches L, gives null at a k-mer it has added and, at a k-mer the first walk
 *     added, null if SeqUtils.isLowComplexityShort (:499-543) of it, else the first walk up to that k-mer and its own k-mers; null otherwise).
 *     null or empty: the run is copied.  leftAdjust = kmers2.size() - 1 - L's index, rightAdjust = R's index - i, oriPathLen = run + leftAdjust +
 *     rightAdjust.  A run with a k-mer of count 0: accepted if |oriPathLen - |path|| <= D.  Any other run: altCov = median of the path's counts,
 *     oriCov = median of the run's; accepted if 2 * oriCov <= altCov and the same length test and ((oriCov < min_kmer_cov and altCov >= 10 *
 *     oriCov) or getPercentIdentity(assemble(path), assemble(window k-mers [i - run - leftAdjust, i + rightAdjust))) >= percent_identity) — the
 *     indices are the WINDOW's although leftAdjust was counted in kmers2 (reproduced); where i - run - leftAdjust < 0 the reference throws and
 *     the run is copied here.  getPercentIdentity / getDistance as rb_graph_correct_errors states them (the stale column included).  Accepted:
 *     kmers2 is cut back to L, the path is appended, the scan continues at R.  Else the run is copied.
 *   A run still open at the window's end is copied unless it is the whole window.  A window in which nothing was accepted returns null: its
 *   original k-mers are used.  Medians are float32 ((a + b) / 2f), all comparisons float32.
 *   Chains: a copied run, the k k-mers of getKmers(2k - 1 letters) between the good k-mers before and behind a bubble, and a path from L to R
 *   each overlap their neighbours by k - 1 letters, so kmers2 spells a text and the next pass's list is getKmers of it.
 *   trim_low_cov_edges != 0 (:3173-3179): if the median count of the final list >= 2 * min_kmer_cov, trimLowCoverageEdgeKmers(list, graph,
 *   min_kmer_cov) (:3187-3241): headIndex = the first i whose k-mers i - 1 and i both have count >= min_kmer_cov (0: none); tailIndex = i + 2 for
 *   the last i > headIndex whose k-mers i and i + 1 (i + 1 < nk) both have (nk: none).  headIndex > 0 or tailIndex < nk: the list becomes
 *   [headIndex, tailIndex) if tailIndex - headIndex > 1, else empty (RB_LONG_TRIMMED_TO_NOTHING).  The reference's caller sets the flag per
 *   read (minKmerCov > 1 && !hasPolyA): it is per call here, a split by flag is the caller's.
 *   Letters outside ACGTU follow the existing primitives, exactly as the rb_graph_correct_errors comment states: such windows count 0; the
 *   anchors of a path have a count above 0 and so no such letter; letters taken from a path come out as upper-case A C G T, copied letters as
 *   they went in.
 *   Output: out_offsets (host, n + 1) is an INPUT, the caller's capacity layout: the final text of sequence i is written to out_seq +
 *   out_offsets[i] if its length <= out_offsets[i+1] - out_offsets[i]; else nothing is written for it and recs[i].flags has RB_LONG_OVERFLOW.
 *   recs[i].out_len is the length needed either way; the computation is deterministic, so a second call with room gives the text.  There is no
 *   closed capacity formula (growth compounds over passes; in practice a few letters).
 *   recs[i], 16 ints: status (RB_LONG_NULL the screen failed; RB_LONG_UNCHANGED; RB_LONG_CHANGED a pass corrected or the edge trim cut;
 *   RB_LONG_NO_KMER nk == 0, nothing done — the reference's caller never passes it); passes that corrected; out_len; trim_begin, trim_end: the
 *   k-mers [headIndex, tailIndex) of the final list where the edge trim cut, else -1, -1; then, summed over all passes and windows: snv_replaced,
 *   snv_kept, path_none (null or empty), zero_accepted, zero_kept (runs with a k-mer of count 0), accepted_10x (oriCov < min_kmer_cov and
 *   altCov >= 10 * oriCov held), accepted_identity, cov_kept, short_skipped (good k-mers swallowed by a short run), anchor_moved (path events
 *   whose left or right anchor left its default); flags.
 * Window slots: a window of len k-mers may return at most len + (len / 2) * max(max_indel_size, 1) k-mers (accepted events are at least two
 * input k-mers apart and add at most that many each); a window has at most 2 window_size k-mers (the first window of a shifted pass merged with
 * the rest), and a slot may hold 2^30 k-mers, so window_size * (2 + max(max_indel_size, 1)) <= 2^30 is required: RB_LONG_MAX_WINDOW is admitted
 * with max_indel_size <= 1022, 4096 with any.  RB_ERR_STATE, in the middle of the call (earlier sequences' records may be written, none is
 * complete): a slot is outgrown (an internal error), a sequence grows beyond 2^30 letters, or one pass over a piece has 2^31 windows or more.
 * The call works in pieces (RB_QUERY_PIECE input k-mers, by default 4 M); results do not depend on the cuts.  Texts and counts stay on the
 * device between passes; only the final texts and 5 ints a sequence come back.  Device scratch of a piece: 2 x (1 byte a letter + 1 byte a
 * k-mer) of its live sequences, the windows' slots (above) and, for each of at most 2048 wavefronts, rows bounded by the longest window W of
 * the pass, not by the read: 25 (W + max_indel_size) + 5 W + 2 k bytes or so.  It leases a query context (re-entrant on one handle).  Profile
 * entry "correct_long": the interval from a piece's first to its last kernel, the host's work between the passes included.
 * Refused (RB_ERR_INVALID, nothing launched): a null handle / offsets / p / out_offsets / out_seq / recs (n > 0), seq where there is text; a
 * shard handle; a destroyed dbgbf or counting filter; max_cov_gradient or percent_identity not finite; decreasing offsets (input or capacity);
 * k < 2; window_size < 1 (the reference would loop forever) or > RB_LONG_MAX_WINDOW (2^20); lookahead < 1 or > RB_LONG_MAX_WINDOW; max_itr < 0;
 * max_indel_size outside 0..4096; window_size * (2 + max(max_indel_size, 1)) > 2^30.  n == 0 succeeds and touches nothing; a null seq is taken
 * where no sequence has a letter. */
enum { RB_LONG_NULL = 0, RB_LONG_UNCHANGED = 1, RB_LONG_CHANGED = 2, RB_LONG_NO_KMER = 3 };     /* rb_long_rec.status */
enum { RB_LONG_OVERFLOW = 1, RB_LONG_TRIMMED_TO_NOTHING = 2 };                                  /* rb_long_rec.flags */
#define RB_LONG_MAX_WINDOW (1 << 20)
typedef struct rb_long_params {
    int32_t max_itr, lookahead, max_indel_size, min_kmer_cov, min_num_solid, trim_low_cov_edges, window_size;
    float max_cov_gradient, percent_identity;
} rb_long_params;
typedef struct rb_long_rec {            /* 64 bytes */
    int32_t status, passes, out_len, trim_begin, trim_end;
    int32_t snv_replaced, snv_kept, path_none, zero_accepted, zero_kept, accepted_10x, accepted_identity, cov_kept, short_skipped, anchor_moved;
    int32_t flags;
} rb_long_rec;
int rb_graph_correct_long(rb_graph *g, const char *seq, const int64_t *offsets, int64_t n, const rb_long_params *p,
                          const int64_t *out_offsets, char *out_seq, rb_long_rec *recs);
/* Kmer.getSuccessors/getPredecessors R/graph/Kmer.java:210-255, CanonicalKmer.java:226-270:
 * for each (f, r, char_out) the 4 neighbours in order A,C,G,T: forward hash, reverse hash and
 * graph.getCount.  direction 0 = successors (char_out = first base), 1 = predecessors
 * (char_out = last base); 2 = left variants (first base replaced, char_out = first base), 3 = right
 * variants (last base replaced, char_out = last base) — Kmer.getLeftVariants/getRightVariants
 * R/graph/Kmer.java:357-405 over R/bloom/hash/{,Canonical}{Left,Right}VariantsNTHashIterator.java; the
 * entry whose base equals char_out is the k-mer itself.  Callers apply minKmerCov to count4.  * On a shard handle: candidate hashes only (count4 = 0), counts by rb_shard_query_* (ShardRank.neighbors). */
int rb_graph_neighbors(rb_graph *g, const uint64_t *f, const uint64_t *r, const uint8_t *char_out,
                       size_t n, int direction, uint64_t *f4, uint64_t *r4, float *count4);

/* Greedy maximum-coverage walks, batched: the loop the reference runs around Kmer.getMaxCovSuccessor /
 * getMaxCovPredecessor (R/graph/Kmer.java:301-355) in GraphUtils.getMaxCoveragePath (R/util/GraphUtils.java:1591-1675)
 * — one JNI call per batch of walks instead of 4 graph.getCount calls per step.  seeds / targets: n x k bases
 * (ASCII, left to right; targets may be NULL).  direction 0 extends to the right (successors), 1 to the left
 * (predecessors).  Per step the best neighbour is the first strict maximum of graph.getCount among A,C,G,T
 * with count >= min_cov.  Walk i ends with out_reason[i] = 0 no such neighbour, 1 the best neighbour is the
 * target (not appended), 2 it is a k-mer the walk appended before (not appended; Kmer.equals: same bases),
 * 3 `bound` k-mers appended, 4 the seed holds a base outside ACGTU.  out_len[i] appended k-mers; for walk i and
 * step j < out_len[i]: out_bases[i*bound + j] the base added (last base of the k-mer for direction 0, first base
 * for direction 1), out_f / out_r / out_count (each may be NULL: 20 of the 21 bytes a step returns) its forward hash,
 * reverse hash, graph.getCount. */
int rb_graph_walk(rb_graph *g, const char *seeds, const char *targets, size_t n, int direction, int bound, float min_cov,
                  char *out_bases, uint64_t *out_f, uint64_t *out_r, float *out_count, int32_t *out_len, uint8_t *out_reason);

/* GraphUtils.greedyExtendRight / greedyExtendLeft(graph, source, lookahead, bound), batched
 * (R/util/GraphUtils.java:1961-1976, :1906-1921): up to `bound` times greedyExtend{Right,Left}Once (:501-529, :564-592) —
 * the neighbours with graph.getCount >= 1 (Kmer.getSuccessors / getPredecessors, R/graph/Kmer.java:199-255); none ends the
 * walk (out_reason 0), one is taken, several are scored with getMaxMedianCoverage{Right,Left} (:248-310, :375-438: the
 * best minimum k-mer coverage over the depth-first paths of exactly `lookahead` k-mers starting at the candidate) and
 * the highest score wins, a tie going to the strictly larger count.  out_reason 3 = bound reached, 4 = seed with a
 * base outside ACGTU.  Outputs as rb_graph_walk (out_count may be NULL).  lookahead <= 16.
 * gate (may be NULL): the `BloomFilter bf` of the gated variants (greedyExtendRight(graph, source, lookahead, bound, bf),
 * :1978-1993; Kmer.getSuccessors(k, numHash, graph, bf), R/graph/Kmer.java:257-299: a neighbour must pass bf.lookup before
 * its count is read) — another handle on the same device, same k, whose dbgbf is that filter. */
int rb_graph_greedy_extend(rb_graph *g, const rb_graph *gate, const char *seeds, size_t n, int direction, int lookahead, int bound,
                           char *out_bases, float *out_count, int32_t *out_len, uint8_t *out_reason);
/* GraphUtils.naiveExtendRight / naiveExtendLeft R/util/GraphUtils.java:6780-7112, one walk per seed k-mer (n seeds of k
 * bases): follow the only neighbour with count >= min_cov while the walk is unbranched.  mode 0 = the forms with a
 * terminator set (:6780-6833, :6959-7012): every k-mer of the walk's terminator sequence term_seq[term_off[i], term_off[i+1])
 * stops it, and so does a k-mer it added before; `cap` = room for added bases per walk (these forms have no bound; a walk
 * that fills it reports reason 6 and can be continued from its last k-mer).  mode 1 = the bounded forms (:6835-6886,
 * :7014-7065), mode 2 = naiveExtend{Right,Left}NoBackChecks (:6888-6933, :7067-7112); both write up to bound + 1 bases per
 * walk (out_bases is n * (bound + 1)).  maxTipLength does not appear: it only feeds Kmer.hasDepthLeft / hasDepthRight,
 * which never consult the graph and always return true (R/graph/Kmer.java:407-486).
 * out_reason: 0 no neighbour, 1 back branch (a variant of the current k-mer in the base about to leave exists), 2 several
 * neighbours, 3 bound, 4 seed with a base outside ACGTU, 5 terminator / already-added k-mer, 6 capacity, 7 the candidate
 * repeats the seed or the k-mer added last (mode 2). */
int rb_graph_naive_extend(rb_graph *g, const char *seeds, size_t n, int direction, int mode, int bound, int cap, float min_cov,
                          const char *term_seq, const int64_t *term_off, char *out_bases, int32_t *out_len, uint8_t *out_reason);

/* ---- filter state: popcount / FPR / raw bytes (the on-disk format of
 *      R/bloom/BloomFilter.java:113-124 is exactly these bytes,
 *      R/bloom/buffer/UnsafeByteBuffer.java:160-201) ---- */
int rb_filter_size(rb_graph *g, int which, int64_t *size /* bits or bytes */, int64_t *nbytes, int *num_hash);
/* bit filters: set bits (UnsafeByteBuffer.bitPopCount :131-150); cbf: non-zero bytes (:121-129) */
int rb_filter_popcount(rb_graph *g, int which, int64_t *out);
int rb_filter_fpr(rb_graph *g, int which, float *out); /* BloomFilter.getFPR :185-194 */
/* 64-bit digest of the filter bytes this handle holds, computed on the device: the wrapping sum, over the non-zero 32-bit
 * little-endian words, of splitmix64(global word number * 0x9E3779B97F4A7C15 + word).  The digests of the shards of a
 * distributed filter add up (mod 2^64) to the digest of the same filter on one GPU, so filters too large to export
 * (BASELINE config 4: 150 GB of counters) are compared on the device.  No reference counterpart (the reference compares
 * nothing); tests/test_gpu_config3.py, rnabloom.graph.fold_bytes is the host restatement. */
int rb_filter_fold(rb_graph *g, int which, uint64_t *out);
int rb_filter_export(rb_graph *g, int which, void *dst, size_t nbytes);
int rb_filter_import(rb_graph *g, int which, const void *src, size_t nbytes);
int64_t rb_expected_size(int64_t n, float fpr, int num_hash); /* BloomFilter.getExpectedSize :196-199 */
/* BloomFilterDeBruijnGraph.destroyDbgbf / destroyCbf / destroyRpkbf / destroyFpkbf R/graph/BloomFilterDeBruijnGraph.java:249-275
 * (BloomFilter.destroy :244-246): frees the filter's device memory; rb_filter_size then reports RB_ERR_STATE and calls
 * that need the filter fail.  rb_graph_init_fragment_pairs may create an fpkbf again (restorePkbf :341-350). */
int rb_graph_destroy_filter(rb_graph *g, int which);
/* CountingBloomFilter.incrementAndGet(long[]) R/bloom/CountingBloomFilter.java:196-222 for h0[0..n) one after the other,
 * in array order (every call sees the increments before it); out[i] = MiniFloat.toFloat(updated).  Order-exact and serial
 * on the device: meant for the subsampler's short per-read sequences, not for bulk counting (rb_graph_apply). */
int rb_filter_increment_and_get(rb_graph *g, const uint64_t *h0, size_t n, float *out);
/* CountingBloomFilter.getBloomFilter(minCov) R/bloom/CountingBloomFilter.java:328-338: bit i of filter `which` of `dst`
 * (same number of bits as src has counters, same device) := MiniFloat.toFloat(counter i of src) >= min_cov. */
int rb_cbf_to_bloom(rb_graph *src, float min_cov, rb_graph *dst, int which);

/* ---- hash-only test hook: {,Canonical,ReverseComplement}NTHashIterator over every usable
 *      segment of every read of a batch.  mode 0 fwd, 1 canonical, 2 reverse-complement.
 *      out_h0[count] in read order; out_read/out_pos optional.  Call with out_h0 == NULL to get
 *      the count. ---- */
int rb_nthash_batch(const rb_batch *b, int k, int mode, int64_t first, int64_t n, int64_t *count,
                    uint64_t *out_h0, uint32_t *out_read, uint32_t *out_pos);

/* ---- sketching over long reads (BASELINE config 5): hash-only, no shared state => plain data
 *      parallelism over reads (replicas on several GPUs, no collective).  Both hash EVERY window of a
 *      read like the reference iterators do (no segmentation; unusable bases hash as seed 0). ----
 * MinimizerHashIterator.next() R/bloom/hash/MinimizerHashIterator.java:27-128 over
 * LongRollingWindow R/util/LongRollingWindow.java:23-83: for every window of w consecutive k-mers
 * the SIGNED minimum of hVals[0] (mode 0 forward / 1 canonical / 2 reverse-complement iterator).
 * moffsets[n_reads+1]: read i yields max(0, len_i-k+1-w+1) windows.  out_pos = LongRollingWindow.getMinPos()
 * (the rolling window is replayed exactly, including which of several equal minima it reports). */
int rb_minimizers(int device, const char *seq, const int64_t *offsets, int64_t n_reads, int k, int w, int mode,
                  int64_t *moffsets, uint64_t *out_hash, int64_t *out_pos);
/* StrobeHashIterator.getInterval(p) R/bloom/hash/StrobeHashIterator.java:133-164 (as used by
 * SeqSubsampler.strobemerBased R/util/SeqSubsampler.java:367): order-n randstrobes over FORWARD k-mer
 * hashes, unsigned argmin of combineHashValues, ties -> rightmost, equal k-mer hash -> slide right.
 * soffsets[n_reads+1]: read i yields numKmers - wMax*(n-2) - wMin strobemers if numKmers > wMax*(n-1). */
int rb_strobemers(int device, const char *seq, const int64_t *offsets, int64_t n_reads, int k, int n, int wmin, int wmax,
                  int64_t *soffsets, uint64_t *out_hash, int32_t *out_start, int32_t *out_end);

/* The other strobemer iterators, batched the same way (one thread per strobemer).  `count_in` (may be NULL): a handle
 * whose counting filter is asked CountingBloomFilter.getCount(long) (R/bloom/CountingBloomFilter.java:235-251) for
 * every hash without leaving the device — the "hash -> cbf.getCount" half of SeqSubsampler.strobemerBased / kmerBased
 * (R/util/SeqSubsampler.java:389-395, 176-179); out_count then receives the counts.
 * rb_randstrobes: StrobeHashIterator.next() / get() R/bloom/hash/StrobeHashIterator.java:73-131 and
 * CanonicalStrobeHashIterator.next() / get() R/bloom/hash/CanonicalStrobeHashIterator.java:79-140.  out_pos: n
 * positions per strobemer (the k-mer itself, then the strobes = getStrobes() / HashedPositions.pos). */
#define RB_STROBE_CANONICAL 1 /* CanonicalStrobeHashIterator: strobes chosen on forward hashes, SIGNED min with the reverse chain */
#define RB_STROBE_SLIDE 2     /* StrobeHashIterator.get / getInterval: the chosen strobe slides across equal k-mer hashes */
#define RB_MAX_STROBES 8
int rb_randstrobes(int device, const char *seq, const int64_t *offsets, int64_t n_reads, int k, int n, int wmin, int wmax, int flags,
                   rb_graph *count_in, int64_t *soffsets, uint64_t *out_hash, int32_t *out_pos, float *out_count);
/* Strobe3HashIterator / CanonicalStrobe3HashIterator next() / get() (R/bloom/hash/Strobe3HashIterator.java:78-151,
 * R/bloom/hash/CanonicalStrobe3HashIterator.java:85-225): strobemers of positions getMin()..getMax(); read i yields
 * numKmers - 2*wMin (canonical: numKmers - 2*wMax, if positive) when numKmers > 2*wMin.  out_pos: {pos1, p, pos3}. */
int rb_strobe3(int device, const char *seq, const int64_t *offsets, int64_t n_reads, int k, int wmin, int wmax, int canonical,
               rb_graph *count_in, int64_t *soffsets, uint64_t *out_hash, int32_t *out_pos, float *out_count);
/* SeqSubsampler.kmerBased's k-mer pair hashes R/util/SeqSubsampler.java:176-179 (stranded: combine(h[i], h[i+shift]))
 * and :266-268 (min_signed(combine(f[i], f[i+shift]), combine(r[i+shift], r[i]))): read i yields numKmers - shift. */
int rb_kmer_pair_hashes(int device, const char *seq, const int64_t *offsets, int64_t n_reads, int k, int shift, int canonical,
                        rb_graph *count_in, int64_t *poffsets, uint64_t *out_hash, float *out_count);
/* MinimizerHashIterator.nextMinimizer() R/bloom/hash/MinimizerHashIterator.java:97-112 while hasNext(): the first
 * window's minimizer, then one entry whenever the position of the window minimum moves (the sequence
 * SeqUtils.getMinimizerChainString consumes, R/util/SeqUtils.java:1731-1757).  out_hash / out_pos need room for one
 * entry per window (rb_minimizers' count); moffsets[n_reads+1] receives the per-read offsets of what was written. */
int rb_minimizers_next(int device, const char *seq, const int64_t *offsets, int64_t n_reads, int k, int w, int mode,
                       int64_t *moffsets, uint64_t *out_hash, int64_t *out_pos);
/* GraphUtils.getMinimizers(seq, numKmers, itr, windowSize) R/util/GraphUtils.java:2462-2549: the distinct window
 * minimizers of each read, sorted as signed longs.  Reads with numKmers <= windowSize yield ONE value,
 * min_signed(stale[i], every k-mer hash), where stale[i] is what itr.hVals[0] held before the call (:2480-2488:
 * 0 on a fresh iterator — pass stale = NULL — else the last hash of the previous sequence).  out needs room for
 * max(1, windows) entries per read. */
int rb_minimizer_set(int device, const char *seq, const int64_t *offsets, int64_t n_reads, int k, int w, int mode,
                     const uint64_t *stale, int64_t *moffsets, uint64_t *out);

/* ---- preparation of raw long reads: text work, no graph ----
 * What LongReadCorrectionWorker.run (R/RNABloom.java:3700-3779) does to a raw read before it makes a segment, for n host reads in one call:
 *   1. reverse_complement != 0: SeqUtils.reverseComplement (R/util/SeqUtils.java:1120-1152: A C G T U -> T G C A A, every other byte, lower
 *      case included, -> N).  The result is "the finder's read"; its length is the raw length, and length < min_len ends here: RB_PREP_SHORT.
 *   2. polya != 0 (minPolyATailLengthRequired > 0): PolyATailFinder.findPolyATail (R/util/PolyATailFinder.java:319-338 over findPolyASeed
 *      :201-277, letters A a) and, unless strand_specific, findPolyTHead (:476-495 over findPolyTSeed :355-432, letters T t), with the finder's
 *      seed_length, min_identity, max_gap and window = max(seed_length, window) (setWindow).  Float32 as the reference: a seed window passes when
 *      count / (float) seed_length >= min_identity, two regions join when prev.end + max_gap >= best.start or the float32 share of the letter
 *      between them >= min_identity.  Both quirks of the refinement are kept: a tail region that starts at the search start walks down while
 *      seq[start] is an A, so it ends ON the other letter (or at 0); findPolyTSeed opens its region one letter longer than the seed.
 *   3. the five-way rule (:3715-3766).  Stranded: cut at tail.end and hasPolyA only if tail.end < length.  Else tail only: cut if tail.end <
 *      length, hasPolyA either way; head only: cut from head.start, reverse-complement (the map of 1., once more), hasPolyA; both: keep
 *      [head.end, tail.start) if head.end < tail.start, hasPolyA stays false.  The result is "the transformed read".
 *   4. SeqUtils.trimLowComplexityRegions(transformed, lc_window, lc_min_length) (:839-902): with numWindows = len / lc_window >= 5 the windows
 *      start at offset = (len % lc_window) / 2, a window is low by isLowComplexityLong (:585-659: only upper-case A C G T U count, U as T;
 *      thresholds round(len * 0.89f), round(len * 0.89f / 2.0f), round(len * 0.89f / 3.0f) in float32 with Math.round), and if numLow * lc_window
 *      >= lc_min_length the runs of complex windows are the segments — a run from window 0 starts at letter 0, a run open at the end runs to
 *      len —, else the whole read is one segment.  With fewer windows: no segment if isLowComplexityLongWindowed (:661-682: windows of 50, with 4
 *      or more of them low when numLow >= floor(0.75 * numWindows), else isLowComplexityLong of the whole), otherwise the whole read.
 *   5. more than one segment clears hasPolyA (:3777-3779).
 * recs[i], 16 ints: status (RB_PREP_SHORT: nothing else is set but -1 in the four region fields; RB_PREP_LOW_COMPLEXITY: no segment, the
 * worker emits the transformed read flagged low-complexity; RB_PREP_SEGMENTS); flags (RB_PREP_REVCOMP the transformed read runs against the
 * input: exactly one of the argument and the head rule turned it; RB_PREP_MAPPED_TWICE both did: it runs with the input but its letters went
 * through the complement map twice, U -> T and every byte outside ACGTU -> N; RB_PREP_HAS_POLYA after 5.; RB_PREP_TAIL_FOUND / HEAD_FOUND a
 * region is not null; RB_PREP_CUT_FIRED; which of the three complexity routes ran: RB_PREP_ROUTE_WINDOWS, _WINDOWED (windows of 50), _WHOLE);
 * kept_begin, kept_end: the input letters the transformed read is made of, in input coordinates; tail_start, tail_end, head_start, head_end in
 * the coordinates of the finder's read, -1 for null; n_windows, n_low, offset of the route that ran (_WHOLE: 0, 1 if low, 0); n_segments; the
 * seed searches the tail chain and the head chain made; 0, 0.
 * Segments: [begin, end) pairs in the transformed read's coordinates, n_segments of them at out_segs + 2 * seg_offsets[i].  seg_offsets (n + 1)
 * is an INPUT, the caller's layout as in rb_graph_paired_kmer_segments: every read needs room for max(1, (len / lc_window + 1) / 2) segments.
 * Slots a read does not fill are not touched.  out_seq (may be NULL): the transformed read of every read that is not RB_PREP_SHORT, kept_end -
 * kept_begin bytes at out_seq + offsets[i] — a caller takes its segments as substrings without a host pass.  kernel_ms (may be NULL) receives
 * the time from the first to the last kernel of every piece, summed, by events.
 * One kernel, a wavefront per read: the finder's scans are ballots over the positions of a search range, the complexity pass has the lanes
 * across a window's letters with the window's 84 counters in LDS; nothing is staged, so a read of any length (up to 2^30) works.  The call works
 * in pieces of 64 M letters (RB_QUERY_PIECE counts letters here); results do not depend on the cuts.  Device memory of a piece: 1 byte a letter
 * (2 with out_seq), 16 bytes a read and 8 a segment slot.
 * Refused (RB_ERR_INVALID, before anything is written): null p; n < 0; null offsets / seg_offsets / recs / out_segs (n > 0), seq where there is
 * text; min_len < 0; seed_length < 1; min_identity not in (0, 1]; max_gap outside 0 .. 2^30; window < 0; lc_window outside 1 .. 1024;
 * lc_min_length < 0; decreasing offsets; a read of more than 2^30 letters; a read's room below the bound.  n == 0 succeeds and touches nothing. */
enum { RB_PREP_SHORT = 0, RB_PREP_LOW_COMPLEXITY = 1, RB_PREP_SEGMENTS = 2 };                   /* rb_prep_rec.status */
enum { RB_PREP_REVCOMP = 1, RB_PREP_HAS_POLYA = 2, RB_PREP_TAIL_FOUND = 4, RB_PREP_HEAD_FOUND = 8, RB_PREP_CUT_FIRED = 16,
       RB_PREP_ROUTE_WINDOWS = 32, RB_PREP_ROUTE_WINDOWED = 64, RB_PREP_ROUTE_WHOLE = 128, RB_PREP_MAPPED_TWICE = 256 };   /* rb_prep_rec.flags */
#define RB_PREP_MAX_LC_WINDOW 1024
typedef struct rb_prep_params {
    int32_t min_len, reverse_complement, strand_specific, polya, seed_length, max_gap, window, lc_window, lc_min_length;
    float min_identity;
} rb_prep_params;
typedef struct rb_prep_rec {            /* 64 bytes */
    int32_t status, flags, kept_begin, kept_end, tail_start, tail_end, head_start, head_end;
    int32_t n_windows, n_low, offset, n_segments, tail_searches, head_searches, reserved[2];
} rb_prep_rec;
int rb_long_prepare(int device, const char *seq, const int64_t *offsets, int64_t n, const rb_prep_params *p, const int64_t *seg_offsets,
                    rb_prep_rec *recs, int32_t *out_segs, char *out_seq, double *kernel_ms);

/* ---- subsampling of long reads: the accept / reject loop of SeqSubsampler on the device ----
 * SeqSubsampler.strobemerBased (R/util/SeqSubsampler.java:339-481, the loop body :374-460) and kmerBased (:120-337, the loop bodies :150-226
 * stranded and :233-318 canonical) for n_reads host reads, judged IN ARRAY ORDER against the counting filter of `cbf`, which the call reads AND
 * writes; the handle is taken exclusively.  The filter's state and the handle's op ordinal carry from one call to the next, so a library cut
 * into several calls gives the bytes of one call.  Per read:
 *   1. its elements are hashed.  RB_SUB_STROBEMER: StrobeHashIterator(3, k, wmin, wmax).getInterval(i) — hash, start = i, end — as rb_strobemers;
 *      start() fails for numKmers <= 2 * wmax (or fewer than k letters) and the read is KEPT (:456-460).  RB_SUB_KMER: the k-mer pairs at shift
 *      k + 1 as rb_kmer_pair_hashes (canonical != 0: min of the forward and the reverse pair, :266-268) for i in [start, end), start / end as
 *      :167-175 with tooShort = length < 3 * max_edge_clip; start() fails for fewer than k letters and the read is DROPPED; end - start < 0
 *      throws in the reference (new boolean[negative]) and is reported as RB_SUB_NOT_JUDGED, dropped, nothing incremented.
 *   2. seen[i] = cbf.getCount(hash_i) >= max_multiplicity (CountingBloomFilter.getCount :235-251).
 *   3. the scan.  Strobemer mode :394-434 with maxEdgeClip = max(max_edge_clip, wmax): the namInterval fold (ComparableInterval.merge succeeds
 *      iff IntervalUtils.getOverlap > 0), its four breaks and the tail test.  k-mer mode :187-195 / :273-281: a run of 2k + 1 unseen pairs.
 *   4. a kept read increments every DISTINCT hash of a set once (CountingBloomFilter.increment :170-194): strobemer mode the hashes with
 *      !seen[i] (:441-453); k-mer mode ALL pair hashes at gaps 1, 2 and 0 over the three ranges of :204-217 (:290-309).  The reference leaves
 *      the order of one read's increments open (parallelStream over a HashSet); here it is fixed: the distinct hashes are incremented as if one
 *      after the other in order of FIRST OCCURRENCE (strobemers by i; pairs in the gap-1 list, then gap-2, then gap-0, each by i), the j-th
 *      increment of the call drawing rng31(seed, ordinal0 + j, 0), and the op ordinal advances by the number of increments — what a loop of
 *      rb_graph_apply(RB_OP_ADD_COUNT_ONLY) of one hash does.  Any serial order is a legal execution of the reference.
 * out_keep[i]: 1 kept, 0 dropped.  out_recs (may be NULL), 8 ints a read in this order: status (RB_SUB_*); the reference line that decided
 * (RB_SUB_LINE_*); the deciding index (-1 where no element decided); strobemer mode namInterval.start and namInterval.end (-1, -1 when null),
 * k-mer mode `start` and missingChainLen when the loop ended; the number of elements (strobemers, or end - start); how many are unseen; the
 * distinct hashes incremented.  totals (may be NULL), 4 values: reads kept, increments, reads not judged, nanoseconds in the walker kernel
 * (by events, summed over the pieces).
 * Hashing of a piece is the sketch kernels of rb_strobemers / rb_kmer_pair_hashes with the results left on the device; then ONE launch of ONE
 * workgroup walks the piece's reads one after the other: all lanes look the counts up, the scan is a prefix maximum plus a first-index
 * reduction, the distinct hashes are picked in an open-addressing set (in LDS up to RB_SUB_LDS_ELEMS elements of a read, in device scratch
 * beyond), increments that share no counter with another increment of the read are applied by all lanes at once and the others by one lane in
 * the defined order.  Pieces of 16 M letters (RB_QUERY_PIECE counts letters here); results do not depend on the cuts.
 * Refused (RB_ERR_INVALID): null cbf / p / out_keep, a shard handle, no counting filter, k outside the handle's, mode outside 0 .. 1, strobemer
 * mode with wmin < 1 or wmax < wmin, max_multiplicity < 1, max_edge_clip < 0 or above 2^28, decreasing offsets, a read of more than 2^28 letters. */
enum { RB_SUB_STROBEMER = 0, RB_SUB_KMER = 1 };                                                   /* rb_subsample_params.mode */
enum { RB_SUB_DROPPED = 0, RB_SUB_KEPT_SCAN = 1, RB_SUB_KEPT_TAIL = 2, RB_SUB_KEPT_START_FAILED = 3, RB_SUB_NOT_JUDGED = 4 };   /* status */
enum { RB_SUB_LINE_SEEN_BEYOND_EDGE = 402, RB_SUB_LINE_MERGE_FAILED = 408, RB_SUB_LINE_UNSEEN_BEYOND_EDGE = 414, RB_SUB_LINE_GAP = 421,
       RB_SUB_LINE_TAIL = 429, RB_SUB_LINE_START_FAILED = 456,                                    /* strobemer mode */
       RB_SUB_LINE_KMER_START_FAILED = 153, RB_SUB_LINE_KMER_RANGE = 178, RB_SUB_LINE_KMER_CHAIN = 191, RB_SUB_LINE_KMER_NO_CHAIN = 197,
       RB_SUB_LINE_KMER_START_FAILED_C = 236, RB_SUB_LINE_KMER_RANGE_C = 263, RB_SUB_LINE_KMER_CHAIN_C = 277, RB_SUB_LINE_KMER_NO_CHAIN_C = 283 };
#define RB_SUB_LDS_ELEMS 2048
typedef struct rb_subsample_params {
    int32_t mode, k, wmin, wmax, canonical, max_multiplicity, max_edge_clip, reserved;
} rb_subsample_params;
int rb_subsample_reads(rb_graph *cbf, const rb_subsample_params *p, const char *seq, const int64_t *offsets, int64_t n_reads,
                       uint8_t *out_keep, int32_t *out_recs, int64_t *totals);

/* ---- input formats ----
 * FASTQ text -> the buffers rb_graph_add_reads / rb_batch_create_ascii take.  FastqReader.nextWithoutName
 * R/io/FastqReader.java:140-186: four lines per record, line 1 starts with '@', line 3 with '+' (else RB_ERR_INVALID with
 * the reference's message), a record cut off by the end of the text is dropped; lines end at \n, \r\n or \r.
 * Threaded (n_threads <= 0: all hardware threads).  Call with offsets == NULL for the record count; seq / qual
 * (qual may be NULL) need offsets[n_reads] bytes — len is always enough. */
int rb_fastq_split(const char *text, size_t len, int n_threads, char *seq, char *qual, int64_t *offsets, int64_t cap_reads,
                   int64_t *n_reads);

/* FileUtils.getTextFileReader for ".gz" (R/util/FileUtils.java:50-57: GZIPInputStream, every member of a concatenated file).
 * dst == NULL: *out_len = uncompressed size.  Whatever follows a member and is not another gzip header (padding, garbage) ends the stream
 * silently, as GZIPInputStream.readTrailer does; the first member must be gzip.  BGZF input (bgzip: members of at most 64 KiB that carry their own size) is
 * inflated by n_threads threads at once (<= 0: all hardware threads); any other gzip file member after member on one thread. */
int rb_gunzip(const void *src, size_t n, int n_threads, void *dst, size_t cap, size_t *out_len);

/* The same on the GPU: the text is uploaded as it is and lines, records (same rules, same error texts) and the 2-bit
 * encoding + quality mask are found there — no host pass over the bytes, no intermediate buffers.
 * rb_batch_create_fastq: at most 4 GiB of text; final = 0: the text is a piece of a longer input (a last line without an
 * end of line belongs to the next piece); *consumed = where the records that were not complete start.
 * rb_graph_add_fastq = FastqToGraphWorker's loop (R/RNABloom.java:526-643) over a whole file's text: 1 GiB pieces, the
 * next piece is uploaded and parsed while the current one is inserted; *n_records (may be NULL) = records inserted. */
int rb_batch_create_fastq(int device, const char *text, size_t len, int final, int min_base_qual, int use_qual, rb_batch **out, size_t *consumed);
int rb_graph_add_fastq(rb_graph *g, const char *text, size_t len, int min_base_qual, unsigned flags, rb_add_stats *stats, int64_t *n_records);
/* FASTA the same way (FastaReader.next, R/io/FastaReader.java:70-104: trimmed lines, '>' opens a record, the lines after it are joined,
 * an empty line closes it and must be followed by a header — "Incorrect FASTA header format" — or by another empty line, which
 * ends the iteration: *ended; a header that is the very last line is never handed out).  rb_graph_add_fasta = FastaToGraphWorker's
 * loop (R/RNABloom.java:645-732), no quality pass.  A non-final piece leaves its last record unread. */
int rb_batch_create_fasta(int device, const char *text, size_t len, int final, rb_batch **out, size_t *consumed, int *ended);
int rb_graph_add_fasta(rb_graph *g, const char *text, size_t len, unsigned flags, rb_add_stats *stats, int64_t *n_records);
/* The same two worker loops over a FILE, streamed as FastqReader / FastaReader stream theirs (R/io/FastqReader.java:140-186,
 * R/io/FastaReader.java:70-104 over FileUtils.getTextFileReader, R/util/FileUtils.java:50-57: GZIPInputStream for gzip input — detected
 * here by the magic bytes, every member of the file).  Pieces of 256 MiB of text (RB_FASTQ_PIECE): a reader thread reads — and
 * inflates — piece c + 1 into pinned memory, uploads and parses it while the GPU inserts piece c, so the file never sits in memory
 * as a whole and a single-member .gz (which nothing can inflate in parallel) costs max(inflate, insert) instead of their sum. */
int rb_graph_add_fastq_file(rb_graph *g, const char *path, int min_base_qual, unsigned flags, rb_add_stats *stats, int64_t *n_records);
int rb_graph_add_fasta_file(rb_graph *g, const char *path, unsigned flags, rb_add_stats *stats, int64_t *n_records);
/* .nbits files (R/io/NucleotideBitsReader.java, R/util/SeqBitsUtils.java:159-161, 236-263: per sequence a 4-byte
 * big-endian length, then ceil(len/4) bytes of four 2-bit bases each, first base in the top bits, value - 128) straight
 * into a packed device batch: the bytes are uploaded as they are and permuted on the GPU (every base is usable — the
 * format has no code for N).  At most max_reads records (< 0: all); *consumed = bytes used; a truncated last record
 * is left unread, as NucleotideBitsReader.next() returns null for it. */
int rb_batch_create_nbits(int device, const void *bytes, size_t nbytes, int64_t max_reads, rb_batch **out, size_t *consumed);
/* ---- read batches packed in HOST memory ("input already resident in host memory in the build's batch format") ----
 * The build's own batch format, as a host keeps it once its reads are packed (by rb_batch_download_packed, or by a caller's packer):
 *   codes[w] u64: 32 bases, 2 bits each, base i of the word at bits 2i..2i+1 (A C G T = 0 1 2 3);  valid[w] u32: bit i = base i is usable
 *   (ACGTU and quality >= the threshold the reads were packed with);  len[r] u32: read r owns ceil(len[r] / 32) consecutive words.
 * 12 bytes per 32 bases + 4 per read over the link; the device-only columns of a batch are computed on the GPU.  The reader side of
 * FastqToGraphWorker.run (R/RNABloom.java:551-634: reads are fetched while other workers insert) is the packed stream: two device
 * batches taking turns, chunk c + 1 uploading on the stream's own HIP stream while the caller inserts chunk c. */
typedef struct rb_packed_stream rb_packed_stream;
/* pinned host memory (hipHostMalloc): uploads from it run at link speed without a registration pass per call */
int rb_host_alloc(size_t bytes, void **out);
int rb_host_free(void *p);
/* reads [first, first + n) of a device batch in the host format; *n_words = words of those reads (all three arrays NULL: size query) */
int rb_batch_download_packed(const rb_batch *b, int64_t first, int64_t n, uint64_t *codes, uint32_t *valid, uint32_t *len, int64_t *n_words);
/* a stream whose chunks hold at most max_reads reads / max_words words (the two device batches are allocated here, once) */
int rb_packed_stream_create(int device, int64_t max_reads, int64_t max_words, rb_packed_stream **out);
/* start the upload of one chunk and return at once (a helper thread drives the copies); one chunk may be in flight */
int rb_packed_stream_begin(rb_packed_stream *s, const uint64_t *codes, const uint32_t *valid, const uint32_t *len, int64_t n_reads, int64_t n_words);
/* wait for the chunk begun last; *out is a device batch owned by the stream (never rb_batch_destroy it), valid until the begin() after
 * next reuses its buffer.  An error (the lengths do not add up to n_words, a failed copy) is reported here. */
int rb_packed_stream_finish(rb_packed_stream *s, const rb_batch **out);
int rb_packed_stream_destroy(rb_packed_stream *s);
/* FastqToGraphWorker.run over n_reads packed reads in host memory as ONE insert: the lengths go up first (word offsets and owners are computed
 * on the GPU), then codes / valid follow on the handle's copy stream in pieces of piece_reads reads (0: 2^20 reads, doubling up to 2^23) while
 * the insert pipeline already works on the pieces that have arrived — a sub-batch waits only for the pieces its words lie in.  Same filters
 * and statistics as rb_graph_add_batch of the same reads with `flags`; the caller's arrays are free again when the call returns. */
int rb_graph_add_packed(rb_graph *g, const uint64_t *codes, const uint32_t *valid, const uint32_t *len, int64_t n_reads, int64_t n_words,
                        int64_t piece_reads, unsigned flags, rb_add_stats *stats);
/* Start the upload of a packed batch that a later rb_graph_add_packed call with THE SAME arrays and sizes will insert, and return at once (the
 * reader side of stage 1 fetches the next file while the workers insert this one, R/RNABloom.java:7123-7188).  The arrays must stay as they
 * are until that call returns.  Up to two batches may be on their way (uploads run in the order they were started). */
int rb_graph_prefetch_packed(rb_graph *g, const uint64_t *codes, const uint32_t *valid, const uint32_t *len, int64_t n_reads, int64_t n_words,
                             int64_t piece_reads);
/* NucleotideBitsWriter.write R/io/NucleotideBitsWriter.java:24-31 for n_reads sequences; out == NULL: *written = size
 * needed.  A base outside ACGTU is an error (the reference stores a RANDOM base there, SeqBitsUtils.java:154-155). */
int rb_nbits_encode(const char *seq, const int64_t *offsets, int64_t n_reads, void *out, size_t cap, size_t *written);

/* ---- sharded engine (one process per GPU; filters split by index range across `count` shards) ----
 * Multi-GPU counterpart of rb_graph_add_batch.  The reference is a single shared-memory process, so
 * there is no reference interface for this; the phases below are what bench.py / rnabloom.sharded
 * drive, with torch.distributed (RCCL all_to_all / all_gather) moving the byte buffers between
 * ranks.  Shard s of a filter of `size` indices owns [s*span, min(size,(s+1)*span)), span =
 * roundup64(ceil(size/count)); k-mer hash space is split by log2(count) bits of hashVals[0]
 * (bits 40.., uniform even for canonical hashes)
 * (count must be a power of two).  All `dev` pointers are DEVICE pointers owned by the caller
 * (exchange buffers).  Results equal the single-GPU / sequential results bit for bit.
 *
 * per global sub-batch = a range of reads of a batch EVERY rank holds (replicated input: packed reads
 * are 1/38 of the bytes of their (hash, occurrence) records, so the reads travel, not the records):
 *   hash_group  walk all reads of the sub-batch, keep the windows whose k-mer this rank owns and the
 *             no-op prefilter lets through, group them into runs -> Bloom-bit / counter requests
 *             bucketed by filter owner; read-paired k-mers of this rank's 1/count slice of the reads
 *             -> rpkbf bit indices bucketed by owner
 *   [all_to_all requests, pair probes]
 *   serve     owner: bit tests + first-setter arbitration + bit sets, counter claims, pair bit sets
 *   [all_to_all replies back]
 *   resolve   found flags, op counts, counter updates of runs that own their counters alone; the runs that share
 *             a counter and can reach one of theirs ask those counters' owners who else can (RB_SLOT_ORD_IDX)
 *   [all_to_all counter writes + ordered-set questions]     apply_writes, order_serve (claimants per counter)
 *   [all_to_all answers]
 *   order_finish   a run that can reach a contested counter another such run claimed is in the ordered set O* (a superset of the
 *             single-GPU engine's set, without its closure rounds: csrc/rb_shard.hip) -> its (run, contested counter) edges; every
 *             other run is finished in place, its writes to other ranks' counters follow the edges as tagged records
 *   [all_gather edges + tagged writes]      apply_tagged (every rank: the writes that fall into its range)
 *   conflict_route    components of the edge graph (same on every rank); each rank sends its
 *             conflicting runs + their pending occurrence ids to the rank owning the component
 *   [all_to_all runs, ops]
 *   conflict_replay   ordered replay of whole components on a private counter table
 *   [all_to_all final counter bytes]   apply_writes
 *
 * Read-pair filter of a sharded graph: every rank ORs the pairs of its reads into a private full-size copy and the copies are merged into
 * the owners' shards at the end of an insert call; a copy KEEPS its bits afterwards (its seen-pair cache vouches for them) and merges them
 * again with the next call.  Therefore rb_graph_clear and rb_filter_import of RB_RPKBF on a sharded graph are COLLECTIVE: every rank must
 * clear (or import its shard) before any rank inserts again — a rank that does not would OR its old bits back into the peers' freshly
 * cleared or imported shards at the next flush.  (rnabloom.sharded.ShardRank.clear / the Java driver clear all ranks.)
 */
enum {
    RB_SLOT_REC_KEYS = 0,    /* split-reads mode: u64 h0 of the surviving records, bucketed by k-mer owner */
    RB_SLOT_REC_OCC = 1,     /* u32 occurrence ids (same order)          */
    RB_SLOT_PAIR_IDX = 2,    /* u64 global rpkbf bit indices, by owner   */
    RB_SLOT_DREQ_IDX = 3,    /* u64 global dbgbf bit index               */
    RB_SLOT_DREQ_PROBE = 4,  /* u64 (occ_first << 4 | probe)             */
    RB_SLOT_CREQ_IDX = 5,    /* u64 global counter index                 */
    RB_SLOT_W_IDX = 6,       /* u64 global counter index                 */
    RB_SLOT_W_VAL = 7,       /* u8 new byte, 0xFF = just drop the claim  */
    RB_SLOT_CONF_EDGES = 8,  /* 16 B {u64 counter index, u32 run id, u32 0}; run id = local number * count + rank.  Round 6: followed by the counter
                              * writes of the runs finished outside the ordered set, {u64 counter index, u32 0xFFFFFFFF, u32 byte (0xFF: drop the claim)} */
    RB_SLOT_CONF_RUNS = 9,   /* 24 B {u64 h0, u64 counter bytes, u32 component, u32 n_ops | kinds << 28}, by component owner */
    RB_SLOT_CONF_OPS = 10,   /* u32 occurrence ids of those runs, run after run */
    RB_SLOT_CW_IDX = 11,     /* u64 global counter index (replayed components) */
    RB_SLOT_CW_VAL = 12,     /* u8 final byte                            */
    RB_SLOT_Q_BIDX = 13,     /* u64 global bit indices of a query, by owner   */
    RB_SLOT_Q_CIDX = 14,     /* u64 global counter indices of a query, by owner */
    RB_SLOT_CACHE_UPD = 15,  /* split-reads mode: 16 B {u64 h0, u64 exponent} prefilter-cache entries learnt this sub-batch */
    RB_SLOT_ORD_IDX = 16,    /* u64 global counter index: the contested counters of the runs that can reach one (ordered-set question), by owner */
    RB_SLOT_COUNT = 17
};
int rb_graph_create_shard(const rb_graph_params *p, int shard_rank, int shard_count, rb_graph **out);
/* reads [first, first+n) = the global sub-batch (identical arguments on every rank); [pair_first,
 * +pair_n) = the slice of it whose read-paired k-mers this rank walks; ordinal0 = op ordinal of read
 * `first`; flags as rb_graph_add_batch.  counts: requests per destination rank. */
/* ---- split-reads mode (the default from 4 ranks up; rnabloom.sharded picks): every rank hashes only ITS slice
 * of the sub-batch and prefilters it against a REPLICA of the whole prefilter cache; the survivors
 * (12 B records) travel to the k-mer owners; what the owners learn (cache entries) is all-gathered and
 * applied to every replica.  Hashing is then 1/count per rank instead of replicated.
 *   hash   (own slice -> records bucketed by owner, pair probes)   [all_to_all records, pair probes]
 *   group  (received records, source-rank order = read order -> runs -> requests)   [all_to_all requests]
 *   serve / resolve / conflict_* as above; resolve also fills RB_SLOT_CACHE_UPD   [all_gather]   cache_apply */
int rb_shard_set_cache_replication(rb_graph *g, int on);
int rb_shard_hash(rb_graph *g, const rb_batch *b, int64_t first, int64_t n, int64_t own_first, int64_t own_n,
                  uint64_t ordinal0, uint32_t pos_bits, unsigned flags, int64_t *rec_counts /*[count]*/,
                  int64_t *pair_counts /*[count]*/, rb_add_stats *stats);
/* (round 4: the records are grouped where they lie — keys_dev / occ_dev are scratch of the call and hold garbage afterwards) */
int rb_shard_group(rb_graph *g, void *keys_dev, void *occ_dev, int64_t n, uint64_t ordinal0,
                   uint32_t pos_bits, unsigned flags, int64_t *dreq_counts, int64_t *creq_counts);
int rb_shard_cache_apply(rb_graph *g, const void *upd_dev, int64_t n);
/* split reads, look-ahead (k <= 31): the window walk + prefilter of this rank's slice [own_first, own_first + own_n) of the NEXT
 * sub-batch, enqueued on the library's producer stream without waiting for the GPU.  Call it after rb_shard_cache_apply of the current
 * sub-batch; rb_shard_hash with the same arguments then starts from its result.  Any other call in between simply discards it. */
int rb_shard_hash_begin_split(rb_graph *g, const rb_batch *b, int64_t first, int64_t n, int64_t own_first, int64_t own_n,
                              uint64_t ordinal0, uint32_t pos_bits, unsigned flags);
/* optional look-ahead (k <= 31): enqueue the window-hash/prefilter pass of the NEXT sub-batch on the
 * library's producer stream (begin), then its emit + sort + run grouping (emit; waits for the count of
 * kept records only) — both return without waiting for the GPU, so the work overlaps the serve /
 * resolve / conflict phases and the exchanges of the current sub-batch.  rb_shard_hash_group with the
 * same arguments picks the prepared sub-batch up; with different arguments it starts from scratch. */
int rb_shard_hash_begin(rb_graph *g, const rb_batch *b, int64_t first, int64_t n, uint64_t ordinal0, uint32_t pos_bits,
                        unsigned flags);
int rb_shard_hash_emit(rb_graph *g);
int rb_shard_hash_group(rb_graph *g, const rb_batch *b, int64_t first, int64_t n, int64_t pair_first, int64_t pair_n,
                        uint64_t ordinal0, uint32_t pos_bits, unsigned flags, int64_t *dreq_counts /*[count]*/,
                        int64_t *creq_counts /*[count]*/, int64_t *pair_counts /*[count]*/, rb_add_stats *stats);
int rb_shard_serve(rb_graph *g, int mode, const void *dreq_idx_dev, const void *dreq_probe_dev, int64_t nd,
                   const void *creq_idx_dev, int64_t nc, const void *pair_idx_dev, int64_t np,
                   void *dreply_dev /* u8[nd] */, void *creply_dev /* u8[nc] */);
int rb_shard_resolve(rb_graph *g, int mode, const void *dreply_dev, const void *creply_dev, int64_t *w_counts /*[count]*/,
                     int64_t *ord_counts /*[count]: RB_SLOT_ORD_IDX entries per counter owner*/, rb_add_stats *stats);
int rb_shard_order_serve(rb_graph *g, const void *ord_idx_dev, int64_t n, void *reply_dev /* u8[n]: claimants that can reach a contested counter */);
int rb_shard_order_finish(rb_graph *g, int mode, const void *ord_reply_dev /* answers to this rank's RB_SLOT_ORD_IDX, in its order */,
                          int64_t *n_conf_runs, int64_t *n_conf_records /* 16-byte records in RB_SLOT_CONF_EDGES: edges, then tagged writes */, rb_add_stats *stats);
int rb_shard_apply_tagged(rb_graph *g, const void *records_dev /* the gathered RB_SLOT_CONF_EDGES of all ranks */, int64_t n_records);
int rb_shard_apply_writes(rb_graph *g, const void *w_idx_dev, const void *w_val_dev, int64_t n);
/* edges_dev: the edges of ALL ranks (rank order); gid_bound > every run id in them */
int rb_shard_conflict_route(rb_graph *g, const void *edges_dev, int64_t n_edges, int64_t gid_bound, int64_t *run_counts,
                            int64_t *op_counts, rb_add_stats *stats);
int rb_shard_conflict_replay(rb_graph *g, const void *runs_dev, int64_t n_runs, const void *ops_dev, int64_t n_ops,
                             int64_t *w_counts);
/* an internal slot (bucketed by destination): copy it out, or borrow the device pointer (valid until
 * the phase that fills the slot runs again) */
int rb_shard_take(rb_graph *g, int slot, void *dst_dev, int64_t nbytes);
int rb_shard_slot(rb_graph *g, int slot, void **dev_ptr, int64_t *nbytes);
int rb_shard_span(rb_graph *g, int which, int64_t *span, int64_t *lo, int64_t *hi);
/* queries on a sharded graph (BloomFilter.lookup R/bloom/BloomFilter.java:139-147,
 * CountingBloomFilter.getCount :196-210, BloomFilterDeBruijnGraph.getCount :562-570) for hashes any
 * rank holds: make (indices bucketed by owner: slots Q_BIDX / Q_CIDX) -> [all_to_all] -> serve (bit /
 * counter byte per index) -> [all_to_all back] -> finish.  what: 0 = lookup in bit filter
 * `which_bits` (RB_DBGBF / RB_RPKBF), 1 = counting-filter count, 2 = graph count (count + 1, or 0 unless in dbgbf). */
int rb_shard_query_make(rb_graph *g, int what, int which_bits, const uint64_t *h0_host, size_t n, int64_t *bit_counts,
                        int64_t *ctr_counts);
int rb_shard_query_serve(rb_graph *g, int which_bits, const void *bidx_dev, int64_t nb, const void *cidx_dev, int64_t nc,
                         void *breply_dev /* u8[nb] */, void *creply_dev /* u8[nc] */);
int rb_shard_query_finish(rb_graph *g, int which_bits, const void *breply_dev, const void *creply_dev,
                          uint8_t *out8_host /* what 0 */, float *outf_host /* what 1, 2 */);

/* ---- graph traversal on a sharded graph: rb_graph_walk / rb_graph_greedy_extend / rb_graph_naive_extend when no GPU holds the
 * filters (BASELINE configs[3]: stage 2's inner loops, R/util/GraphUtils.java:1591-1675, :1906-1996, :6780-7112, over
 * Kmer.getSuccessors / getPredecessors R/graph/Kmer.java:199-355).  Every rank drives its own walks with the SAME kernels the
 * single-GPU calls run; the counts they need come from the owners of the filter ranges through the query exchange above:
 *   begin (this rank's seeds; may be none) -> repeat { advance -> [all_to_all of slots Q_BIDX / Q_CIDX] -> rb_shard_query_serve ->
 *   [all_to_all back] -> absorb } until no rank reports an active walk -> end.
 * advance runs every walk up to the next neighbourhood whose counts it has not been told (a walk suspends at the start of its
 * current step and replays it from there when the answers are in: the step's earlier questions are then cache hits), files the
 * requests — the four neighbours of a k-mer go out together, a naive extension's back-branch variants with them — and makes the
 * query for them (bit_counts / ctr_counts per destination rank, as rb_shard_query_make).  One exchange round per step for the
 * max-coverage walk and the naive extension, one per level of the lookahead search for the greedy extension.
 * kind 0 = rb_graph_walk (targets may be NULL), 1 = rb_graph_greedy_extend (mode_or_lookahead = lookahead; gate: rb_shard_trav_set_gate),
 * 2 = rb_graph_naive_extend (mode_or_lookahead = mode; term_seq / term_off for mode 0); the other arguments, the
 * outputs and the reasons are those calls'.  answer_cap: counts one step of a walk may hold (0: 4, 8, or
 * 4 (1 + 4 (1 + 2 lookahead)) by kind); a greedy step whose search needs more ends the walk with reason 8.  Results equal the
 * single-GPU calls on the same filters (tests/test_gpu_sharded_walks.py). */
int rb_shard_trav_begin(rb_graph *g, int kind, const char *seeds, const char *targets, size_t n, int direction, int mode_or_lookahead,
                        int bound, int cap, float min_cov, const char *term_seq, const int64_t *term_off, int answer_cap);
/* the `bf` variants of the greedy extension (R/util/GraphUtils.java:1978-1993, Kmer.getSuccessors(k, numHash, graph, bf)
 * R/graph/Kmer.java:257-299): gate = this rank's shard handle of ANOTHER sharded graph (same k, strandedness, rank count) whose dbgbf is
 * that filter.  Call after begin; every round then carries a second request: advance also fills slot Q_BIDX of the GATE handle
 * (gate_bit_counts per destination rank) with the same k-mers as a lookup, to be exchanged, served by rb_shard_query_serve on the
 * owners' gate handles and handed to absorb as gate_breply_dev.  A k-mer that fails the gate counts 0. */
int rb_shard_trav_set_gate(rb_graph *g, rb_graph *gate);
int rb_shard_trav_advance(rb_graph *g, int64_t *n_active, int64_t *bit_counts, int64_t *ctr_counts, int64_t *gate_bit_counts /* NULL without a gate */);
int rb_shard_trav_absorb(rb_graph *g, const void *breply_dev, const void *creply_dev, const void *gate_breply_dev /* NULL without a gate */);
/* out_f: kinds 0 and 2 (forward hashes of the appended k-mers), out_r and out_count: kind 0, out_count: kinds 0 and 1; each may be
 * NULL.  rounds (may be NULL): exchange rounds this rank's walks took.  Frees the traversal. */
int rb_shard_trav_end(rb_graph *g, char *out_bases, uint64_t *out_f, uint64_t *out_r, float *out_count, int32_t *out_len,
                      uint8_t *out_reason, int64_t *rounds);

/* development: milliseconds for 2 x 2^28 random returning atomics on the counting filter where it lies (mode 0: OR with 0, 1: XOR pairs that
 * restore the contents) — tools/alloc_lottery.py looks for what the probe stages' allocation-dependent time follows */
int rb_debug_probe_cbf(rb_graph *g, int mode, float *ms_out);
/* development / tests: the library's own device-wide primitives (csrc/rb_sort.hip, csrc/rb_group.hip; rocPRIM until round 3) on
 * host arrays.  rb_debug_scan_u32: out[i] = in[0] + ... + in[i-1] (wrapping); the device copies start
 * (misalign & 3) [input] and (misalign >> 2) [output] words past a 16-byte boundary (0: both aligned — the vectorised path).  rb_debug_sort_pairs: stable sort of (key, value) on key bits [lo_begin, lo_end) then [hi_begin, hi_end)
 * (hi_begin < 0: one range); vals may be NULL (keys only), vals64 != 0: 64-bit values. */
int rb_debug_scan_u32(int device, const uint32_t *in, size_t n, uint32_t *out, int misalign);
int rb_debug_sort_pairs(int device, uint64_t *keys, void *vals, int vals64, size_t n, int lo_begin, int lo_end, int hi_begin, int hi_end);
/* development / tests: the grouping stage of the insert pipeline (csrc/rb_group.hip) on host arrays, called the way an insert calls it.
 * In: n > 0 records (keys[i], vals[i]) = (base hash, occurrence id); group_bits, bucket_target (0: default) and flags (1: records with
 * key and value all ones are cancelled ones) as an insert passes them; seed, ordinal0, pos_bits of the strength draws; idx_span != 0:
 * partition keyed by the filter index ((key >> 1) % idx_size, indices [idx_lo, idx_lo + idx_span)), else by the hash bits.
 * Out, n entries each: vals_out (occurrences in grouped order; the first info[9] are written), tz_out (their strengths), and the runs
 * uniq / counts / starts (the first info[7] are written; the rest reads 0).  brun / bnr (both or neither; room for 2^20 entries, the
 * first 2^T are written): per fine bucket the first run slot and the number of runs, as the swept Bloom-bit stage gets them.
 * info[12]: 0 T (partition bits), 1 t_hi, 2 t_lo (first / second partition pass), 3 l_hi, 4 l_lo (locally sorted bits below them),
 * 5 the fix level in force, 6 index-keyed (0 / 1), 7 runs, 8 runs before the oversized buckets' (-1 without brun), 9 live records,
 * 10 oversized buckets, 11 records of the largest of them.  The RB_GROUP_* environment switches are read on every call. */
int rb_debug_group(int device, const uint64_t *keys, const uint32_t *vals, size_t n, int group_bits, int bucket_target, unsigned flags,
                   uint64_t seed, uint64_t ordinal0, uint32_t pos_bits, uint64_t idx_size, uint64_t idx_lo, uint64_t idx_span,
                   uint32_t *vals_out, uint8_t *tz_out, uint64_t *uniq, uint32_t *counts, uint32_t *starts, uint32_t *brun, uint32_t *bnr,
                   int64_t *info);
/* development / tests: the selection primitives (csrc/rb_sort.hip).  out_a = the indices i in [0, n) with (status[i] & mask_a) != 0, in
 * order, counts[0] of them; mask_b != 0: the same for mask_b into out_b / counts[1] in the same two passes (mask_b == 0: the one-list
 * call, out_b may be NULL, counts[1] = 0).  out_a / out_b have room for n entries. */
int rb_debug_select(int device, const uint32_t *status, size_t n, uint32_t mask_a, uint32_t mask_b, uint32_t *out_a, uint32_t *out_b,
                    uint32_t *counts);
/* development / tests: the no-op prefilter (step 1 of an insert) and its hot-k-mer cache, for tests/test_gpu_prefilter.py.
 * rb_debug_cache_export: the handle's cache table to the host as it stands.  which = 0: the minimizer-bucketed table (*log2 = log2 of the
 * number of buckets, 16 words each; *m = minimizer length), 1: the hash-bucketed table (*log2 = log2 of the number of words, 8 per bucket;
 * *m = 0).  out == NULL: geometry only (the size query); else cap_words >= the table's words.  Fails when the handle has no such table.
 * rb_debug_prefilter: the window walk of an insert over words [first_word, first_word + n_words) of the batch — whole reads — as add_range
 * would dispatch it now (same cache choice, same walker, the RB_FILTER_PIPE / RB_READ_LANES / RB_RAGGED_LANES / RB_NO_MPF switches as read on
 * every call), forward or canonical hashing by the handle's strandedness, draws from (the handle's seed, ordinal0 + read - first read of the range,
 * window start).  cnt_out / mask_out, n_words entries each: kept windows and their bit mask per word (the word a window starts in).  Nothing
 * is inserted; filters, cache and op ordinal stay as they are.  Both calls are synchronous. */
int rb_debug_cache_export(rb_graph *g, int which, uint64_t *out, size_t cap_words, uint32_t *log2, uint32_t *m);
int rb_debug_prefilter(rb_graph *g, const rb_batch *b, int64_t first_word, int64_t n_words, uint64_t ordinal0, uint32_t pos_bits,
                       uint32_t *cnt_out, uint32_t *mask_out);

/* ---- the exchange driver below the C ABI (csrc/rb_comm.hip) ----
 * rb_shard_add_range = rnabloom/sharded.py::ShardRank.add_range in the library: all sub-batches of reads [first, first + n)
 * (the same call on every rank, every rank holding the same batch), every phase above and every exchange between them, on the
 * handle's stream — nothing but per-peer byte counts visits the host, no interpreter between the phases.  ordinal0 = reads
 * inserted since the last clear (the op ordinal of read `first`).  The communicator is either
 *   RCCL (one process per GPU): rank 0 calls rb_shard_comm_unique_id, the 128 bytes travel to the other ranks by whatever the
 *     host has (torch.distributed broadcast, MPI, a file), every rank calls rb_shard_comm_create_rccl; transfers are
 *     ncclSend / ncclRecv groups in pieces of at most 256 MiB per peer (librccl.so is loaded with dlopen on first use), or
 *   a loopback hub for `world` virtual ranks of ONE process on one GPU (one host thread per rank calls rb_shard_add_range with
 *     the same hub; device-to-device copies): what the one-GPU tests drive the protocol with. */
typedef struct rb_shard_comm rb_shard_comm;
int rb_shard_comm_unique_id(void *out128);
int rb_shard_comm_create_rccl(const void *id128, int rank, int world, int device, rb_shard_comm **out);
int rb_shard_comm_create_loopback(int world, rb_shard_comm **out);
/* Read-pair filter of a sharded graph, replicated accumulation (round 4): rpkbf.add is a pure OR (R/bloom/BloomFilter.java:133-137),
 * so while a file is inserted every rank ORs the pairs of its reads into a private full-size copy and the copies are merged into the
 * owners' index ranges when the call ends: begin() hands out this rank's copy as ONE send buffer cut into `shard_count` consecutive
 * pieces (counts[r] = bytes of rank r's range; all zero when the handle uses the routed path, RB_SHARD_PAIRS=route), the caller does
 * the all-to-all, end() ORs the G received pieces (each the size of this rank's range) into the shard and clears the copy.  Every rank
 * calls both at the end of every collective insert call (rb_shard_add_range and rnabloom/sharded.py::ShardRank.add_range do). */
int rb_shard_pairs_flush_begin(rb_graph *g, void **send_dev, int64_t *counts);
int rb_shard_pairs_flush_end(rb_graph *g, const void *recv_dev, const int64_t *recv_counts);
/* a small all-to-all and all-gather of known bytes through the communicator's own transport, checked on arrival (every rank calls it;
 * big_bytes is added to every message: > 256 MiB exercises the piece-wise path).  bench.py runs it before the first step. */
int rb_shard_comm_selftest(rb_shard_comm *c, int rank, int device, int64_t big_bytes);
int rb_shard_comm_destroy(rb_shard_comm *c);
int rb_shard_add_range(rb_graph *g, rb_shard_comm *c, const rb_batch *b, int64_t first, int64_t n, unsigned flags,
                       int64_t reads_per_substep, uint32_t pos_bits, uint64_t ordinal0, rb_add_stats *stats);

/* ---- instrumentation: per-kernel-class HIP-event timing on the library's own stream ---- */
#define RB_PROF_MAX 32
typedef struct rb_profile {
    int32_t n;
    const char *name[RB_PROF_MAX];
    double ms[RB_PROF_MAX];        /* accumulated since last reset */
    int64_t launches[RB_PROF_MAX];
} rb_profile;
int rb_graph_profile_enable(rb_graph *g, int on);
int rb_graph_profile_get(rb_graph *g, rb_profile *out, int reset);

#ifdef __cplusplus
}
#endif
#endif
