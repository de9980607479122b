package rnabloom.graph;

import java.nio.ByteBuffer;

/**
 * JNI surface of librb_hip.so (include/rb_capi.h): one static native method per C entry point a single-process host
 * needs.  Handles are the rb_graph / rb_batch pointers as long.  Large inputs (reads, filter bytes) travel in DIRECT
 * ByteBuffers; hash / result arrays are primitive arrays.  Every method throws (IllegalArgumentException,
 * IllegalStateException, OutOfMemoryError or RuntimeException carrying rb_last_error()) instead of returning a status.
 *
 * BloomFilterDeBruijnGraph keeps its public signature (src/rnabloom/graph/BloomFilterDeBruijnGraph.java:75-104,
 * 405-461, 534-590) and forwards to these methods; only hashVals[0] crosses the boundary — the library re-derives
 * hashVals[1..] with NTM64 (src/rnabloom/bloom/hash/NTHash.java:518-527) from the graph's k.
 * The multi-GPU phases (rb_shard_*) are driven by one process per GPU and are not part of this class.
 */
public final class NativeGraph {
    static { System.loadLibrary("rb_jni"); }          // librb_jni.so links librb_hip.so

    private NativeGraph() { }

    /** HIP device the drop-in classes create their handles on: -Drb.device=N (default 0) */
    public static int defaultDevice() { return Integer.getInteger("rb.device", 0); }

    // filters (RB_DBGBF .. RB_FPKBF), add flags (RB_ADD_*), per-hash ops (RB_OP_*), neighbour directions
    public static final int DBGBF = 0, CBF = 1, RPKBF = 2, FPKBF = 3;
    public static final int ADD_REVCOMP = 1, ADD_COUNT_IF_PRESENT = 2, ADD_STORE_READ_PAIRS = 4, ADD_PAIRS_IF_PRESENT = 8;
    public static final int OP_ADD = 0, OP_ADD_IF_ABSENT = 1, OP_ADD_COUNT_IF_PRESENT = 2, OP_ADD_DBG_ONLY = 3,
            OP_ADD_COUNT_ONLY = 4, OP_ADD_READ_PAIR = 5, OP_ADD_FRAG_PAIR = 6;
    public static final int SUCCESSORS = 0, PREDECESSORS = 1, LEFT_VARIANTS = 2, RIGHT_VARIANTS = 3;
    public static final int STROBE_CANONICAL = 1, STROBE_SLIDE = 2;

    // ---- graph lifetime ----
    public static native int version();
    public static native long create(long dbgbfNumBits, long cbfNumBytes, long pkbfNumBits, int dbgbfNumHash, int cbfNumHash,
                                     int pkbfNumHash, int k, boolean stranded, boolean useReadPairedKmers, int device, long rngSeed);
    public static native void destroy(long h);
    public static native void clear(long h, int whichMask);
    public static native void destroyFilter(long h, int which);
    public static native void setReadPairedKmerDistance(long h, int d);
    public static native void setFragPairedKmerDistance(long h, int d);
    public static native void initFragmentPairs(long h, long pkbfNumBits, int pkbfNumHash);
    public static native long getOpOrdinal(long h);
    public static native void setOpOrdinal(long h, long v);

    // ---- read batches resident on the device ----
    /** seq / qual (qual may be null): direct buffers of concatenated reads; offsets[nReads + 1]. */
    public static native long batchCreateAscii(int device, ByteBuffer seq, ByteBuffer qual, long[] offsets, int nReads, int minBaseQual);
    /** .nbits bytes (NucleotideBitsWriter format) -> batch; consumed[0] receives the number of bytes used. */
    public static native long batchCreateNbits(int device, ByteBuffer bytes, long nBytes, long maxReads, long[] consumed);
    public static native void batchDestroy(long b);
    /** {reads, bases, device bytes} */
    public static native long[] batchInfo(long b);

    // ---- reads packed in HOST memory (the build's batch format: codes 8 B + valid 4 B per 32 bases, len 4 B per read; little endian) ----
    /** pinned host memory as a direct buffer: uploads from it run at link speed.  Free with hostFree — the collector does not own it. */
    public static native ByteBuffer hostAlloc(long bytes);
    public static native void hostFree(ByteBuffer buf);
    /** reads [first, first + n) of a device batch into direct buffers; returns their word count (all buffers null: size query) */
    public static native long batchDownloadPacked(long b, long first, long n, ByteBuffer codes, ByteBuffer valid, ByteBuffer len);
    /** two device batches taking turns: begin() starts the upload of a chunk and returns, finish() waits and returns a BORROWED batch handle
     *  (addBatch it, never batchDestroy it) that stays valid until the begin() after next */
    public static native long packedStreamCreate(int device, long maxReads, long maxWords);
    public static native void packedStreamBegin(long s, ByteBuffer codes, ByteBuffer valid, ByteBuffer len, long wordOffset, long readOffset, long nReads, long nWords);
    public static native long packedStreamFinish(long s);
    public static native void packedStreamDestroy(long s);
    /** FastqToGraphWorker's loop over reads already packed in host memory: ONE insert; the input goes up in pieces of pieceReads reads (0: 2^20 doubling to 2^23) on a copy stream while the pipeline works on what has arrived */
    public static native long[] addPacked(long h, ByteBuffer codes, ByteBuffer valid, ByteBuffer len, long nReads, long nWords, long pieceReads, int flags);

    /** start the upload of a packed batch the next addPacked with the same buffers and sizes inserts; returns at once (the buffers must stay untouched until then) */
    public static native void prefetchPacked(long h, ByteBuffer codes, ByteBuffer valid, ByteBuffer len, long nReads, long nWords, long pieceReads);

    // ---- stage-1 inserts; every add returns {reads, kmers, pairs, distinct, conflictOps, sortedKmers} ----
    public static native long[] addBatch(long h, long batch, long first, long n, int flags);
    public static native long[] addPairs(long h, long batch, long first, long n, int which, int flags);
    public static native long[] addFragments(long h, long batch, long first, long n, boolean loadPairedKmers);
    public static native long[] addReads(long h, ByteBuffer seq, ByteBuffer qual, long[] offsets, int nReads, int minBaseQual, int flags);
    public static native void apply(long h, int op, long[] baseHashes, int n);

    // ---- queries (may be called from many threads on one handle) ----
    public static native void contains(long h, long[] baseHashes, int n, byte[] out);
    public static native void getCount(long h, long[] baseHashes, int n, float[] out);
    public static native void filterLookup(long h, int which, long[] baseHashes, int n, byte[] out);
    public static native void filterLookupThenAdd(long h, int which, long[] baseHashes, int n, byte[] out);
    public static native void filterGetCount(long h, long[] baseHashes, int n, float[] out);
    public static native void filterIncrementAndGet(long h, long[] baseHashes, int n, float[] out);
    /** Counts of getKmers for reads [first, first + n) of a resident batch (one float per window, no hashes): packed rows at koffsets[i]
     *  (koffsets[n + 1], koffsets[0] = 0), or — koffsets == null — rows of the returned stride (longest read - k + 1), zero-padded.
     *  Call with n = 0 to learn the stride before allocating `out`. */
    public static native long batchCounts(long h, long batch, long first, long n, long[] koffsets, float[] out);
    /** Coverage statistics of the count profile of reads [first, first + n) of a resident batch (rb_graph_read_coverage): segments READS (0)
     *  or WINDOWS (1, windowSize = window); mates != 0 (READS only): a batch whose read mateFirst + i is read first + i's mate.  out holds
     *  12 ints per record (n, nSolid, nComplex, flags, then min q1 median q3 max dropoff seThreshold peThreshold as raw float bits);
     *  out == null fills segOffsets[n + 1] only.  Returns the number of records. */
    public static native long readCoverage(long h, long batch, long first, long n, long mates, long mateFirst, int segments, int window,
                                           int lookahead, float maxCovGradient, float covFPR, float minKmerCov, long[] segOffsets, int[] out);
    /** Paired-k-mer segments of n sequences (rb_graph_paired_kmer_segments; GraphUtils.breakWithReadPairedKmers / breakWithFragPairedKmers,
     *  R/util/GraphUtils.java:4184-4405): which = RPKBF (2) or FPKBF (3); ranges = null for whole k-mer lists, else 2n ints [rangeStart,
     *  rangeEnd).  segOffsets[n + 1] is filled from the lengths alone; segment j of sequence i is segs[2 * (segOffsets[i] + j)] .. + 1
     *  ([start, end) in k-mer indices) for j < nSegs[i].  segs == null sizes the outputs only.  support (with koffsets[n + 1]): one byte per
     *  k-mer, 1 where the pair at that position is in the filter.  Returns the number of segment slots. */
    public static native long pairedKmerSegments(long h, int which, ByteBuffer seq, long[] offsets, int n, int numPairsRequired, int[] ranges,
                                                 long[] segOffsets, int[] segs, int[] nSegs, byte[] support, long[] koffsets);
    /** Mismatch correction of n sequences (rb_graph_correct_mismatches; GraphUtils.correctMismatches, R/util/GraphUtils.java:3914-3996):
     *  covThreshold[n] one threshold per sequence, outSeq a direct buffer with seq's layout that receives the corrected bases, nFixed[n]
     *  the number of replacements per sequence.  koffsets[n + 1] (optional) and counts (optional, with koffsets: one float per k-mer at
     *  koffsets[i] + p) return the final count profile — getKmers of the corrected sequences. */
    public static native void correctMismatches(long h, ByteBuffer seq, long[] offsets, int n, float[] covThreshold, float minKmerCov,
                                                ByteBuffer outSeq, int[] nFixed, long[] koffsets, float[] counts);
    /** Error correction of n sequences (rb_graph_correct_errors; GraphUtils.correctErrorHelper, R/util/GraphUtils.java:3711-3912): gap repair
     *  and the mismatch pass on the device.  outOffsets[n + 1] is filled from the lengths and maxIndelSize alone; outSeq == null sizes the
     *  outputs only (gapOffsets, if given, then holds the capacity layout of the gap records).  Else corrected sequence i is outLen[i] bytes at
     *  outSeq + outOffsets[i], flags[i] has bit 0 corrected (the reference returns non-null), bit 1 a gap was replaced or trimmed, bit 2 the
     *  mismatch pass replaced a base.  gaps (optional, with gapOffsets[n + 1]): 5 ints per gap — sequence, first bad k-mer, run length,
     *  replacement length, kind | outcome << 8 (kind 0 left edge, 1 right edge, 2 SNV, 3 path; outcome 0 kept, 1 replaced, 2 trimmed) —
     *  those of sequence i at gaps[5 * gapOffsets[i]] .. gaps[5 * gapOffsets[i + 1]).  Returns outOffsets[n]; IllegalArgumentException
     *  when that is more than an int holds (cut the batch). */
    public static native int correctErrors(long h, ByteBuffer seq, long[] offsets, int n, float[] covThreshold, int lookahead, int maxIndelSize,
                                           float percentIdentity, float minKmerCov, long[] outOffsets, ByteBuffer outSeq, int[] outLen, int[] flags,
                                           int[] gaps, long[] gapOffsets);
    /** Overlap of n read pairs (rb_graph_overlap_pairs; GraphUtils.overlap, R/util/GraphUtils.java:4898-5063): pair i is lseq[loffsets[i],
     *  loffsets[i + 1]) and rseq[roffsets[i], roffsets[i + 1]).  outOffsets[n + 1] is filled from the lengths alone (room for both reads);
     *  outSeq == null sizes the output only.  Else recs holds 8 ints per pair — outcome (0 none, 1 left's k-mers, 2 right's k-mers, 3 merged,
     *  4 spanned, 5 the reference would rescue the pair: lines :5018-5056 are the caller's), why (0 found, 1 no match, 2 no complex k-mer,
     *  3 no singleton in the right read, 4 none in the left read, 5 the shared bases are a repeat, 6 a read shorter than max(k, minOverlap),
     *  7 the reference's isRepeat throws), flags (bit 0: the reads changed roles), bases overlapped, length of the text, first spanning
     *  window and number of spanning windows of that text, 0 — and the string the returned k-mers spell is recs[8 i + 4] bytes at outSeq +
     *  outOffsets[i].  Read-only.  Returns outOffsets[n]; IllegalArgumentException when that is more than an int holds (cut the batch). */
    public static native int overlapPairs(long h, ByteBuffer lseq, long[] loffsets, ByteBuffer rseq, long[] roffsets, int n, int minOverlap,
                                          float minKmerCov, long[] outOffsets, ByteBuffer outSeq, int[] recs);
    /** Paired-k-mer branch extension of n sequences (rb_graph_extend_se; GraphUtils.extendRightSE / extendLeftSE, R/util/GraphUtils.java:6018-6204):
     *  sequence i is seq[offsets[i], offsets[i + 1]) in its natural orientation with the floor minKmerCov[i]; direction 0 extends to the right,
     *  1 to the left.  recs holds 8 ints per sequence — outcome (0 none: the reference returns null, 1 the only candidate and its walk, 2 a
     *  first-level winner, 3 a second-level winner), why (0 found, 1 no candidate, 2 no candidate was supported, 3 the last k-mer holds a letter
     *  outside ACGTU, 4 shorter than k), candidates, k-mers returned, supporting pairs, last partnered k-mer, winner (candidate base, second base in
     *  bits 4..5), Float.floatToRawIntBits(score) — and the bases the returned k-mers add are recs[8 i + 3] bytes at outBases + i * (d + 2), in
     *  walking order; outCount (may be null) their counts.  Read-only. */
    public static native void extendSE(long h, ByteBuffer seq, long[] offsets, int n, int direction, float[] minKmerCov, byte[] outBases,
                                       float[] outCount, int[] recs);
    /** Fragment-paired branch extension of n sequences (rb_graph_extend_pe; GraphUtils.extendRightPE / extendLeftPE, R/util/GraphUtils.java:6206-6414):
     *  arguments as extendSE.  recs holds 10 ints per sequence — outcome, why (as extendSE; 5: the reference's isRepeat throws on a k-mer of the
     *  repeat scan), candidates, k-mers returned, supporting read pairs, supporting fragment pairs, last partnered k-mer, winner,
     *  Float.floatToRawIntBits(score), the bound the first-level walks ran with — and the bases the returned k-mers add are recs[10 i + 3] bytes
     *  at outBases + i * (fragD + 2), in walking order; outCount (may be null) their counts.  Read-only. */
    public static native void extendPE(long h, ByteBuffer seq, long[] offsets, int n, int direction, float[] minKmerCov, byte[] outBases,
                                       float[] outCount, int[] recs);
    /** Joining of n read pairs through the graph (rb_graph_join_pairs; GraphUtils.join, R/util/GraphUtils.java:892-1147): pair i is lseq[loffsets[i],
     *  loffsets[i + 1]) and rseq[roffsets[i], roffsets[i + 1]).  outOffsets[n + 1] is filled from the lengths, bound, d and k alone; outSeq == null
     *  sizes the output only.  Else recs holds 12 ints per pair — outcome (0 none: the reference returns null, 1 joined, 2 not judged), why
     *  (0 the left walk reached the right read's first k-mer, 1 a k-mer inside the right read, 2 the right walk reached the left read's last
     *  k-mer, 3 a k-mer of the left path, 4 the right walk met a loop or a homopolymer, 5 both walks ended, 6 a read shorter than k, 7 a letter
     *  outside ACGTU), how the left and the right walk ended (0 not run, 1 no neighbour, 2 loop or homopolymer, 3 the branch step returned
     *  nothing, 4 a homopolymer inside a step's k-mers, 5 bound reached, 6 returned), k-mers added by each, branch steps taken by each, the
     *  index of the meeting k-mer (-1: none), the length of the text, Float.floatToRawIntBits of the two walks' final thresholds — and the
     *  string the returned k-mers spell is recs[12 i + 9] bytes at outSeq + outOffsets[i].  maxTipLen is not read (the branch step does not
     *  read it).  Read-only.  Returns outOffsets[n]; IllegalArgumentException when that is more than an int holds (cut the batch). */
    public static native int joinPairs(long h, ByteBuffer lseq, long[] loffsets, ByteBuffer rseq, long[] roffsets, int n, int bound,
                                       float maxCovGradient, int maxTipLen, float minKmerCov, long[] outOffsets, ByteBuffer outSeq, int[] recs);
    /** The extension loop of n fragments on the device (rb_graph_extend_loop; GraphUtils.extendSE, which = 0, and extendPE, which = 1,
     *  R/util/GraphUtils.java:6454-6678): every sequence — upper-case A C G T, at least k letters — is extended to the left and then to the right,
     *  round after round, until the step returns nothing at the lowest floor or only k-mers the sequence already holds.  room (at least the loop's
     *  distance + 2) is the most letters a call adds on each side; outOffsets[n + 1] is filled with the capacity layout length + 2 room; outSeq ==
     *  null sizes the output only.  Else recs holds 16 ints per sequence — status (0 done, 1 out of room: call again with the returned text and
     *  phase 0 after a left end 4, phase 1 after a right end 4; 2 not judged: keep the host loop for it), why (1 fewer than k letters, 2 a letter
     *  other than upper-case A C G T), k-mers added left and right, the length of the text, how the left and the right side ended (0 not run, 1
     *  nothing found, 2 only known k-mers and the list shorter than the distance, 3 a duplicated k-mer pair, 4 out of room), rounds left and right,
     *  steps, floor drops, rounds of known k-mers that went on, the bits of both sides' last floors (Float.intBitsToFloat), 0, 0 — and the text is
     *  recs[16 i + 4] bytes at outSeq + outOffsets[i].  phase (may be null: all 0): 0 both sides, 1 the right side only.  Read-only.  Returns
     *  outOffsets[n]; IllegalArgumentException when that is more than an int holds (cut the batch). */
    public static native int extendLoop(long h, int which, ByteBuffer seq, long[] offsets, int n, byte[] phase, float minKmerCov, int room,
                                        long[] outOffsets, ByteBuffer outSeq, int[] recs);
    /** Naive extension of n fragments on the device (rb_graph_naive_extend_fragments; GraphUtils.naiveExtend(kmers, graph, maxTipLength, minKmerCov),
     *  R/util/GraphUtils.java:6935-6957): every sequence — upper-case A C G T, at least k letters — is walked to the left from its first k-mer with
     *  its own k-mers as terminators, then to the right from its last k-mer with its k-mers and the left extension as terminators.  room (1 .. 2^24)
     *  is the most letters a call adds on each side; outOffsets[n + 1] is filled with the capacity layout length + 2 room; outSeq == null sizes the
     *  output only.  Else recs holds 16 ints per sequence — status (0 done, 1 out of room: call again with the returned text and phase 0 after a left
     *  end 5, phase 1 after a right end 5; 2 not judged), why (1 fewer than k letters, 2 a letter other than upper-case A C G T), k-mers added left
     *  and right, the length of the text, how the left and the right walk ended (0 not run, 1 no neighbour, 2 a back branch, 3 several neighbours, 4
     *  the candidate is a k-mer of the text, 5 out of room), for an end 4 the lowest index of that k-mer in the returned text's k-mer list on either
     *  side (else -1), seven zeros — and the text is recs[16 i + 4] bytes at outSeq + outOffsets[i].  phase (may be null: all 0): 0 both walks, 1
     *  the right one only.  Read-only.  Returns outOffsets[n]; IllegalArgumentException when that is more than an int holds (cut the batch). */
    public static native int naiveExtendFragments(long h, ByteBuffer seq, long[] offsets, int n, byte[] phase, float minKmerCov, int room,
                                                  long[] outOffsets, ByteBuffer outSeq, int[] recs);
    /** Connection of the segment lists of n reads through the graph (rb_graph_connect_segments; GraphUtils.connect(ArrayList, graph, lookahead),
     *  R/util/GraphUtils.java:4836-4872): read i owns list entries [readSegs[i], readSegs[i + 1]), entry j is seq[segOffsets[j], segOffsets[j + 1]);
     *  entries with an odd index within a read are placeholders read by length only.  outOffsets[n + 1] is filled from the lengths alone; outSeq ==
     *  null sizes the output only.  Else recs holds 8 ints per read — outcome (0 empty, 1 single, 2 chained, 3 not judged), why (1 an even number of
     *  entries, 2 a segment shorter than k, 3 a letter outside ACGTU), gaps, gaps connected, the list indices of the returned run's first and last
     *  segment, the length of the text, 0 — and the returned string is recs[8 i + 6] bytes at outSeq + outOffsets[i].  gapRecs (may be null) holds 8
     *  ints per odd entry in list order: connected, how (0 not run, 1 the left walk arrived, 2 the right walk arrived, 3 the paths meet, 4 they meet
     *  in a low-complexity k-mer, 5 the right walk looped, 6 both walks ended), how each walk ended (0 not run, 1 no neighbour, 2 loop, 3 bound, 4
     *  arrived, 5 met the left path), k-mers added by each, the left-path index of the meeting (-1: none), the k-mers of the path.  lookahead is not
     *  read.  Read-only.  Returns outOffsets[n]; IllegalArgumentException when that is more than an int holds (cut the batch). */
    public static native int connectSegments(long h, ByteBuffer seq, long[] segOffsets, long[] readSegs, int n, int lookahead, float minKmerCov,
                                             long[] outOffsets, ByteBuffer outSeq, int[] recs, int[] gapRecs);
    /** The fragment screens of n sequences (rb_graph_screen_fragments; GraphUtils.isBranchFree, isChimera and isBluntEndArtifact,
     *  R/util/GraphUtils.java:7651-7672, :7674-7760, :8535-8586): what = 1 branch-free | 2 chimera | 4 blunt-end artifact; gateHandleOr0 is the
     *  handle whose dbgbf is the BloomFilter assembledKmers (0 only for what == 1); maxDepth is maxEdgeClipLength; maxVisits the budget of one
     *  static hasDepth* search (0: the library's default).  recs holds 8 ints per sequence — flags (the predicates in bits 0..2; not judged:
     *  8 a letter outside ACGTU, 16 no k-mer, 32 a depth search ran out of its budget), chim_why, isChimera's i and j, the lengths of its two
     *  greedy walks, blunt_why, the arm's boundary index.  Read-only on both handles. */
    public static native void screenFragments(long h, long gateHandleOr0, ByteBuffer seq, long[] offsets, int n, int what, int lookahead,
                                              int maxDepth, long maxVisits, int[] recs);
    /** GraphUtils.represented (rb_graph_represented; R/util/GraphUtils.java:711-824) of n sequences: gateHandle is the handle whose dbgbf is the
     *  worker's screeningBf (required); maxVisits the budget of one static hasDepth* search (0: the library's default).  recs holds 12 ints
     *  per sequence — flags (bit 0: represented; not judged: 8 a letter outside ACGTU, 16 no k-mer, 32 a depth search ran out of its budget),
     *  why (the line that returned: 0 true, 1 no run of assembled k-mers, 2 / 3 the left edge's length / identity, 4 a gap wider than d + k,
     *  5 no path, 6 / 7 the path's length / identity, 8 / 9 the right edge's length / identity), the deciding test's left, right, expected
     *  length, found length and distance (-1 where there is none), the tests passed before it, the sum of their distances, the edges
     *  hasDepth* excused, the form of the last path (0 none, 1 from the left, 2 from the right, 3 spliced), 0.  Read-only on both handles. */
    public static native void represented(long h, long gateHandle, ByteBuffer seq, long[] offsets, int n, int lookahead, int maxIndelSize,
                                          int maxEdgeClipLength, float percentIdentity, long maxVisits, int[] recs);
    /** The in-order represented-then-add loop of TranscriptWriter.write (rb_graph_represented_then_add; R/RNABloom.java:1639-1720) and of
     *  GraphUtils.reduceRedundancy (R/util/GraphUtils.java:652-699) for n sequences in list order: sequence i is judged as represented judges
     *  it, but against gateHandle's dbgbf — the writer's screeningBf, which this call WRITES — as every earlier kept sequence of the call
     *  left it.  recs as represented's; keep[i] = 1 where the sequence is judged and not represented: the hash of each of its k-mers has
     *  been added to the gate, and median[i] (median may be null) is its getMedianKmerCoverage, the header's c= value; 0 elsewhere.
     *  Returns n, or the index of the first sequence whose depth search ran out of its budget (flags 32): the walk stops there, the records
     *  behind it are blank with flags 64 (not reached), and the caller decides that sequence itself and calls again on the rest. */
    public static native long representedThenAdd(long h, long gateHandle, ByteBuffer seq, long[] offsets, int n, int lookahead, int maxIndelSize,
                                                 int maxEdgeClipLength, float percentIdentity, long maxVisits, int[] recs, byte[] keep,
                                                 float[] median);
    /** GraphUtils.trimReverseComplementArtifact (rb_graph_trim_rc_artifacts) of n sequences: mode 0 the (kmers, graph, stranded) overload
     *  (R/util/GraphUtils.java:8588-8661), 1 the one with maxEdgeClip (:7918-8057), 2 the one with maxEdgeClip and maxCovGradient (:7762-7916);
     *  the graph's own strandedness is the reference's `stranded`.  recs holds 16 ints per sequence — flags (1: a line of the reference cut,
     *  for mode 0 the result is not null; 2: something was trimmed; not judged: 8 a letter outside ACGTU, 16 no k-mer, 32 reserved), begin and
     *  end of the k-mers kept (the list's subList(begin, end)), the mode, then for each of the two passes the line that decided and four
     *  indices (include/rb_capi.h), 0, 0.  Read-only. */
    public static native void trimArtifacts(long h, ByteBuffer seq, long[] offsets, int n, int mode, int maxEdgeClip, float maxCovGradient, int[] recs);
    /** GraphUtils.correctLongSequenceWindowed (rb_graph_correct_long, R/util/GraphUtils.java:3087-3185) of n sequences.  params: maxErrCorrItr,
     *  lookahead, maxIndelSize, minKmerCov, minNumSolidKmers, trimLowCovEdges (0 / 1), windowSize.  outOffsets (n + 1) is the caller's capacity
     *  layout of `out`: the final text of sequence i is written at outOffsets[i] if it fits.  recs holds 16 ints per sequence — status (0 the
     *  reference returns null, 1 unchanged, 2 changed, 3 no k-mer), the passes that corrected, the final length (the room needed, where it did
     *  not fit), the k-mers the edge trim kept or -1, -1, ten event counters (include/rb_capi.h), flags (1: the text did not fit and was not
     *  written, 2: trimmed to nothing).  Read-only. */
    public static native void correctLong(long h, ByteBuffer seq, long[] offsets, int n, int[] params, float maxCovGradient, float percentIdentity,
                                          long[] outOffsets, ByteBuffer out, int[] recs);
    /** The accept / reject loop of SeqSubsampler.strobemerBased / kmerBased (rb_subsample_reads, R/util/SeqSubsampler.java:374-460, :150-226,
     *  :233-318) over n reads IN ARRAY ORDER against the counting filter of handle h, which the call reads and writes; the filter and the op
     *  ordinal carry from call to call.  params: mode (0 strobemers, 1 k-mer pairs), k, wMin, wMax, canonical (k-mer mode, !stranded),
     *  maxMultiplicity, maxEdgeClip.  keep: a byte per read (1 kept); recs (may be null): 8 ints a read — status, the reference line that
     *  decided, the deciding index, namInterval.start, namInterval.end (k-mer mode: start, missingChainLen), elements, unseen, distinct hashes
     *  incremented; totals (may be null): kept, increments, not judged, nanoseconds in the walker.  One read's distinct hashes are incremented
     *  in order of first occurrence: one of the orders the reference's parallelStream may take. */
    public static native void subsampleReads(long h, int[] params, ByteBuffer seq, long[] offsets, int n, byte[] keep, int[] recs, long[] totals);
    /** What LongReadCorrectionWorker.run does to n raw reads before its first graph call (rb_long_prepare, R/RNABloom.java:3705-3779): the
     *  reverse complement where asked, PolyATailFinder.findPolyATail / findPolyTHead and the five-way rule that cuts and turns the read,
     *  SeqUtils.trimLowComplexityRegions, hasPolyA.  No graph handle: text work on `device`.  params: k (shorter reads are discarded),
     *  reverseComplement, strandSpecific, minPolyATailLengthRequired > 0 (0 / 1), the finder's seedLength, maxGap and window, the window and the
     *  minimum length of trimLowComplexityRegions (100, 500).  segOffsets (n + 1) is the caller's layout of `segs`, 2 ints a slot: read i needs
     *  room for max(1, (length / window + 1) / 2) segments.  recs holds 16 ints per read — status (0 too short, 1 low complexity: no segment,
     *  2 segments), flags (1 the transformed read runs against the input, 2 hasPolyA, 4 / 8 a tail / a head was found, 16 the cut fired,
     *  32 / 64 / 128 the complexity route, 256 turned twice), the input letters kept [begin, end), tail and head as [start, end) or -1, the
     *  windows, the low ones, the offset, the number of segments, the seed searches of both chains, 0, 0 (include/rb_capi.h).  out (may be null)
     *  receives the transformed read of read i at offsets[i]: its segments are substrings of it. */
    public static native void longPrepare(int device, ByteBuffer seq, long[] offsets, int n, int[] params, float minIdentity, long[] segOffsets,
                                          int[] recs, int[] segs, ByteBuffer out);
    /** GraphUtils.correctErrorsPE (rb_graph_correct_pairs, R/util/GraphUtils.java:4051-4182) of n read pairs, every round inside the call; with
     *  rseq, roffsets, routOffsets and rout all null, GraphUtils.correctErrorsSE (:3998-4049) of n reads.  params: errorCorrectionIterations,
     *  lookahead, maxIndelSize; fparams: maxCovGradient, covFPR, minCovThreshold, percentIdentity, minKmerCov.  loutOffsets / routOffsets (n + 1)
     *  are the caller's capacity layouts: a final text is written at its offset if it fits.  recs holds 16 ints per pair — status (0 unchanged,
     *  1 corrected, 2 not judged), end (0 the rounds ran out, 1 nothing changed, 2 threshold too low, 3 a mate without a k-mer, 4 a mate lost
     *  its k-mers), the rounds the helper ran in, flags (1 left corrected, 2 right corrected, 4 / 8: the left / right text did not fit and was
     *  not written), the final lengths (the room needed, where it did not fit), the float bits of the first and last threshold, the found bits
     *  of round 0, the rounds that changed the left / right mate, gaps replaced / trimmed / kept, mismatches, 0 (include/rb_capi.h).  Read-only. */
    public static native void correctPairs(long h, ByteBuffer lseq, long[] loffsets, ByteBuffer rseq, long[] roffsets, int n, int[] params,
                                           float[] fparams, long[] loutOffsets, ByteBuffer lout, long[] routOffsets, ByteBuffer rout, int[] recs);
    /** getKmers of nReads sequences: koffsets[nReads + 1] is filled; pass f == null to size the outputs first. */
    public static native void getKmers(long h, ByteBuffer seq, long[] offsets, int nReads, long[] koffsets, long[] f, long[] r, float[] count);
    public static native void neighbors(long h, long[] f, long[] r, byte[] charOut, int n, int direction, long[] f4, long[] r4, float[] count4);
    public static native void walk(long h, byte[] seeds, byte[] targets, int n, int direction, int bound, float minKmerCov,
                                   byte[] outBases, long[] outF, long[] outR, float[] outCount, int[] outLen, byte[] outReason);
    public static native void greedyExtend(long h, long gateHandleOr0, byte[] seeds, int n, int direction, int lookahead, int bound,
                                           byte[] outBases, float[] outCount, int[] outLen, byte[] outReason);

    /** GraphUtils.naiveExtendRight / Left for n seeds: mode 0 terminator forms (termSeq / termOff, capacity cap), 1 bounded, 2 NoBackChecks. */
    public static native void naiveExtend(long h, byte[] seeds, int n, int direction, int mode, int bound, int cap, float minKmerCov,
                                          byte[] termSeq, long[] termOff, byte[] outBases, int[] outLen, byte[] outReason);

    // ---- filter state ----
    /** {size, bytes, numHash} */
    public static native long[] filterSize(long h, int which);
    public static native long popcount(long h, int which);
    /** rb_filter_fold: 64-bit digest of the filter's bytes, computed on the device (compare filters without exporting them) */
    public static native long fold(long h, int which);
    public static native float fpr(long h, int which);
    public static native void exportFilter(long h, int which, ByteBuffer dst, long nBytes);
    public static native void importFilter(long h, int which, ByteBuffer src, long nBytes);
    /** the same for filters of 2 GiB and more (beyond a direct ByteBuffer): the shim maps the file */
    public static native void importFilterFromFile(long h, int which, String path, long nBytes);
    public static native void exportFilterToFile(long h, int which, String path, long nBytes);
    public static native long expectedSize(long expNumElements, float fpr, int numHash);
    public static native void cbfToBloom(long src, float minCov, long dst, int which);

    // ---- hash-only work over sequences (no graph needed; countIn: 0 or a handle whose cbf is asked getCount) ----
    /** returns the number of windows / strobemers written; offsetsOut[nReads + 1]. Call with outHash == null to size. */
    public static native long minimizers(int device, ByteBuffer seq, long[] offsets, int nReads, int k, int w, int mode,
                                         long[] offsetsOut, long[] outHash, long[] outPos);
    public static native long minimizersNext(int device, ByteBuffer seq, long[] offsets, int nReads, int k, int w, int mode,
                                             long[] offsetsOut, long[] outHash, long[] outPos);
    public static native long minimizerSet(int device, ByteBuffer seq, long[] offsets, int nReads, int k, int w, int mode, long[] stale,
                                           long[] offsetsOut, long[] out);
    public static native long strobemers(int device, ByteBuffer seq, long[] offsets, int nReads, int k, int n, int wMin, int wMax,
                                         long[] offsetsOut, long[] outHash, int[] outStart, int[] outEnd);
    public static native long randstrobes(int device, ByteBuffer seq, long[] offsets, int nReads, int k, int n, int wMin, int wMax, int flags,
                                          long countIn, long[] offsetsOut, long[] outHash, int[] outPos, float[] outCount);
    public static native long strobe3(int device, ByteBuffer seq, long[] offsets, int nReads, int k, int wMin, int wMax, boolean canonical,
                                      long countIn, long[] offsetsOut, long[] outHash, int[] outPos, float[] outCount);
    public static native long kmerPairHashes(int device, ByteBuffer seq, long[] offsets, int nReads, int k, int shift, boolean canonical,
                                             long countIn, long[] offsetsOut, long[] outHash, float[] outCount);

    // ---- input formats ----
    /** FASTQ text -> seq / qual (direct buffers of at least textLen bytes; qual may be null) + offsets; returns the record count.
     *  Call with offsets == null for the count only. */
    public static native long fastqSplit(ByteBuffer text, long textLen, int nThreads, ByteBuffer seq, ByteBuffer qual, long[] offsets);
    /** every member of a gzip byte string (direct buffers; dst == null: returns the uncompressed size); BGZF in parallel. */
    public static native long gunzip(ByteBuffer src, long n, int nThreads, ByteBuffer dst, long cap);
    /** FASTQ text (direct buffer) parsed and encoded on the GPU; isFinal = false: a piece of a longer input, consumed[0] = where the
     *  next piece starts. */
    public static native long batchCreateFastq(int device, ByteBuffer text, long textLen, boolean isFinal, int minBaseQual, boolean useQual, long[] consumed);
    /** FASTA text parsed on the GPU (FastaReader.next semantics); consumedAndEnded = {bytes consumed, 1 if an empty header line ended the iteration}. */
    public static native long batchCreateFasta(int device, ByteBuffer text, long textLen, boolean isFinal, long[] consumedAndEnded);
    /** FastaToGraphWorker's loop over the text of a whole FASTA file; nRecords[0] = records inserted. */
    public static native long[] addFasta(long h, ByteBuffer text, long textLen, int flags, long[] nRecords);
    /** FastqToGraphWorker's loop over the text of a whole file (pieces of 1 GiB, parsed on the GPU); nRecords[0] = records inserted. */
    public static native long[] addFastq(long h, ByteBuffer text, long textLen, int minBaseQual, int flags, long[] nRecords);
    /** a FASTQ / FASTA FILE (plain or gzip) streamed piece by piece: the next piece is read / inflated and parsed while the current one is inserted */
    public static native long[] addFastqFile(long h, String path, int minBaseQual, int flags, long[] nRecords);
    public static native long[] addFastaFile(long h, String path, int flags, long[] nRecords);
    /** NucleotideBitsWriter.write for nReads sequences; out == null: returns the size needed. */
    public static native long nbitsEncode(ByteBuffer seq, long[] offsets, int nReads, ByteBuffer out, long cap);
}
