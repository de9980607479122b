"""Host mirror of the part of rnabloom.util.GraphUtils that sits directly on the neighbour-extension loop, batched over
many k-mer pairs: the graph work (every getMaxCovSuccessor / getMaxCovPredecessor step) runs in two rb_graph_walk calls
per batch; what is left on the host is the bookkeeping of R/util/GraphUtils.java:1591-1675."""
import ctypes as C
import math

LOW_COMPLEXITY_THRESHOLD_SHORT_SEQ = 0.95          # R/util/SeqUtils.java:61
_IDX = {65: 0, 67: 1, 71: 2, 84: 3, 85: 3}         # nucleotideArrayIndex, R/util/SeqUtils.java:315-330 (upper case only)


def _java_round(x):
    return int(math.floor(x + 0.5))                # Math.round(float)


def isLowComplexityShort(seq):
    """R/util/SeqUtils.java:499-543 (String version): homopolymer / di- / tri-nucleotide repeats counted over a sliding
    window of three bases, then the two-letter content test.  length/2 and length/3 are integer divisions."""
    seq = bytes(seq)
    length = len(seq)
    t1 = min(32767, _java_round(length * LOW_COMPLEXITY_THRESHOLD_SHORT_SEQ))
    t2 = min(32767, _java_round((length // 2) * LOW_COMPLEXITY_THRESHOLD_SHORT_SEQ))
    t3 = min(32767, _java_round((length // 3) * LOW_COMPLEXITY_THRESHOLD_SHORT_SEQ))
    nf1 = [0] * 4
    nf2 = [[0] * 4 for _ in range(4)]
    nf3 = [[[0] * 4 for _ in range(4)] for _ in range(4)]
    c3, c2, c1 = _IDX[seq[0]], _IDX[seq[1]], _IDX[seq[2]]
    nf1[c3] += 1; nf1[c2] += 1; nf1[c1] += 1
    nf2[c3][c2] += 1; nf2[c2][c1] += 1
    nf3[c3][c2][c1] += 1
    for ch in seq[3:]:
        c3, c2, c1 = c2, c1, _IDX[ch]
        nf1[c1] += 1
        if nf1[c1] >= t1:
            return True
        nf2[c2][c1] += 1
        if nf2[c2][c1] >= t2:
            return True
        nf3[c3][c2][c1] += 1
        if nf3[c3][c2][c1] >= t3:
            return True
    return any(nf1[a] + nf1[b] >= t1 for a in range(4) for b in range(a + 1, 4))


def _kmers_right(seed, appended, k):
    s = seed + appended
    return [s[j + 1:j + 1 + k] for j in range(len(appended))]


def _kmers_left(seed, prepended, k):
    """k-mers of a left walk in the order they were found (nearest to the seed first)"""
    s = prepended[::-1] + seed
    n = len(prepended)
    return [s[n - 1 - j:n - 1 - j + k] for j in range(n)]


def getMaxCoveragePaths(graph, lefts, rights, bound, minKmerCov=1.0):
    """GraphUtils.getMaxCoveragePath(graph, left, right, bound, lookahead, minKmerCov) (R/util/GraphUtils.java:1591-1675) for
    many (left, right) pairs at once.  lefts / rights: k-mers as upper-case bytes.  Returns, per pair, the list of k-mers
    strictly between left and right along the path found, or None — exactly what the reference returns."""
    n = len(lefts)
    k = graph.k
    out = [None] * n
    bases, _, _, _, ln, reason = graph.walkMaxCov(lefts, 0, bound, minKmerCov, rights, hashes=False, counts=False)      # :1603-1620
    left_paths = []
    todo = []
    for i in range(n):
        lp = _kmers_right(lefts[i], bytes(bases[i, :ln[i]]), k)
        left_paths.append(lp)
        if reason[i] == 1:
            out[i] = lp                                                                     # :1609-1611
        elif reason[i] != 4:
            todo.append(i)
    if todo:
        bases, _, _, _, ln, reason = graph.walkMaxCov([rights[i] for i in todo], 1, bound, minKmerCov, [lefts[i] for i in todo], hashes=False, counts=False)   # :1629-1672
        for j, i in enumerate(todo):
            if reason[j] == 4:
                continue
            rp = _kmers_left(rights[i], bytes(bases[j, :ln[j]]), k)
            lp = left_paths[i]
            lset = {km: idx for idx, km in reversed(list(enumerate(lp)))}                    # first index of every k-mer
            last = {}
            for idx, km in enumerate(lp):
                last[km] = idx                                                              # descendingIterator finds the LAST equal one
            hit = next((d for d, km in enumerate(rp) if km in lset), None)
            if hit is not None:                                                             # :1644-1664: the right path meets the left path
                best = rp[hit]
                if isLowComplexityShort(best):
                    continue
                out[i] = lp[:last[best]] + [best] + rp[:hit][::-1]
            elif reason[j] == 1:                                                            # :1637-1639
                out[i] = rp[::-1]
    return out


# ---- the k-mer-list pair helpers of BloomFilterDeBruijnGraph (R/graph/BloomFilterDeBruijnGraph.java:474-526), batched over sequences ----
import numpy as np

from . import _native as N
from .graph import _ptr


def _combine(a, b):
    """HashFunction.combineHashValues, R/bloom/hash/HashFunction.java:260-263 (uint64 arithmetic wraps like Java's long)"""
    with np.errstate(over="ignore"):
        return a ^ (b + np.uint64(0xFFFFFFFF9E3779B9) + (a << np.uint64(6)) + (b >> np.uint64(2)))


def kmerPairHashValues(f, r, d, stranded):
    """Kmer.getKmerPairHashValue / CanonicalKmer.getKmerPairHashValue (R/graph/Kmer.java:65-67, CanonicalKmer.java:61-72)
    of the k-mers i and i + d of one sequence, for every i: combine(fL, fR), canonical: the signed minimum of that and
    combine(rR, rL)."""
    fl, fr = f[:-d], f[d:]
    p = _combine(fl, fr)
    if not stranded:
        q = _combine(r[d:], r[:-d])
        p = np.where(q.view(np.int64) < p.view(np.int64), q, p)
    return p


def _pairs_per_sequence(graph, seqs, d):
    ko, f, r, _ = graph.getKmers(seqs)
    out, spans = [], []
    for i in range(len(seqs)):
        a, b = int(ko[i]), int(ko[i + 1])
        n = b - a - d
        spans.append(max(n, 0))
        if n > 0:
            out.append(kmerPairHashValues(f[a:b], r[a:b], d, graph.stranded))
    return (np.concatenate(out) if out else np.zeros(0, np.uint64)), spans


def containsAllPairedKmers(graph, seqs, d):
    """graph.containsAllPairedKmers(kmers) for many sequences (:496-511): False for a sequence without a pair"""
    p, spans = _pairs_per_sequence(graph, seqs, d)
    hit = graph.lookupFragmentKmerPair(p) if p.size else np.zeros(0, bool)
    res, at = [], 0
    for n in spans:
        res.append(bool(n > 0 and hit[at:at + n].all()))
        at += n
    return res


def lookupAndAddAllPairedKmers(graph, seqs, d):
    """graph.lookupAndAddAllPairedKmers(kmers) for many sequences, in order (:513-526): per sequence the AND of
    fpkbf.lookupThenAdd over its pairs (True for a sequence without a pair) — a later sequence sees the pairs of the earlier ones."""
    p, spans = _pairs_per_sequence(graph, seqs, d)
    hit = graph.lookupThenAdd(N.FPKBF, p) if p.size else np.zeros(0, bool)
    res, at = [], 0
    for n in spans:
        res.append(bool(hit[at:at + n].all()))
        at += n
    return res


def getKmersMinCoverage(graph, seqs, minCoverage):
    """HashFunction.getKmers(seq, numHash, graph, minCoverage) (R/bloom/hash/HashFunction.java:86-134) for many sequences:
    the k-mers of the "longest" run with count >= minCoverage — with the reference's bookkeeping kept as it is: the
    list that is open when the scan starts is the result unless a LATER closed run replaces it (its length is never
    recorded, so any later closed run does), and a run still open at the end of the sequence is never compared.
    Returns per sequence (first k-mer index, number of k-mers, their counts)."""
    ko, _, _, c = graph.getKmers(seqs)
    out = []
    for i in range(len(seqs)):
        cnt = c[int(ko[i]):int(ko[i + 1])]
        cur_start, cur_len, cur_min = 0, 0, float("inf")
        best = None                      # None: the result is still the list that was open at the start
        first_open = True                # the current list IS that first list
        first = (0, 0)
        best_len, best_min = 0, float("inf")
        for j, x in enumerate(cnt):
            if x >= minCoverage:
                if cur_len == 0:
                    cur_start = j
                cur_len += 1
                cur_min = min(cur_min, float(x))
            elif cur_len:
                if first_open:
                    first = (cur_start, cur_len)
                elif cur_len > best_len or (cur_len == best_len and cur_min > best_min):
                    best, best_len, best_min = (cur_start, cur_len), cur_len, cur_min
                first_open = False
                cur_len, cur_min = 0, float("inf")
        if first_open:
            first = (cur_start, cur_len) if cur_len else (0, 0)
        s, n = best if best is not None else first
        out.append((s, n, cnt[s:s + n].copy()))
    return out


def overlapAndConnect(graph, lefts, rights, bound, minOverlap, maxCovGradient, maxTipLen, minKmerCov=1.0):
    """GraphUtils.overlapAndConnect (R/util/GraphUtils.java:5065-5090) for many read pairs: graph.overlapPairs of all of them, then ONE
    graph.joinPairs over the pairs overlap returned null for.  Returns per pair (bytes or None, how): the string the returned k-mers spell
    and "overlap" / "join"; None with "none" where both return null, with "not_judged" where join cannot be asked (a read shorter than k,
    a letter outside ACGTU).  A pair overlap would rescue by writing to the graph comes back as (joined text before the rescue, "rescue"),
    not joined: the caller applies graph.applyOverlapRescue, as with overlapPairs alone."""
    ov = graph.overlapPairs(lefts, rights, minOverlap, minKmerCov)
    res = [(text, "rescue" if outcome == graph.OVL_RESCUE else "overlap") for text, outcome, _ in ov]
    todo = [i for i, (_, outcome, _) in enumerate(ov) if outcome == graph.OVL_NONE]
    if todo:
        jn = graph.joinPairs([lefts[i] for i in todo], [rights[i] for i in todo], bound, maxCovGradient, maxTipLen, minKmerCov)
        for i, (text, outcome, _) in zip(todo, jn):
            res[i] = (text, "join") if outcome == graph.JOIN_JOINED else (None, "not_judged" if outcome == graph.JOIN_NOT_JUDGED else "none")
    return res


def connect(graph, segment_lists, lookahead=0):
    """GraphUtils.connect(segments, graph, lookahead) (R/util/GraphUtils.java:4836-4872) for many reads in ONE graph.connectSegments call: the
    segment lists are filterFastq's / filterFasta's (rnabloom.io).  Returns per read the string the reference returns as bytes, or None for a
    read it cannot be asked about (an even number of entries, a segment shorter than k in a list of several, a letter outside ACGTU).  The
    reference's minKmerCov is 1; lookahead is not read."""
    return [None if outcome == graph.CONNECT_NOT_JUDGED else text for text, outcome, _ in graph.connectSegments(segment_lists, lookahead, 1.0)]


def connectComposed(graph, segment_lists):
    """The same from getMaxCoveragePaths (two lane-per-walk launches for all gaps of one bound, the letters stitched here): the route a caller had
    before graph.connectSegments, kept as its in-library cross-check and as the other side of tools/connect_bench.py.  Every list has an odd
    number of entries, segments of at least k letters of ACGT in upper case."""
    k = graph.k
    by_bound = {}
    for r, segs in enumerate(segment_lists):
        for i in range(1, len(segs), 2):
            by_bound.setdefault(len(segs[i]) + k, []).append((r, i))
    paths = {}
    for bound, where in by_bound.items():
        got = getMaxCoveragePaths(graph, [bytes(segment_lists[r][i - 1][-k:]) for r, i in where], [bytes(segment_lists[r][i + 1][:k]) for r, i in where], bound)
        for key, p in zip(where, got):
            paths[key] = p if p and len(p) <= bound else None
    out = []
    for r, segs in enumerate(segment_lists):
        if len(segs) < 2:
            out.append(bytes(segs[0]) if segs else b"")
            continue
        last = longest = bytes(segs[0])
        for i in range(1, len(segs), 2):
            p = paths[(r, i)]
            last = last + bytes(km[-1] for km in p) + bytes(segs[i + 1][k - 1:]) if p else bytes(segs[i + 1])
            if len(last) > len(longest):
                longest = last
        out.append(longest)
    return out


def _pair_params(lookahead, maxIndelSize, maxCovGradient, covFPR, errorCorrectionIterations, minCovThreshold, percentIdentity, minKmerCov):
    return dict(lookahead=lookahead, maxIndelSize=maxIndelSize, maxCovGradient=maxCovGradient, covFPR=covFPR,
                errorCorrectionIterations=errorCorrectionIterations, minCovThreshold=minCovThreshold, percentIdentity=percentIdentity,
                minKmerCov=minKmerCov)


def correctErrorsPE(graph, lefts, rights, lookahead, maxIndelSize, maxCovGradient, covFPR, errorCorrectionIterations, minCovThreshold,
                    percentIdentity, minKmerCov):
    """GraphUtils.correctErrorsPE (R/util/GraphUtils.java:4051-4182) for many pairs in ONE graph.correctPairs call, all rounds on the device
    (rb_graph_correct_pairs).  Returns per pair (left, right, corrected) — the strings the reference's ReadPair spells, as bytes — or None for a
    pair one of whose mates has no k-mer (the reference throws).  The k-mer lists are getKmers(String)'s of the texts: the worker's stretch
    selection getKmers(left, minKmerCov) comes before the call."""
    return graph.correctPairs(lefts, rights, **_pair_params(lookahead, maxIndelSize, maxCovGradient, covFPR, errorCorrectionIterations,
                                                            minCovThreshold, percentIdentity, minKmerCov))


def correctErrorsSE(graph, seqs, lookahead, maxIndelSize, maxCovGradient, covFPR, percentIdentity, minKmerCov):
    """GraphUtils.correctErrorsSE (R/util/GraphUtils.java:3998-4049) for many reads in ONE graph.correctReads call.  Returns per read the
    string the returned k-mers spell, as bytes, or None where the reference returns null."""
    return graph.correctReads(seqs, **_pair_params(lookahead, maxIndelSize, maxCovGradient, covFPR, 1, 0.0, percentIdentity, minKmerCov))


def correctErrorsPEComposed(graph, lefts, rights, lookahead, maxIndelSize, maxCovGradient, covFPR, errorCorrectionIterations, minCovThreshold,
                            percentIdentity, minKmerCov):
    """The same from the calls a caller had before graph.correctPairs, with the loop (:4066-4179) on the host: per round a ReadBatch of each
    side's current texts, graph.coverageStats with mates (the two searches and the combining rule), graph.correctErrors on the mates of the
    pairs whose threshold passes, the texts read back.  Kept as the in-library cross-check of correctErrorsPE and as the other side of
    tools/correct_pairs_bench.py."""
    from .graph import ReadBatch, _pack
    k = graph.k
    cur = [[s.encode() if isinstance(s, str) else bytes(s) for s in side] for side in (lefts, rights)]
    n = len(cur[0])
    judged = [len(cur[0][i]) >= k and len(cur[1][i]) >= k for i in range(n)]
    corrected = [False] * n
    live = [i for i in range(n) if judged[i]]
    for _ in range(errorCorrectionIterations):
        if not live:
            break
        packed = [_pack([cur[side][i] for i in live]) for side in (0, 1)]
        lb, rb = (ReadBatch.from_ascii(seq, None, off, 0, graph.device) for seq, off in packed)
        try:
            _, _, thr = graph.coverageStats(lb, mates=rb, maxCovGradient=maxCovGradient, covFPR=covFPR, minKmerCov=minKmerCov)
        finally:
            lb.close()
            rb.close()
        run = [j for j in range(len(live)) if thr[j] >= minCovThreshold]
        if not run:
            break                                    # nothing can change any more: every later round repeats this one
        res = graph.correctErrors([cur[side][live[j]] for side in (0, 1) for j in run], [float(thr[j]) for _ in (0, 1) for j in run],
                                  lookahead, maxIndelSize, percentIdentity, minKmerCov)
        nxt = []
        for x, j in enumerate(run):
            i = live[j]
            changed = False
            for side in (0, 1):
                text, ok = res[side * len(run) + x]
                if ok:
                    cur[side][i] = text
                    corrected[i] = changed = True
            if changed:
                if len(cur[0][i]) < k or len(cur[1][i]) < k:
                    judged[i] = False                # the next round would throw
                else:
                    nxt.append(i)
        live = nxt
    return [(cur[0][i], cur[1][i], corrected[i]) if judged[i] else None for i in range(n)]


def extendSE(graph, seqs, minKmerCov, max_rounds=100000):
    """GraphUtils.extendSE(kmers, graph, maxTipLength, minKmerCov) (R/util/GraphUtils.java:6454-6565) for many sequences: first to the left,
    then to the right, each sequence is extended across branches by extendLeftSE / extendRightSE until the step returns nothing at the
    lowest floor or only k-mers the sequence already holds (usedKmers + hasDuplicatedKmerPair, :6416-6452).  The step runs on the device,
    ONE graph.extendStepSE call per round for all sequences still growing, each with its own floor max(minKmerCov, min count of its last d
    k-mers * 0.1), lowered by a further * 0.1 while the step returns nothing; the counts come from graph.getKmers of the sequences' ends.
    Returns (extended sequences, [leftExtLen, leftExtLen + origLen] per sequence, in k-mers).  The reference's loop has no bound;
    max_rounds raises instead of looping forever.  extendSEOnDevice is the same in one device call for all rounds."""
    return _extend_loop(graph, seqs, minKmerCov, max_rounds, graph.getReadPairedKmerDistance(), graph.extendStepSE, "extendSE")


def extendPE(graph, seqs, minKmerCov, max_rounds=100000):
    """GraphUtils.extendPE (R/util/GraphUtils.java:6567-6678), the loop the transcript stage runs whenever fragment-paired k-mers exist
    (R/RNABloom.java:1846-1851): extendSE's loop with d = the FRAGMENT-paired k-mer distance and extendLeftPE / extendRightPE as the step
    (graph.extendStepPE, one call per round).  A step the reference's isRepeat would throw in counts as one that returns nothing.
    extendPEOnDevice is the same in one device call for all rounds."""
    return _extend_loop(graph, seqs, minKmerCov, max_rounds, graph.getFragPairedKmerDistance(), graph.extendStepPE, "extendPE")


def extendSEOnDevice(graph, seqs, minKmerCov, room=4096):
    """extendSE with the whole loop on the device (graph.extendLoop, rb_graph_extend_loop): what extendSE returns — the extended sequences and
    [leftExtLen, leftExtLen + origLen] per sequence — from ONE call for all rounds of all sequences.  room is the most letters a call adds on
    each side of a sequence; the few sequences that want more get further calls, with the room doubled each time.  A sequence the device does
    not judge (a letter other than upper-case A C G T) goes through extendSE's host loop, in one call for all of them."""
    return _extend_on_device(graph, seqs, minKmerCov, room, graph.EXTL_SE, extendSE)


def extendPEOnDevice(graph, seqs, minKmerCov, room=4096):
    """extendPE with the whole loop on the device: as extendSEOnDevice, with the fragment-paired distance and step."""
    return _extend_on_device(graph, seqs, minKmerCov, room, graph.EXTL_PE, extendPE)


def naiveExtend(graph, seqs, maxTipLength, minKmerCov, room=256, keepNotJudged=False):
    """GraphUtils.naiveExtend(kmers, graph, maxTipLength, minKmerCov) (R/util/GraphUtils.java:6935-6957) of each sequence's getKmers list on
    the device (graph.naiveExtendFragments, rb_graph_naive_extend_fragments): the strings the extended lists spell.  maxTipLength is accepted and
    unused, as in the reference's effect (Kmer.hasDepthLeft / hasDepthRight never consult the graph).  room is the most letters a call adds
    on each side; a sequence that wants more is resumed with the returned text — both walks after a left walk ran out of room, the right walk
    only (phase 1) after the right one did — until every sequence is done.  A sequence the device does not judge (fewer than k letters, a
    letter other than upper-case A C G T) raises ValueError, or is returned as it is with keepNotJudged."""
    texts = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    todo, phase = list(range(len(texts))), None
    while todo:
        got, recs = graph.naiveExtendFragments([texts[i] for i in todo], minKmerCov, room, phase)
        nxt, phase = [], []
        for i, t, rc in zip(todo, got, recs):
            status = int(rc["status"])
            if status == N.NFRAG_NOT_JUDGED:
                if not keepNotJudged:
                    raise ValueError("naiveExtend: sequence %d is not judged (%s)" % (i, graph.NFRAG_WHYS[int(rc["why"])]))
                continue
            texts[i] = t
            if status == N.NFRAG_ROOM:
                nxt.append(i)
                phase.append(0 if int(rc["left_end"]) == N.NFRAG_END_ROOM else 1)
        todo = nxt
    return texts


def naiveExtendComposed(graph, seqs, minKmerCov, cap):
    """What ONE graph.naiveExtendFragments call with room = cap returns as texts, composed of two graph.naiveExtend calls (rb_graph_naive_extend,
    mode 0) as a caller had to before rb_graph_naive_extend_fragments: the left walk from each sequence's first k-mer with the sequence as
    terminators, then — for the sequences whose left walk did not fill its cap — the right walk from the last k-mer with the left extension +
    the sequence as terminators.  Sequences of upper-case A C G T with at least k letters.  Serves the A/B
    (tools/naive_extend_fragments_bench.py) and an equality test."""
    k = graph.k
    texts = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    if not texts:
        return []
    lext, lreason = graph.naiveExtend([t[:k] for t in texts], 1, mode=0, minKmerCov=minKmerCov, terminators=texts, cap=cap)
    texts = [l[::-1] + t for l, t in zip(lext, texts)]                # (a left walk returns its bases in walking order)
    go = [i for i, r in enumerate(lreason) if r != 6]                 # (6: the cap was reached — the new call's END_ROOM, behind which its right walk does not run)
    if go:
        rext, _ = graph.naiveExtend([texts[i][-k:] for i in go], 0, mode=0, minKmerCov=minKmerCov, terminators=[texts[i] for i in go], cap=cap)
        for i, r in zip(go, rext):
            texts[i] += r
    return texts


FRAG_KEPT, FRAG_INCONSISTENT, FRAG_SPURIOUS, FRAG_EMPTY, FRAG_NO_COMPLEX_KMER, FRAG_TOO_SHORT = range(6)
FRAG_OUTCOMES = ("kept", "inconsistent", "spurious", "empty", "no_complex_kmer", "too_short")


def finishFragments(graph, fragments, leftNk, rightNk, *, lookahead, minNumKmerPairs, maxTipLength, minKmerCov, extendFragments, trimArtifact,
                    room=256):
    """The second half of FragmentAssembler.run for connected read pairs (R/RNABloom.java:2182-2268): fragments[i] is the string the k-mers
    overlapAndConnect returned spell (upper-case A C G T), leftNk[i] / rightNk[i] the numbers of k-mers of the pair's (corrected) reads.  One
    batched device call per step over the fragments still alive:
      1. :2186-2203  with readPairedKmerDistance < nk: breakWithReadPairedKmers(F, graph, lookahead) — the argument really is lookahead; not
         exactly one range: dropped (FRAG_INCONSISTENT); range[0] >= leftNk or range[1] < nk - rightNk: dropped (FRAG_SPURIOUS); else cut to it.
      2. :2205-2208  trimArtifact: trimReverseComplementArtifact with maxEdgeClip = maxTipLength.  An empty list is reported (FRAG_EMPTY) where
         the reference would throw in kmers.get(0) of naiveExtend.
      3. :2210-2234  preExtensionFragLen = nk + k - 1.  extendFragments: E = naiveExtend(F); the reference's `E.size() != preExtensionFragLen`
         compares a k-mer count with a letter count, so it holds unless exactly k - 1 k-mers were added — restated as written.  Where it holds:
         breakWithReadPairedKmers(E, graph, minNumKmerPairs), the whole-list form; exactly one range: F = E cut to it (adopted); else F stays.
      4. :2237-2268  nk + k - 1 >= k + lookahead: minCov = the smallest count and hasComplexKmer = some k-mer graph.isRepeatKmer rejects, both
         from the coverage record of the final text (min, n_complex > 0); no complex k-mer: dropped (FRAG_NO_COMPLEX_KMER); shorter: dropped
         (FRAG_TOO_SHORT).
    Returns, per fragment, (text or None, preExtensionFragLen or -1 where steps 1 and 2 dropped it, minCov as numpy.float32 or None, outcome,
    adopted).  graph.addFragmentPairKmers of a kept fragment writes to the graph, and the unconnected pairs (:2269-2307) need no graph call: both
    stay with the caller."""
    from .graph import ReadBatch
    k, d = graph.k, graph.getReadPairedKmerDistance()
    n = len(fragments)
    text = [f.encode() if isinstance(f, str) else bytes(f) for f in fragments]
    outcome, pre, min_cov, adopted = [FRAG_KEPT] * n, [-1] * n, [None] * n, [False] * n
    nk_of = lambda i: len(text[i]) - k + 1
    cut = lambda t, r: t[r[0]:r[1] + k - 1]
    alive = lambda: [i for i in range(n) if outcome[i] == FRAG_KEPT]
    # 1
    idx = [i for i in alive() if d < nk_of(i)]
    if idx:
        for i, ranges in zip(idx, graph.breakWithReadPairedKmers([text[i] for i in idx], lookahead)):
            if len(ranges) != 1:
                outcome[i] = FRAG_INCONSISTENT
            elif ranges[0][0] >= leftNk[i] or ranges[0][1] < nk_of(i) - rightNk[i]:
                outcome[i] = FRAG_SPURIOUS
            else:
                text[i] = cut(text[i], ranges[0])
    # 2
    idx = alive()
    if trimArtifact and idx:
        for i, t in zip(idx, trimReverseComplementArtifact(graph, [text[i] for i in idx], graph.TRIM_EDGE, maxEdgeClip=maxTipLength)):
            if len(t) < k:
                outcome[i] = FRAG_EMPTY
            else:
                text[i] = t
    # 3
    idx = alive()
    for i in idx:
        pre[i] = nk_of(i) + k - 1
    if extendFragments and idx:
        ext = naiveExtend(graph, [text[i] for i in idx], maxTipLength, minKmerCov, room)
        # `extendedFragmentKmers.size() != preExtensionFragLen` (:2216): k-mers against letters, as written
        was = [(i, e) for i, e in zip(idx, ext) if len(e) - k + 1 != pre[i]]
        if was:
            for (i, e), ranges in zip(was, graph.breakWithReadPairedKmers([e for _, e in was], minNumKmerPairs)):
                if len(ranges) == 1:
                    text[i], adopted[i] = cut(e, ranges[0]), True
    # 4
    idx = []
    for i in alive():
        if nk_of(i) + k - 1 >= k + lookahead:
            idx.append(i)
        else:
            outcome[i] = FRAG_TOO_SHORT
    if idx:
        batch = ReadBatch.from_reads([text[i] for i in idx], device=graph.device)
        try:
            recs, _ = graph.coverageStats(batch, minKmerCov=minKmerCov)
        finally:
            batch.close()
        for i, rc in zip(idx, recs):
            min_cov[i] = np.float32(rc["min"])
            if int(rc["n_complex"]) == 0:
                outcome[i] = FRAG_NO_COMPLEX_KMER
    return [(text[i] if outcome[i] == FRAG_KEPT else None, pre[i], min_cov[i], outcome[i], adopted[i]) for i in range(n)]


def _extend_on_device(graph, seqs, minKmerCov, room, which, host_loop):
    k = graph.k
    texts = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    n0 = [max(len(t) - k + 1, 0) for t in texts]
    left = [0] * len(texts)
    todo, phase, host = list(range(len(texts))), None, []
    while todo:
        got, recs = graph.extendLoop([texts[i] for i in todo], which, minKmerCov, room, phase)
        nxt, phase = [], []
        for i, t, rc in zip(todo, got, recs):
            status = int(rc["status"])
            if status == graph.EXTL_NOT_JUDGED:
                host.append(i)
                continue
            texts[i] = t
            left[i] += int(rc["left_ext"])
            if status == graph.EXTL_ROOM:                       # resume where the whole rounds ended: the right side only once the left side has ended
                nxt.append(i)
                phase.append(0 if int(rc["left_end"]) == N.EXTL_END_ROOM else 1)
        todo, room = nxt, min(2 * room, N.EXTL_MAX_ROOM)
    if host:
        got, ranges = host_loop(graph, [texts[i] for i in host], minKmerCov)
        for i, t, r in zip(host, got, ranges):
            texts[i], left[i] = t, r[0]
    return texts, [[l, l + n] for l, n in zip(left, n0)]


def _extend_loop(graph, seqs, minKmerCov, max_rounds, d, step, who):
    """the loop extendSE (:6454-6565) and extendPE (:6567-6678) share: d is the distance of the floor, of the usedKmers test and of
    hasDuplicatedKmerPair; step(seqs, direction, floors) -> (extensions or None, records) is the batched step"""
    F = np.float32
    k = graph.k
    floor = F(minKmerCov)
    texts = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    n0 = [max(len(t) - k + 1, 0) for t in texts]
    kmers = [[t[i:i + k] for i in range(n)] for t, n in zip(texts, n0)]
    used = [set(km) for km in kmers]
    left = [0] * len(texts)
    for direction in (1, 0):
        if direction:
            for km in kmers:
                km.reverse()                                                                        # :6465
        active = [i for i, n in enumerate(n0) if n > 0]
        thr, rounds = {}, 0
        while active:
            rounds += 1
            if rounds > max_rounds:
                raise RuntimeError("%s: %d sequences still grow after %d rounds" % (who, len(active), max_rounds))
            fresh = [i for i in active if i not in thr]
            if fresh:                                                                               # :6468 / :6519 and the first :6473
                ko, _, _, c = graph.getKmers([texts[i][:d + k - 1] if direction else texts[i][-(d + k - 1):] for i in fresh])
                for j, i in enumerate(fresh):
                    thr[i] = max(floor, F(F(c[int(ko[j]):int(ko[j + 1])].min()) * F(0.1)))
            ext, _ = step([texts[i] for i in active], direction, np.array([thr[i] for i in active], F))
            nxt = []
            for i, e in zip(active, ext):
                if not e:
                    if thr[i] != floor:                                                             # :6477: lower the floor and ask again
                        thr[i] = max(floor, F(thr[i] * F(0.1)))
                        nxt.append(i)
                    continue
                t, km = texts[i], kmers[i]
                new = e[::-1] + t if direction else t + e
                ek = [new[len(e) - 1 - j:len(e) - 1 - j + k] for j in range(len(e))] if direction else [new[len(t) - k + 1 + j:len(t) + 1 + j] for j in range(len(e))]
                is_used = all(x in used[i] for x in ek)                                             # :6486-6504
                end_index = max(0, len(km) - d + len(ek))
                j = len(km) - 1
                while j >= end_index and is_used:
                    is_used = km[j] in used[i]
                    j -= 1
                if is_used and (len(km) < d or _has_duplicated_kmer_pair(km, ek[-1], d, len(km) - 1 - d + len(ek))):
                    continue                                                                        # :6506-6508
                km += ek
                used[i].update(ek)
                texts[i] = new
                del thr[i]
                nxt.append(i)
            active = nxt
        if direction:
            for i, km in enumerate(kmers):
                left[i] = len(km) - n0[i]                                                           # :6514
                km.reverse()
    return texts, [[l, l + n] for l, n in zip(left, n0)]


def _has_duplicated_kmer_pair(kmers, cursor, d, mate_index):
    """GraphUtils.hasDuplicatedKmerPair (R/util/GraphUtils.java:6416-6452)"""
    if mate_index < 0:
        return False
    mate = kmers[mate_index]
    idx = [i for i, km in enumerate(kmers) if km == cursor]
    if not idx or idx[-1] - d < 0:
        return False
    if mate == kmers[idx[-1] - d]:
        return True
    return any(i - d >= 0 and mate == kmers[i - d] for i in idx[:-1])


def trimReverseComplementArtifact(graph, seqs, mode, maxEdgeClip=0, maxCovGradient=0.0, keepNotJudged=False):
    """GraphUtils.trimReverseComplementArtifact for many sequences in one rb_graph_trim_rc_artifacts call: mode graph.TRIM_HASHES is the
    (kmers, graph, stranded) overload (R/util/GraphUtils.java:8588-8661), TRIM_EDGE the one the fragment assembler calls with maxTipLength
    (:7918-8057), TRIM_LONG the long-read corrector's (:7762-7916).  Returns, per sequence, the string the returned k-mers spell —
    seq[begin:end + k - 1], "" for an empty list — or None where TRIM_HASHES returns null.  A sequence that is not judged (a letter outside
    ACGTU, no k-mer) raises ValueError, or is returned as it is with keepNotJudged."""
    k = graph.k
    recs = graph.trimArtifacts(seqs, mode, maxEdgeClip, maxCovGradient)
    out = []
    for i, (s, rc) in enumerate(zip(seqs, recs)):
        flags, begin, end = int(rc["flags"]), int(rc["begin"]), int(rc["end"])
        if flags & graph.TRIM_NOT_JUDGED:
            if not keepNotJudged:
                raise ValueError("trimReverseComplementArtifact: sequence %d is not judged (flags %d)" % (i, flags))
            out.append(s)
        elif mode == graph.TRIM_HASHES and not flags & graph.TRIM_FOUND:
            out.append(None)
        else:
            out.append(s[begin:end + k - 1] if end > begin else s[:0])
    return out


def _keep_out(i, seq):
    """writeTranscripts' default decision for a sequence the walk stopped at: report it, keep it out"""
    import sys
    print("writeTranscripts: sequence %d (%d letters) is over the depth search's budget and is left out" % (i, len(seq)), file=sys.stderr)
    return False


def writeTranscripts(graph, bf, seqs, lookahead, maxIndelSize, maxTipLength, percentIdentity, maxVisits=0, decide=_keep_out):
    """The decisions of TranscriptWriter.write (R/RNABloom.java:1639-1720) for a list of transcripts in the order the writer would be handed
    them, in rb_graph_represented_then_add calls: bf is the writer's screeningBf and is written.  Returns (kept, records): kept holds, in
    order, (index, l, c) for every sequence the writer would write — its index in seqs, `l=` its length, `c=` the "%.1f" of
    getMedianKmerCoverage — and records the REPR_DTYPE record of every sequence.  The poly-A regexes and the FASTA stay with the caller.
    A sequence that is over the budget of a depth search stops the walk; decide(index, sequence) -> bool says whether the writer keeps it (its
    k-mers then go into bf through bf.add, its `c=` comes from graph.getKmers), and the walk resumes behind it.  The default reports it and
    keeps it out."""
    seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    recs = np.zeros(len(seqs), graph.REPR_DTYPE)
    kept, at = [], 0
    while at < len(seqs):
        r, keep, median, done = graph.representedThenAdd(seqs[at:], bf, lookahead, maxIndelSize, maxTipLength, percentIdentity, maxVisits)
        upto = min(done + 1, len(r))                         # the records the call judged, the stopped one included
        recs[at:at + upto] = r[:upto]
        kept += [(at + i, len(seqs[at + i]), "%.1f" % float(median[i])) for i in np.flatnonzero(keep[:upto])]
        if done == len(r):
            break
        i = at + done
        if decide(i, seqs[i]):
            _, f, rv, cnt = graph.getKmers([seqs[i]])
            bf.add(f if graph.stranded else np.where(rv.view(np.int64) < f.view(np.int64), rv, f))
            kept.append((i, len(seqs[i]), "%.1f" % _median_f32(cnt)))
        at = i + 1
    return kept, recs


def _median_f32(counts):
    """getMedianKmerCoverage (R/util/GraphUtils.java:229-247): the middle count, or the float32 mean of the two middle ones"""
    c = np.sort(np.asarray(counts, np.float32))
    n = c.size
    return float(c[n // 2]) if n % 2 else float((c[n // 2] + c[n // 2 - 1]) / np.float32(2))


def reduceRedundancy(graph, bf, seqs, lookahead, maxIndelSize, maxTipLength, percentIdentity, maxVisits=0):
    """GraphUtils.reduceRedundancy (R/util/GraphUtils.java:652-699) without its files: the sequences sorted by length, longest first
    (BitSequence.compareTo; Collections.sort is stable), then the represented-then-add loop in one rb_graph_represented_then_add call; bf is
    written.  Returns (kept, removed): kept holds (cid, l, sequence) for every sequence the reference writes as ">cid l=<l>", in its order,
    and removed = seqs.size() - cid.  A sequence over the budget of a depth search raises ValueError (the reference's search has no budget)."""
    seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    order = sorted(range(len(seqs)), key=lambda i: -len(seqs[i]))
    ordered = [seqs[i] for i in order]
    _, keep, _, done = graph.representedThenAdd(ordered, bf, lookahead, maxIndelSize, maxTipLength, percentIdentity, maxVisits)
    if done != len(ordered):
        raise ValueError("reduceRedundancy: sequence %d of the sorted list is over the depth search's budget" % done)
    kept = [(cid + 1, len(ordered[i]), ordered[i]) for cid, i in enumerate(np.flatnonzero(keep))]
    return kept, len(seqs) - len(kept)


def representedThenAddComposed(graph, bf, seqs, lookahead, maxIndelSize, maxEdgeClipLength, percentIdentity, maxVisits=0):
    """The route a caller took before rb_graph_represented_then_add: graph.represented of ONE sequence, then bf.add of a kept sequence's
    hashes, sequence after sequence — a launch and two copies each.  Kept for the tests and tools/represented_then_add_bench.py.  Returns
    (records, keep, n_done) with the stop rule of the one call."""
    seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    recs = np.zeros(len(seqs), graph.REPR_DTYPE)
    keep = np.zeros(len(seqs), np.uint8)
    for i, s in enumerate(seqs):
        recs[i] = graph.represented([s], bf, lookahead, maxIndelSize, maxEdgeClipLength, percentIdentity, maxVisits)[0]
        flags = int(recs[i]["flags"])
        if flags & N.SCREEN_OVER_BUDGET:
            recs[i + 1:] = np.array((N.SCREEN_NOT_REACHED, -1, -1, -1, -1, -1, -1, 0, 0, 0, 0, 0), graph.REPR_DTYPE)
            return recs, keep, i
        if flags == 0:
            _, f, r, _ = graph.getKmers([s])
            bf.add(f if graph.stranded else np.where(r.view(np.int64) < f.view(np.int64), r, f))
            keep[i] = 1
    return recs, keep, len(seqs)


def correctLongSequenceWindowed(graph, seqs, **params):
    """GraphUtils.correctLongSequenceWindowed (R/util/GraphUtils.java:3087-3185) for many sequences in one rb_graph_correct_long call (and a
    second one for the few that outgrew their room).  params: graph.LONG_DEFAULTS' keys, named as the reference's arguments.  Returns, per
    sequence, the string the returned k-mers spell ("" for a list trimmed to nothing), or None where the reference returns null (the
    solid-k-mer screen) and for a sequence without a k-mer, which the reference's caller never passes."""
    texts, recs = graph.correctLong(seqs, **params)
    return [None if int(rc["status"]) in (graph.LONG_NULL, graph.LONG_NO_KMER) else t for t, rc in zip(texts, recs)]


def assembleValidKmers(graph, seqs):
    """GraphUtils.assembleValidKmers (R/util/GraphUtils.java:3626-3654) of each sequence's getKmers list, on the host from one rb_graph_kmers
    call: the strings of the maximal runs of k-mers that have a count above 0 or no letter outside ACGTU."""
    k = graph.k
    seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    ko, _, _, cnt = graph.getKmers(seqs)
    out = []
    for i, s in enumerate(seqs):
        c = cnt[ko[i]:ko[i + 1]]
        bad = np.frombuffer(s, np.uint8)[:, None] != np.frombuffer(b"ACGTUacgtu", np.uint8)[None, :]
        bad = np.concatenate(([0], np.cumsum(bad.all(axis=1))))                       # letters outside ACGTU before each position
        valid = (c > 0) | (bad[k:k + len(c)] - bad[:len(c)] == 0)
        segs, start = [], -1
        for j, v in enumerate(valid):
            if v:
                if start < 0:
                    start = j
            elif start >= 0:
                segs.append(s[start:j - 1 + k])
                start = -1
        if start >= 0:
            segs.append(s[start:])
        out.append(segs)
    return out


def correctLongReads(graph, seqs, trimArtifact=True, **params):
    """What LongReadCorrectionWorker.run does to every segment (R/RNABloom.java:3788-3840), as three batched calls: correctLongSequenceWindowed;
    the seven-argument trimReverseComplementArtifact (mode TRIM_LONG, maxEdgeClip 150, the call's maxCovGradient), whose result is taken only
    if it is not empty and shorter (a sequence that call does not judge — a letter outside ACGTU — stays as it is); assembleValidKmers.
    Returns, per sequence, the list of strings the worker would put out: [] for a segment it discards."""
    return correctLongReadsKept(graph, seqs, trimArtifact, **params)[0]


def correctLongReadsKept(graph, seqs, trimArtifact=True, **params):
    """correctLongReads with what the worker's `kept` needs beside the strings (R/RNABloom.java:3804-3839): per sequence, whether the corrected
    list was not empty — the worker counts the read as kept then, even where assembleValidKmers makes no string of it (every k-mer has
    count 0 and a letter outside ACGTU).  Returns (strings, kept)."""
    corrected = correctLongSequenceWindowed(graph, seqs, **params)
    alive = [i for i, t in enumerate(corrected) if t]
    texts = [corrected[i] for i in alive]
    if trimArtifact and texts:
        grad = params.get("maxCovGradient", graph.LONG_DEFAULTS["maxCovGradient"])
        trimmed = trimReverseComplementArtifact(graph, texts, graph.TRIM_LONG, 150, grad, keepNotJudged=True)
        texts = [t if t and len(t) < len(s) else s for s, t in zip(texts, trimmed)]
    out = [[] for _ in seqs]
    for i, segs in zip(alive, assembleValidKmers(graph, texts)):
        out[i] = segs
    return out, [bool(t) for t in corrected]


# ---- the long-read worker from the raw read on (R/RNABloom.java:3700-3859) ----
# rb_prep_params under the reference's names; the worker's values: the finder's ONT profile with seedLength = minPolyATail and window =
# maxTipLength + minPolyATail (R/RNABloom.java:248-251), trimLowComplexityRegions(seq, 100, 500) (:3768)
PREP_DEFAULTS = dict(reverseComplement=False, strandSpecific=False, minPolyATailLengthRequired=1, seedLength=12, minIdentity=0.9, maxGap=4,
                     window=100, lcWindow=100, lcMinLength=500)
PREP_DTYPE = np.dtype(N.PREP_REC_FIELDS)
assert PREP_DTYPE.itemsize == 64


def prepParams(k, **params):
    unknown = set(params) - set(PREP_DEFAULTS)
    if unknown:
        raise TypeError("prepareLongReads: unknown parameter(s) %s" % sorted(unknown))
    a = dict(PREP_DEFAULTS, **params)
    return N.PrepParams(k, int(bool(a["reverseComplement"])), int(bool(a["strandSpecific"])), int(a["minPolyATailLengthRequired"] > 0),
                        a["seedLength"], a["maxGap"], a["window"], a["lcWindow"], a["lcMinLength"], a["minIdentity"])


def prepSegmentRoom(offsets, lcWindow):
    """the layout rb_long_prepare asks for: seg_offsets (n + 1) with room for max(1, (len / lcWindow + 1) / 2) segments a read"""
    lens = np.diff(np.asarray(offsets, np.int64))
    so = np.zeros(lens.size + 1, np.int64)
    np.cumsum(np.maximum(1, (lens // lcWindow + 1) // 2), out=so[1:])
    return so


def prepareLongFlat(seq, offsets, k, device=0, wantText=True, kernelMs=None, **params):
    """rb_long_prepare on flat host text: read i is seq[offsets[i]:offsets[i + 1]] (uint8).  Returns (recs — PREP_DTYPE —, seg_offsets, segs —
    an (slots, 2) int32 array, recs[i]["n_segments"] rows filled from seg_offsets[i] —, out — the transformed reads at `offsets`, or None).
    kernelMs: a one-element float64 array that receives the kernels' time."""
    seq = np.ascontiguousarray(seq, np.uint8)
    off = np.ascontiguousarray(offsets, np.int64)
    n = off.size - 1
    p = prepParams(k, **params)
    so = prepSegmentRoom(off, max(1, p.lc_window))
    recs = np.zeros(n, PREP_DTYPE)
    segs = np.zeros((int(so[-1]), 2), np.int32)
    out = np.zeros(seq.size, np.uint8) if wantText else None
    ms = None if kernelMs is None else kernelMs.ctypes.data_as(C.POINTER(C.c_double))
    N.check(N.lib.rb_long_prepare(device, _ptr(seq), _ptr(off), n, C.byref(p), _ptr(so), _ptr(recs), _ptr(segs), _ptr(out), ms))
    return recs, so, segs, out


def prepareLongReads(reads, k, device=0, **params):
    """What LongReadCorrectionWorker.run does to a raw read before its first graph call (R/RNABloom.java:3705-3779), for many reads in one
    rb_long_prepare call: the reverse complement where asked, the poly-A tail and poly-T head and the five-way rule that cuts and turns the
    read, trimLowComplexityRegions, hasPolyA.  k: reads shorter than k are discarded.  params: PREP_DEFAULTS' keys.  Returns (recs, segments,
    texts): the records (PREP_DTYPE), per read the list of its segments as bytes ([] for a read that is too short or of low complexity), and
    the transformed read (None for a read that is too short) — what the worker emits for a read of low complexity."""
    reads = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    lens = np.fromiter((len(r) for r in reads), np.int64, len(reads))
    off = np.zeros(len(reads) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    seq = np.frombuffer(b"".join(reads), np.uint8) if len(reads) else np.zeros(0, np.uint8)
    recs, so, segs, out = prepareLongFlat(seq, off, k, device, True, **params)
    raw = out.tobytes()
    segments, texts = [], []
    for i, rc in enumerate(recs):
        if int(rc["status"]) == N.PREP_SHORT:
            segments.append([]); texts.append(None)
            continue
        t = raw[off[i]:off[i] + int(rc["kept_end"]) - int(rc["kept_begin"])]
        texts.append(t)
        segments.append([t[b:e] for b, e in segs[so[i]:so[i] + int(rc["n_segments"])].tolist()])
    return recs, segments, texts


def correctLongReadsFromRaw(graph, names, reads, minKmerCov=1, trimArtifact=True, prep=None, **params):
    """LongReadCorrectionWorker.run (R/RNABloom.java:3700-3859) for a batch of raw reads: prepareLongReads with the graph's k and strandedness
    as strandSpecific (prep: its other parameters), then correctLongReads on the segments — twice at the most, since trimLowCovEdges = minKmerCov
    > 1 and not hasPolyA (:3791) is per read and rb_graph_correct_long takes it per call —, then the worker's naming: _s<sid> for a read cut
    into several segments, _p<partID> for a segment that comes back in several parts, which also clears hasPolyA (:3823-3836).  params: the
    other keys of graph.LONG_DEFAULTS.  Returns (sequences, kept, discarded): the tuples (name, seq, length, score, isRepeat, hasPolyA) of
    Sequence2 in the worker's order — a read of low complexity is emitted as it is with isRepeat true and score 0 — and the worker's counts."""
    names = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    prep = dict(prep or {})
    prep.setdefault("strandSpecific", bool(graph.stranded))
    recs, segments, texts = prepareLongReads(reads, graph.k, graph.device, **prep)
    polya = (recs["flags"] & N.PREP_HAS_POLYA) != 0
    where = [(i, j) for i, segs in enumerate(segments) for j in range(len(segs))]
    parts, alive = {}, {}
    for trim in (False, True):
        group = [(i, j) for i, j in where if (minKmerCov > 1 and not polya[i]) == trim]
        if group:
            got, live = correctLongReadsKept(graph, [segments[i][j] for i, j in group], trimArtifact, minKmerCov=minKmerCov, trimLowCovEdges=trim,
                                             **params)
            parts.update(zip(group, got))
            alive.update(zip(group, live))
    out, kept = [], 0
    for i, (name, rc) in enumerate(zip(names, recs)):
        if int(rc["status"]) == N.PREP_LOW_COMPLEXITY:
            out.append((name, texts[i], len(texts[i]), 0.0, True, False))
        any_kept = False
        for j in range(len(segments[i])):
            seg_name = name + (b"_s%d" % (j + 1) if len(segments[i]) > 1 else b"")
            ps = parts[(i, j)]
            has = bool(polya[i]) and len(ps) == 1
            for q, s in enumerate(ps):
                out.append((seg_name + (b"_p%d" % (q + 1) if len(ps) > 1 else b""), s, len(s), float(len(s)), False, has))
            any_kept = any_kept or alive[(i, j)]              # (:3839: kept once the corrected list is not empty, whatever assembleValidKmers makes of it)
        kept += any_kept
    return out, kept, len(names) - kept
