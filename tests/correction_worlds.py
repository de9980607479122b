"""The worlds of tests/test_gpu_correction_matrix.py and tests/test_correction_reach.py: graphs for rb_graph_correct_mismatches and
rb_graph_correct_errors at k = 16 ... 256, stranded and canonical, with hash counts other than (2, 2), from the World classes of
tests/test_gpu_mismatch_correction.py and tests/test_gpu_error_correction.py with read lengths that grow with k (mismatch: max(250, 5 k + 60),
error correction: max(150, 6 k); a dozen transcripts of 4 ... 6 and 4 ... 7 read lengths, k-mer coverage about 20 and about 17).  Around the
slot boundaries of the kernels (k_mismatch: a lane owns windows w, w + 64, ...; k_resolve_snv: k + 2 candidate windows, 64 to a step) k takes
both neighbours: 62 / 63 / 64 / 65, 127 / 128 / 129, 192 / 193, and 256, the ceiling.  Three worlds more: two whose queries hold gaps of more
than 1024 bad k-mers (the Levenshtein row of such a gap lives in device scratch, ce_distance in csrc/rb_correct.hip), and a mismatch world with
a transcript of more than 4096 windows at k = 129 (the code row in device memory, k_mismatch<false>, with three windows to a lane).
The restatements' answers (tests/test_mismatch_rules.py, tests/test_error_correction_rules.py, on the CPU oracle's filters) are computed once
per case and shared by the CPU file (which proves that the worlds ask something) and the GPU file (which compares).  The error-correction
restatement takes SeqUtils.isLowComplexityShort from rnabloom.graphutils (host code; importing the package needs the built library, not a GPU),
so the CPU file, like tests/test_hash_counts_reach.py, runs on a built tree."""
import functools

import numpy as np

import test_gpu_error_correction as EC
import test_gpu_mismatch_correction as MM
from traversal_worlds import HASHES, _prime_above

ACGT = np.frombuffer(b"ACGT", np.uint8)
KS = (16, 31, 32, 33, 62, 63, 64, 65, 127, 128, 129, 143, 192, 193, 256)
# (k, stranded, (dbg_h, cbf_h, pair_h), mismatch min_kmer_cov, error-correction min_kmer_cov, max_indel_size).  Case number i = 2 * (index of k) +
# (0 stranded, 1 canonical); hash counts go round in i, so each occurs six times, on both strandednesses, at k >= 64 as well; the mismatch
# min_kmer_cov goes round 0 / 1 / 2 in i, the other alternates from case to case and changes side from k to k, max_indel_size changes every three cases
CASES = tuple((k, i % 2 == 0, HASHES[i % 5] + (2,), (0.0, 1.0, 2.0)[i % 3], (1.0, 2.0)[(i // 2 + i) % 2], (1, 3)[(i // 3) % 2])
              for i, k in ((2 * j + s, k) for j, k in enumerate(KS) for s in (0, 1)))
N_TX = 12
T = MM.World.T                                                    # 3.0, as EC.T
MM_PLANTED, MM_REV = 36, 8
MM_SIZES = (1_600_033, 1_600_033, 1009)
EC_SETS = dict(isolated=10, within_k=10, indels=15, tips=40, letters=6, several=6, clean=8, bubbles=8)
# dbgbf and cbf of different sizes: with one hash function each and equal sizes a false positive of dbgbf reads the count of the k-mer it collides with
EC_SLOTS = (_prime_above(16_000_000), _prime_above(8_000_000))
LONG_SLOTS = (_prime_above(16_000_000), _prime_above(16_000_000))
# the long gaps: (k, stranded, hashes, max_indel_size); threshold 3, lookahead 5, identity 0.9, min_kmer_cov 1
LONG_GAP_CASES = ((31, True, (2, 2, 2), 1), (65, False, (2, 3, 2), 3))
LONG_GAP = 1100                                                   # letters with substitutions: LONG_GAP + k - 1 > 1024 columns, whatever k is
LEV_LDS = 1024                                                    # csrc/rb_correct.hip
MM_LDS_ROW = 4096                                                 # csrc/rb_mismatch.hip
LONG_ROW_K = 129


def case_id(case):
    k, stranded, hashes = case[:3]
    return "k%d-%s-h%d%d" % (k, "stranded" if stranded else "canonical", hashes[0], hashes[1])


def mm_read_len(k):
    return max(250, 5 * k + 60)


def ec_read_len(k):
    return max(150, 6 * k)


def n_reads_for(coverage, read_len, k, mean_tx):
    """reads of read_len letters that cover N_TX transcripts of mean_tx letters `coverage` times, k-mer by k-mer"""
    return int(coverage * N_TX * (mean_tx - k + 1) / (read_len - k + 1))


def seed_of(case, call):
    k, stranded, hashes = case[:3]
    return 100_000 * call + 100 * k + 16 * hashes[0] + 2 * hashes[1] + (1 if stranded else 0)


def tile(text, read_len, step, ends=8):
    """reads of read_len letters every `step` letters of text, and its two ends `ends` times"""
    return [text[a:a + read_len] for a in range(0, len(text) - read_len + 1, step)] + [text[:read_len]] * ends + [text[-read_len:]] * ends


# ---- mismatch correction ----
def mismatch_world_of(case, extra_reads=()):
    k, stranded, hashes = case[:3]
    L = mm_read_len(k)
    n_reads = max(n_reads_for(20, L, k, 5 * L), 520)                 # (query_sets takes reads 300 ... 520)
    return MM.World(k, stranded, seed_of(case, 1), n_tx=N_TX, n_reads=n_reads, sizes=MM_SIZES, hashes=hashes, read_len=L, tx_len=(4 * L, 6 * L + 1),
                    n_planted=MM_PLANTED, n_rev=MM_REV, extra_reads=extra_reads)


@functools.lru_cache(maxsize=None)
def mismatch_case(case):
    """(world, its query sets, (changed, reverse-only) of the planted and the reverse-only sequences on the oracle: World.assert_not_vacuous)"""
    w = mismatch_world_of(case)
    sets = w.query_sets()
    sets["untouched"], sets["letters"] = sets["untouched"][:40], sets["letters"][:40]
    return w, sets, w.assert_not_vacuous(case[3])


def per_sequence_thresholds(n):
    return np.linspace(0.0, 8.0, n).astype(np.float32)


LONG_ROW_CASE = next(c for c in CASES if c[0] == LONG_ROW_K and not c[1])


@functools.lru_cache(maxsize=None)
def long_row_case():
    """(world, [the long transcript with four planted substitutions, a short planted read], the restatement's answers): the world of
    LONG_ROW_CASE with one transcript more, of MM_LDS_ROW + k + 300 letters, covered about 20 times"""
    k, L = LONG_ROW_K, mm_read_len(LONG_ROW_K)
    rng = np.random.default_rng(4096 + k)
    long_tx = ACGT[rng.integers(0, 4, MM_LDS_ROW + k + 300)].tobytes()
    w = mismatch_world_of(LONG_ROW_CASE, tile(long_tx, L, (L - k) // 20))
    n = len(long_tx)
    seqs = [MM.plant(long_tx, [n // 5, 2 * n // 5, 2 * n // 5 + k // 2, 4 * n // 5], rng), w.planted[0]]
    return w, seqs, w.o.expected(seqs, T, LONG_ROW_CASE[3])


# ---- error correction ----
def errors_world_of(k, stranded, hashes, seed, slots, extra_reads=()):
    L = ec_read_len(k)
    n_reads = max(n_reads_for(17, L, k, 5.5 * L), sum(EC_SETS.values()) + EC_SETS["indels"])
    return EC.World(k, stranded, seed, n_tx=N_TX, n_reads=n_reads, sizes=slots + (1009,), hashes=hashes, read_len=L, tx_len=(4 * L, 7 * L + 1),
                    n_sets=EC_SETS, extra_reads=extra_reads)


@functools.lru_cache(maxsize=None)
def errors_case(case):
    """(world, its queries, the restatement's (text, flags, gap records) of each under the case's min_kmer_cov / max_indel_size)"""
    k, stranded, hashes, _, mincov, max_indel = case
    w = errors_world_of(k, stranded, hashes, seed_of(case, 2), EC_SLOTS)
    seqs = w.all_queries()
    return w, seqs, w.o.expected_errors(seqs, T, mincov, max_indel)


@functools.lru_cache(maxsize=None)
def errors_second_call(case):
    """(every third query, per-sequence thresholds, the restatement's answers under lookahead 3 and identity 0.97)"""
    w, seqs, _ = errors_case(case)
    sub = list(range(0, len(seqs), 3))
    some, thr = [seqs[i] for i in sub], per_sequence_thresholds(len(seqs))[sub]
    return some, thr, w.o.expected_errors(some, thr, case[4], case[5], lookahead=3, pid=0.97)


def long_gap_queries(tx, k):
    """{(kind, outcome the recipe aims at): query}: the transcript with a substitution every 15 letters (identity 14 / 15: replaced) or every 7
    (6 / 7 < 0.9: kept) over LONG_GAP letters — behind the first k + 20 (a path gap), from letter 3 (a left tip), up to the fourth last (a right tip)"""
    rng = np.random.default_rng(7 * k)
    n, out = len(tx), {}
    for outcome, every in ((EC.REPLACED, 15), (EC.KEPT, 7)):
        out[(EC.PATH, outcome)] = MM.plant(tx, range(k + 20, k + 20 + LONG_GAP, every), rng)
        out[(EC.LEFT_EDGE, outcome)] = MM.plant(tx, range(3, LONG_GAP, every), rng)
        out[(EC.RIGHT_EDGE, outcome)] = MM.plant(tx, [n - 1 - p for p in range(3, LONG_GAP, every)], rng)
    return out


@functools.lru_cache(maxsize=None)
def long_gap_case(long_case):
    """(world, the long queries by (kind, outcome), all queries — the long ones spread among the world's short ones —, the restatement's answers,
    the indices of the long ones)"""
    k, stranded, hashes, max_indel = long_case
    L = ec_read_len(k)
    rng = np.random.default_rng(31 * k)
    tx = ACGT[rng.integers(0, 4, LONG_GAP + 3 * k + 60)].tobytes()
    w = errors_world_of(k, stranded, hashes, 300_000 + k, LONG_SLOTS, tile(tx, L, max(1, (L - k) // 17)))
    long_q = long_gap_queries(tx, k)
    seqs, at = w.all_queries(), {}
    for j, (key, s) in enumerate(long_q.items()):
        at[key] = 5 + 20 * j
        seqs.insert(at[key], s)
    return w, long_q, seqs, w.o.expected_errors(seqs, T, 1.0, max_indel), at
