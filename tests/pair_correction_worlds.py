"""The worlds of tests/test_pair_correction_reach.py and tests/test_gpu_pair_correction.py: read pairs for rb_graph_correct_pairs out of the
query sets of tests/test_gpu_error_correction.py's World (k = 25 canonical and stranded, k = 21; 150-letter reads, 60 refillable bubbles) and of
tests/correction_worlds.py's world at k = 65 (390-letter reads), where a second round runs on device-hashed text beyond one 64-bit word of k.
Every query is the left mate of a clean read, and the right mate of a query with three planted substitutions (`several`); a few mates with
fewer than k letters are planted on purpose and are the only pairs that may come back not judged.  The restatement's answers
(tests/test_pair_correction_rules.py on the CPU oracle's filters) are computed once per case and shared by the two files."""
import functools

import correction_worlds as CW
import test_gpu_error_correction as EC
from test_pair_correction_rules import correct_pairs, correct_single

# gradient 0.5, fpr 0.01, 4 iterations, min threshold 2, lookahead 5, indel 1, identity 0.9, min cov 1
PARAMS = dict(iterations=4, lookahead=5, max_indel=1, gradient=0.5, fpr=0.01, min_thr=2.0, pid=0.9, min_cov=1.0)
CASES = ((25, False), (25, True), (21, False), (65, False))          # k, stranded
ROUND_COUNTS = (0, 1)                                               # the other round counts the GPU file calls with, on the first ROUND_PAIRS pairs
ROUND_PAIRS = 150
SEEDS = {(25, False): 176, (25, True): 177, (21, False): 178, (65, False): 179}


def case_id(case):
    return "k%d-%s" % (case[0], "stranded" if case[1] else "canonical")


def world_of(case):
    k, stranded = case
    if k <= 32:
        return EC.World(k, stranded, seed=SEEDS[case], n_sets=dict(bubbles=60))
    return CW.errors_world_of(k, stranded, (2, 2, 2), SEEDS[case], CW.EC_SLOTS)


def pairs_of(w):
    k = w.k
    queries = [q for q in w.all_queries() if len(q) >= k]
    clean = [s for s in w.sets["clean"] if len(s) >= w.read_len]
    several = w.sets["several"]
    pairs = [(q, clean[i % len(clean)]) for i, q in enumerate(queries)] + [(several[i % len(several)], q) for i, q in enumerate(queries)]
    short = [(queries[0], b"ACGT"), (b"", queries[1]), (w.tx[0][:k - 1], w.tx[0][:k - 1]), (queries[2], w.tx[0][:k])]     # the last is judged: one k-mer is a list
    for j, pr in enumerate(short):
        pairs.insert(7 + 50 * j, pr)
    return pairs


@functools.lru_cache(maxsize=None)
def pair_case(case):
    """(world, [(left, right)], [(record, left text, right text)] of the restatement under PARAMS)"""
    w = world_of(case)
    pairs = pairs_of(w)
    return w, pairs, [correct_pairs(l, r, w.k, PARAMS, w.o) for l, r in pairs]


@functools.lru_cache(maxsize=None)
def pair_case_with(case, iterations, n=ROUND_PAIRS):
    """the first n pairs under another round count"""
    w, pairs, _ = pair_case(case)
    return [correct_pairs(l, r, w.k, dict(PARAMS, iterations=iterations), w.o) for l, r in pairs[:n]]


@functools.lru_cache(maxsize=None)
def single_case(case):
    """(world, reads, [(record, text)] of correct_single under PARAMS)"""
    w = pair_case(case)[0]
    seqs = w.all_queries()
    return w, seqs, [correct_single(s, w.k, PARAMS, w.o) for s in seqs]


def gpu_calls(case):
    """the restatement's answers to every pair call tests/test_gpu_pair_correction.py makes for a case — test_pairs_match_the_oracle_and_the_composed_route
    (PARAMS) and test_round_counts (ROUND_COUNTS): {iterations: [(record, left text, right text)]}.  tests/test_pair_correction_reach.py states its
    conditions on these and on nothing else."""
    calls = {PARAMS["iterations"]: pair_case(case)[2]}
    for it in ROUND_COUNTS:
        calls[it] = pair_case_with(case, it)
    return calls
