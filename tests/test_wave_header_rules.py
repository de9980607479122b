"""The wavefront-per-sequence helpers and the piece loop exist once (csrc/rb_wave.hpp, csrc/rb_pieces.hpp): the sources are searched for the
copies that every device-side call used to bring along, so that they do not grow back.  No GPU, no build: the text of csrc/ is all that is read."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rna-bloom_amd", "csrc")

# a definition of: the 64-bit shuffle, the round-up to 16, Math.round(float), a direction struct of a unit's own, a bad-letter check, a
# wavefront-scope fence macro
COPIES = re.compile(
    r"shfl64\(uint64_t|up16\(size_t|java_round\(float|struct (Ex|Sc)Dir|_bad_letter\(|"
    r'define \w+_FENCE\(\) __builtin_amdgcn_fence\(__ATOMIC_ACQ_REL, "wavefront"\)'
)


def _sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp")):
            with open(os.path.join(CSRC, name), encoding="utf-8") as f:
                yield name, f.read().splitlines()


def test_helpers_are_defined_in_the_wave_header_only():
    found = {}
    for name, lines in _sources():
        for no, line in enumerate(lines, 1):
            for m in COPIES.finditer(line):
                # `_bad_letter(` also matches where the one shared check is called: a call is no definition (a definition starts its line
                # with the function's qualifiers or type)
                is_call = re.search(r"\bwave_bad_letter\($", line[: m.end()]) and not re.match(r"\s*(template\b|__host__|__device__|inline|static|bool)", line)
                if m.group(0) == "_bad_letter(" and name != "rb_wave.hpp" and is_call:
                    continue
                found.setdefault(m.group(0), []).append("%s:%d" % (name, no))
    assert found, "the search found nothing at all: it no longer looks at the sources"
    elsewhere = {k: [w for w in v if not w.startswith("rb_wave.hpp:")] for k, v in found.items()}
    assert not any(elsewhere.values()), {k: v for k, v in elsewhere.items() if v}
    # ... and they are there: each of the five kinds the header has (it has a fence function, no fence macro)
    for kind in ("shfl64(uint64_t", "up16(size_t", "java_round(float", "_bad_letter("):
        assert len(found.get(kind, [])) == 1, (kind, found.get(kind))


def test_longest_list_is_defined_in_the_piece_header_only():
    where = [name for name, lines in _sources() for line in lines if re.search(r"\bint64_t longest_list\(", line)]
    assert where == ["rb_pieces.hpp"], where


def test_piece_loops_do_not_time_themselves():
    """rb_join, rb_overlap and rb_long run on for_each_piece / for_each_host_piece, which times a piece's kernels for them"""
    for name, lines in _sources():
        if name in ("rb_join.hip", "rb_overlap.hip", "rb_long.hip"):
            assert not any("hipEventElapsedTime" in line for line in lines), name
            assert any(re.search(r"\bfor_each_(host_)?piece\(", line) for line in lines), name
