"""What of rb_graph_naive_extend_fragments can be held without a GPU: the header declares the call and a 64-byte record, the Python layer binds it
with the same fields and constants, the JNI function calls it and the Java class has the batched form; the kernel's resources, read from the
code object inside librb_hip.so; the refusals that come before any device call.  Every test here fails on a tree without the call."""
import ctypes as C
import os
import re

import numpy as np

from test_capi_symbols import ROOT, _jni_functions, _kernel_resources

NAME = "rb_graph_naive_extend_fragments"


def header():
    return open(os.path.join(ROOT, "include", "rb_capi.h")).read()


def test_the_header_declares_the_call_and_a_64_byte_record():
    h = header()
    assert re.search(r"int %s\(rb_graph \*g, const char \*seq, const int64_t \*offsets, int64_t n,\s*const uint8_t \*phase[^,]*,\s*float min_kmer_cov, "
                     r"int room,\s*int64_t \*out_offsets, char \*out_seq, rb_naive_frag_rec \*recs\);" % NAME, h)
    body = re.search(r"typedef struct rb_naive_frag_rec \{(.*?)\} rb_naive_frag_rec;", h, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in re.findall(r"int32_t ([^;]+);", body):
        for f in decl.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", f)
            fields.append((m.group(1), int(m.group(2) or 1)))
    assert [f for f, _ in fields] == ["status", "why", "left_ext", "right_ext", "out_len", "left_end", "right_end", "left_hit", "right_hit", "pad"]
    assert 4 * sum(n for _, n in fields) == 64
    assert "R/util/GraphUtils.java:6935-6957" in h and "R/RNABloom.java:2214" in h


def test_the_python_layer_binds_it_with_the_headers_values():
    from rnabloom import _native as N
    from rnabloom import graphutils
    from rnabloom.graph import BloomFilterDeBruijnGraph as G
    assert NAME in {s[0] for s in N.SYMBOLS} and hasattr(N.lib, NAME)
    assert G.NFRAG_DTYPE.itemsize == 64 and G.NFRAG_DTYPE.names[:9] == ("status", "why", "left_ext", "right_ext", "out_len", "left_end", "right_end",
                                                                       "left_hit", "right_hit")
    h = header()
    for name in ("DONE", "ROOM", "NOT_JUDGED", "WHY_NONE", "WHY_NO_KMER", "WHY_LETTER", "END_NOT_RUN", "END_NO_NEIGHBOUR", "END_BACK_BRANCH", "END_SEVERAL",
                 "END_MEMBER", "END_ROOM"):
        assert int(re.search(r"RB_NFRAG_%s = (\d+)" % name, h).group(1)) == getattr(N, "NFRAG_" + name), name
    assert len(G.NFRAG_ENDS) == 6 and len(G.NFRAG_STATUSES) == 3 and len(G.NFRAG_WHYS) == 3
    for f in (G.naiveExtendFragments, G.naiveExtendFragmentsFlat, graphutils.naiveExtend, graphutils.naiveExtendComposed, graphutils.finishFragments):
        assert callable(f)
    assert graphutils.FRAG_OUTCOMES == ("kept", "inconsistent", "spurious", "empty", "no_complex_kmer", "too_short")
    # the threshold between the table's two homes is the kernel's
    src = open(os.path.join(ROOT, "rna-bloom_amd", "csrc", "rb_naive_frag.hip")).read()
    assert int(re.search(r"constexpr int NF_LDS_ENTRIES = (\d+);", src).group(1)) == N.NAIVE_FRAG_LDS_ENTRIES


def test_the_jni_function_calls_it_and_java_has_the_batched_form():
    fns = _jni_functions()
    assert NAME + "(" in fns["naiveExtendFragments"] and "rb_naive_frag_rec" in fns["naiveExtendFragments"]
    java = open(os.path.join(ROOT, "java", "rnabloom", "graph", "NativeGraph.java")).read()
    assert re.search(r"public static native int naiveExtendFragments\(long h, ByteBuffer seq, long\[\] offsets, int n, byte\[\] phase, float minKmerCov, int room,"
                     r"\s*long\[\] outOffsets, ByteBuffer outSeq, int\[\] recs\);", java)
    g = open(os.path.join(ROOT, "java", "rnabloom", "graph", "BloomFilterDeBruijnGraph.java")).read()
    assert "public String[] naiveExtendFragments(String[] seqs, float minKmerCov, int room, int[] records)" in g
    assert g.count("NativeGraph.naiveExtendFragments(handle") == 2          # the size query and the call


def test_the_kernel_spills_no_vector_register_and_five_workgroups_share_a_cu():
    from rnabloom import _native as N
    found = {name: v for name, v in _kernel_resources().items() if "k_naive_frag" in name}
    assert len(found) == 1, sorted(found)
    vgprs, spilled, lds = next(iter(found.values()))
    assert spilled == 0 and vgprs <= 128, (vgprs, spilled)
    assert lds == 2 * 2 * N.NAIVE_FRAG_LDS_ENTRIES * 8 and 5 * lds <= 160 * 1024, lds      # two wavefronts' tables of 2 x 1024 slots


def test_refusals_that_need_no_device_write_nothing():
    from rnabloom import _native as N
    seq = np.frombuffer(b"ACGT" * 20, np.uint8).copy()
    off = np.array([0, 80], np.int64)
    oo, out, rec = np.full(2, 7, np.int64), np.full(80 + 128, 7, np.uint8), np.full(16, 7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                   # noqa: E731
    rc = N.lib.rb_graph_naive_extend_fragments(None, p(seq), p(off), 1, None, 1.0, 64, p(oo), p(out), p(rec))
    assert rc == 1 and NAME.encode() in N.lib.rb_last_error()
    assert (oo == 7).all() and (out == 7).all() and (rec == 7).all()


def test_the_documents_name_the_call():
    for doc, words in (("README.md", (NAME, "rb_naive_frag.hip")), ("DESIGN.md", (NAME,)), ("INTEGRATION.md", ("finishFragments", "naiveExtend")),
                       ("HISTORY.md", (NAME,)), (os.path.join("profiles", "README.md"), ("naive_extend_fragments_bench.txt",))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
