"""The register and LDS budget of the kernel of rb_graph_trim_rc_artifacts (k_trim_artifacts, csrc/rb_trim.hip), read from the code object inside
librb_hip.so; no GPU is needed.  A wavefront-per-sequence kernel spills no vector register and takes at most 256 VGPRs; its LDS is the four
wavefronts' hash tables — 1024 slots of 8 bytes each, twice the 512 k-mers of the longest list whose table stays in LDS (DESIGN.md §5
"Trimming reverse-complement artifacts") — so that five workgroups fit a CU's 160 KB and LDS never holds the kernel below two wavefronts per
SIMD."""
import os
import re

from test_capi_symbols import _kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def trim_kernel():
    res = _kernel_resources()
    tr = {name: v for name, v in res.items() if "k_trim_artifacts" in name}
    assert len(tr) == 1, sorted(tr)
    return next(iter(tr.values()))


def test_the_kernel_spills_no_vector_register_and_takes_at_most_256():
    v = trim_kernel()
    assert v[1] == 0 and v[0] <= 256, v


def test_its_lds_is_what_the_design_states():
    v = trim_kernel()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"`k_trim_artifacts`[^\n]*?LDS list length (\d+)[^\n]*?([\d ]+) bytes of LDS", design)
    assert m, "DESIGN.md states the list length at which the table leaves LDS and the kernel's LDS"
    lds_list, lds = int(m.group(1)), int(m.group(2).replace(" ", ""))
    assert lds == 4 * 2 * lds_list * 8 and v[2] == lds, (v, lds_list, lds)
    src = open(os.path.join(ROOT, "rna-bloom_amd", "csrc", "rb_trim.hip")).read()
    assert re.search(r"constexpr int TR_LDS_LIST = %d;" % lds_list, src)
    import test_trim_artifact_rules as R
    assert R.LDS_LIST == lds_list                                  # the worlds hold lists on both sides of it
