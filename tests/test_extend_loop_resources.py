"""The register and LDS budget of the extension loop's kernels (k_extloop<PE, LDS_ROW>, csrc/rb_extend_loop.hip), read from the code objects inside
librb_hip.so; no GPU is needed.  The loop keeps nothing in LDS of its own: the LDS instantiations hold the branch step's walk rows and nothing
else, EX_WAVES * ex_row_bytes(EX_LDS_D) = 4 * 6512 = 26 048 bytes a workgroup, which lets six workgroups share a CU's 160 KB — six wavefronts per
SIMD.  The registers set the limit below that: the step inlined into the loop takes 228 (SE) and 232 (PE) VGPRs, two wavefronts per SIMD on the
512-entry file (256 is the last allocation that allows two).  The instantiations for D > 256, which run only for distances no RNA-Bloom default
comes near, take a few more and may run one.  Occupancy on hardware is not measured here."""
from test_capi_symbols import _kernel_resources

EX_WAVES, EX_LDS_D, RB_MAX_K = 4, 256, 256


def ex_row_bytes(D):
    """csrc/rb_extend_step.hpp"""
    return (4 * D + 16 * (D + 2) + 4 * ((D + 3) // 4) + 16 * ((D + 2 + 3) // 4) + (RB_MAX_K + 3) // 4 + 15) & ~15


def loop_kernels():
    res = _kernel_resources()
    ks = {name: v for name, v in res.items() if "k_extloopILb" in name}
    assert not any("k_extendIL" in name for name in ks)          # tests/test_extend_pe_resources.py counts the kernels with that in their name
    return ks


def test_the_four_instantiations_exist():
    ks = loop_kernels()
    import re
    assert sorted(re.search(r"k_extloopILb([01])ELb([01])E", n).groups() for n in ks) == [(pe, lds) for pe in "01" for lds in "01"], sorted(ks)


def test_no_instantiation_spills():
    ks = loop_kernels()
    assert len(ks) == 4 and all(v[1] == 0 for v in ks.values()), ks


def test_lds_is_the_step_s_walk_rows_and_registers_allow_two_wavefronts_per_simd():
    ks = loop_kernels()
    lds = {n: v for n, v in ks.items() if "ELb1EE" in n}
    assert len(lds) == 2 and ex_row_bytes(EX_LDS_D) == 6512
    assert all(v[2] == EX_WAVES * ex_row_bytes(EX_LDS_D) for v in lds.values()), lds
    assert all(v[0] <= 256 for v in lds.values()), lds
    assert all(v[2] <= 64 for n, v in ks.items() if n not in lds), ks
