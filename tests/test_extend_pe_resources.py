"""The register and LDS budget of the fragment-paired branch extension's kernels (k_extend<PE = true, LDS_ROW>, csrc/rb_extend.hip), read from
the code objects inside librb_hip.so; no GPU is needed.  The kernel is meant to run three wavefronts per SIMD, as the single-end step does and
as DESIGN.md's LDS arithmetic assumes: 168 VGPRs is the last allocation that allows it on the 512-entry file with its 8-register granule."""
from test_capi_symbols import _kernel_resources


def pe_kernels():
    res = _kernel_resources()
    pe = {name: v for name, v in res.items() if "k_extendILb1E" in name}
    assert len(pe) == 2, sorted(n for n in res if "k_extend" in n)
    lds = [v for name, v in pe.items() if "k_extendILb1ELb1E" in name]
    assert len(lds) == 1
    return pe, lds[0]


def test_no_pe_instantiation_spills():
    pe, _ = pe_kernels()
    assert all(v[1] == 0 for v in pe.values()), pe


def test_pe_instantiations_allow_three_wavefronts_per_simd():
    pe, _ = pe_kernels()
    assert all(v[0] <= 168 for v in pe.values()), pe


def test_lds_rows_allow_four_workgroups_per_cu():
    _, lds = pe_kernels()
    assert 0 < lds[2] <= 40 * 1024, lds
