"""The register and LDS budget of the fragment screens' kernel (k_screen, csrc/rb_screen.hip), read from the code object inside librb_hip.so;
no GPU is needed.  One kernel runs three screens, and it is meant to do so without spilling vector registers and with two wavefronts per
SIMD (256 VGPRs is the last allocation that allows two on the 512-entry file); its LDS is the lookahead stacks alone — 4 wavefronts x 4
candidate lanes x 17 levels x 24 bytes — far below what would limit the workgroups of a CU."""
from test_capi_symbols import _kernel_resources


def screen_kernel():
    res = _kernel_resources()
    sc = {name: v for name, v in res.items() if "k_screen" in name}
    assert len(sc) == 1, sorted(sc)
    return next(iter(sc.values()))


def test_the_kernel_spills_no_vector_register_and_allows_two_wavefronts_per_simd():
    v = screen_kernel()
    assert v[1] == 0 and v[0] <= 256, v


def test_its_lds_is_the_lookahead_stacks():
    v = screen_kernel()
    assert v[2] == 4 * 4 * 17 * 24, v
