"""Residency of the kernels of fb_batch_lqr_backward (csrc/fb_riccati.hpp), read from the compiler's kernel-resource-usage
remarks of the one compilation __graft_entry__.build_hip() stores under tests/_emu (no GPU needed)."""
from test_build_resources import LDS_PER_CU, usage  # noqa: F401  (the remark parser is a fixture of that module)


def _one(usage, tag):  # noqa: F811
    ks = [k for k in usage if tag in k]
    assert len(ks) == 1, list(usage)
    return usage[ks[0]]


def test_riccati_kernels_keep_everything_in_registers(usage):  # noqa: F811
    for tag in ('k_riccati_gemm', 'k_riccati_gain', 'k_riccati_sym', 'k_riccati_init'):
        assert _one(usage, tag)['ScratchSize'] == 0, tag         # the gain kernel's 64-double right-hand side included


def test_riccati_gain_kernel_lds_is_within_one_cu(usage):  # noqa: F811
    k = _one(usage, 'k_riccati_gain')
    # the 64 x 65 factor + five 64-vectors: 35 840 B, four workgroups per CU by LDS; its registers (one wave per SIMD) are what bounds it
    assert 64*65*8 <= k['LDS Size'] <= 40*1024 and 4*k['LDS Size'] <= LDS_PER_CU
    assert k['VGPRs'] + k['AGPRs'] <= 512 and k['Occupancy'] >= 1


def test_riccati_gemm_kernel_occupancy(usage):  # noqa: F811
    k = _one(usage, 'k_riccati_gemm')
    # 2 x 2 accumulators of 4 doubles in AGPRs + four k-steps' sixteen operands and their addresses: 100 VGPRs + 32 AGPRs at the first
    # clean build, 3 waves per SIMD; at least 2 are wanted, so that one wave's MFMAs run behind another's loads
    assert k['LDS Size'] == 0 and k['VGPRs'] + k['AGPRs'] <= 160 and k['Occupancy'] >= 3
