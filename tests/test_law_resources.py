"""Residency of the control-law step kernel k_step_law (csrc/fb_law.hpp, fb_engine.hip), read from the compiler's
kernel-resource-usage remarks that __graft_entry__.build_hip() stores under tests/_emu (no GPU needed): k_fly's occupancy and LDS
layout at both precisions, registers within the budget, scratch pinned against k_step_forces."""
from test_build_resources import LDS_PER_CU, usage  # noqa: F401  (the remark parser is a fixture of that module)
import pytest


# (kernel, its k_step_forces, its k_fly, waves per SIMD, VGPR budget, workgroups per CU in the default build)
@pytest.mark.parametrize('tag,forces_tag,fly_tag,occupancy,vgprs,groups', [('k_step_lawId', 'k_step_forcesId', 'k_flyId', 2, 256, 8),
                                                                          ('k_step_lawIf', 'k_step_forcesIf', 'k_flyIf', 4, 128, 4)])
def test_law_kernel_residency(usage, tag, forces_tag, fly_tag, occupancy, vgprs, groups):  # noqa: F811
    ks = [k for k in usage if tag in k]
    assert len(ks) == 1, list(usage)
    k = usage[ks[0]]
    fly = usage[[n for n in usage if fly_tag in n][0]]
    frc = usage[[n for n in usage if forces_tag in n][0]]
    assert k['Occupancy'] == occupancy == fly['Occupancy'] and k['VGPRs'] <= vgprs       # k_fly's launch bounds
    assert k['LDS Size'] == fly['LDS Size']                                            # k_fly's LDS layout: pool + tree tables, EPB environments
    assert groups*(-(-k['LDS Size'] // 1280)*1280) <= LDS_PER_CU
    # call frames of the stage functions: measured 376 B (FP64) and 416 B (FP32) per lane, 16 B over k_step_forces (360 / 400), which
    # tests/test_forces_resources.py allows 24 B over k_fly
    assert k['ScratchSize'] <= frc['ScratchSize'] + 24
    assert 'k_fly' not in ks[0] and 'k_step_forces' not in ks[0]                       # (the other step kernels' names stay unique)

