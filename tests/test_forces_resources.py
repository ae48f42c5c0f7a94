"""Residency of the applied-force step kernel k_step_forces (csrc/fb_forces.hpp, fb_engine.hip), read from the compiler's
kernel-resource-usage remarks that __graft_entry__.build_hip() stores under tests/_emu (no GPU needed): the step kernel's occupancy
and LDS layout at both precisions, scratch pinned at what was measured."""
from test_build_resources import LDS_PER_CU, usage  # noqa: F401  (the remark parser is a fixture of that module)
import pytest


# (kernel, its k_fly, waves per SIMD, VGPR budget, workgroups per CU in the default build, scratch bound)
@pytest.mark.parametrize('tag,fly_tag,occupancy,vgprs,groups,scratch', [('k_step_forcesId', 'k_flyId', 2, 256, 8, 384), ('k_step_forcesIf', 'k_flyIf', 4, 128, 4, 424)])
def test_forces_kernel_residency(usage, tag, fly_tag, occupancy, vgprs, groups, scratch):  # noqa: F811
    ks = [k for k in usage if tag in k]
    assert len(ks) == 1, list(usage)
    k = usage[ks[0]]
    fly = usage[[n for n in usage if fly_tag in n][0]]
    assert k['Occupancy'] == occupancy == fly['Occupancy'] and k['VGPRs'] <= vgprs       # k_fly's launch bounds
    assert k['LDS Size'] == fly['LDS Size']                                            # k_fly's LDS layout: pool + tree tables, EPB environments
    assert groups*(-(-k['LDS Size'] // 1280)*1280) <= LDS_PER_CU                       # ... LDS for all of them (allocated in 1280-byte granules)
    # register spills of the stage functions' call frames: measured 360 B (FP64) and 400 B (FP32) per lane, k_fly's own figures
    assert k['ScratchSize'] <= scratch and k['ScratchSize'] <= fly['ScratchSize'] + 24
    assert 'k_fly' not in ks[0]                                                        # (the step kernel's name stays unique: test_build_resources)
