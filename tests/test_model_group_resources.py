"""Residency of the grouped batch's kernels k_group_step / k_group_reset (fb_engine.hip), read from the compiler's
kernel-resource-usage remarks that __graft_entry__.build_hip() stores under tests/_emu (no GPU needed): k_fly's occupancy and LDS
layout at both precisions -- the resident-slot count, and with it the choice of scheduler, is the plain batch's -- and scratch pinned
at what the build reports."""
from test_build_resources import LDS_PER_CU, usage  # noqa: F401  (the remark parser is a fixture of that module)
import pytest


# (kernel, its k_fly, waves per SIMD, VGPR budget, workgroups per CU in the default build, scratch the build reports)
@pytest.mark.parametrize('tag,fly_tag,occupancy,vgprs,groups,scratch', [
    ('k_group_stepIdLb0E', 'k_flyId', 2, 256, 8, 360), ('k_group_stepIdLb1E', 'k_flyId', 2, 256, 8, 360),
    ('k_group_stepIfLb0E', 'k_flyIf', 4, 128, 4, 368), ('k_group_stepIfLb1E', 'k_flyIf', 4, 128, 4, 368),
    ('k_group_resetId', 'k_fly_resetId', 2, 256, 8, 296), ('k_group_resetIf', 'k_fly_resetIf', 4, 128, 4, 320)])
def test_group_kernel_residency(usage, tag, fly_tag, occupancy, vgprs, groups, scratch):  # noqa: F811
    ks = [k for k in usage if tag in k]
    assert len(ks) == 1, list(usage)
    k = usage[ks[0]]
    fly = usage[[n for n in usage if fly_tag in n][0]]
    assert k['Occupancy'] == occupancy == fly['Occupancy'] and k['VGPRs'] <= vgprs       # k_fly's launch bounds
    assert k['LDS Size'] == fly['LDS Size']                                            # k_fly's LDS layout: pool + tree tables, EPB environments
    assert groups*(-(-k['LDS Size'] // 1280)*1280) <= LDS_PER_CU                       # ... LDS for all of them (allocated in 1280-byte granules)
    # register spills of the stage functions' call frames, per lane: the build reports 360 B (FP64) and 368 B (FP32) for the step kernels,
    # 296 B and 320 B for the reset -- no more than the plain kernel of the same kind (360 / 400, 296 / 352)
    assert k['ScratchSize'] <= scratch and k['ScratchSize'] <= fly['ScratchSize']
    assert 'k_fly' not in ks[0]                                                        # (the step kernel's name stays unique: test_build_resources)
