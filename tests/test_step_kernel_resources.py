"""Residency of the step kernels beside k_fly (fb_engine.hip: step_kernels() and the grouped reset), read from the
compiler's kernel-resource-usage remarks that __graft_entry__.build_hip() stores under tests/_emu (no GPU needed): k_fly's occupancy
and LDS layout at both precisions -- the resident-slot count, and with it the choice of scheduler, is the plain batch's -- registers
within the budget, scratch pinned at what the build reports."""
from test_build_resources import LDS_PER_CU, usage  # noqa: F401  (the remark parser is a fixture of that module)
import pytest

# Scratch is the register spills of the stage functions' call frames, per lane.
#   k_step_forces: measured 360 B (FP64) and 400 B (FP32), k_fly's own figures; at most 24 B over k_fly.
#   k_step_law: measured 376 B and 416 B, 16 B over k_step_forces (360 / 400); at most 24 B over it.
#   k_group_step / k_group_reset: the build reports 360 B and 368 B for the step kernels, 296 B and 320 B for the reset -- no more than
#   the plain kernel of the same kind (360 / 400, 296 / 352).
# (kernel, the kernel it is compared against, waves per SIMD, VGPR budget, workgroups per CU in the default build, absolute scratch
#  bound or None, scratch allowed over the comparison kernel, names that must not occur in the kernel's: the other step kernels' names
#  stay unique, test_build_resources)
KERNELS = [
    ('k_step_forcesId', 'k_flyId', 2, 256, 8, 384, 24, ('k_fly',)),
    ('k_step_forcesIf', 'k_flyIf', 4, 128, 4, 424, 24, ('k_fly',)),
    ('k_step_lawId', 'k_step_forcesId', 2, 256, 8, None, 24, ('k_fly', 'k_step_forces')),
    ('k_step_lawIf', 'k_step_forcesIf', 4, 128, 4, None, 24, ('k_fly', 'k_step_forces')),
    ('k_group_stepIdLb0E', 'k_flyId', 2, 256, 8, 360, 0, ('k_fly',)),
    ('k_group_stepIdLb1E', 'k_flyId', 2, 256, 8, 360, 0, ('k_fly',)),
    ('k_group_stepIfLb0E', 'k_flyIf', 4, 128, 4, 368, 0, ('k_fly',)),
    ('k_group_stepIfLb1E', 'k_flyIf', 4, 128, 4, 368, 0, ('k_fly',)),
    ('k_group_resetId', 'k_fly_resetId', 2, 256, 8, 296, 0, ('k_fly',)),
    ('k_group_resetIf', 'k_fly_resetIf', 4, 128, 4, 320, 0, ('k_fly',)),
]


@pytest.mark.parametrize('tag,ref_tag,occupancy,vgprs,groups,scratch,over_ref,foreign', KERNELS, ids=[k[0] for k in KERNELS])
def test_step_kernel_residency(usage, tag, ref_tag, occupancy, vgprs, groups, scratch, over_ref, foreign):  # noqa: F811
    ks = [k for k in usage if tag in k]
    assert len(ks) == 1, list(usage)
    k = usage[ks[0]]
    ref = usage[[n for n in usage if ref_tag in n][0]]
    fly = usage[[n for n in usage if 'k_fly' + ('Id' if 'Id' in tag else 'If') in n][0]]     # the layout's owner, same precision
    for other in (ref, fly):
        assert k['Occupancy'] == occupancy == other['Occupancy']                       # k_fly's launch bounds
        assert k['LDS Size'] == other['LDS Size']                                      # k_fly's LDS layout: pool + tree tables, EPB environments
    assert k['VGPRs'] <= vgprs
    assert groups*(-(-k['LDS Size'] // 1280)*1280) <= LDS_PER_CU                       # ... LDS for all of them (allocated in 1280-byte granules)
    assert scratch is None or k['ScratchSize'] <= scratch
    assert k['ScratchSize'] <= ref['ScratchSize'] + over_ref
    assert not [name for name in foreign if name in ks[0]]
