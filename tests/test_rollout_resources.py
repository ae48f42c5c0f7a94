"""Residency of the rollout kernel k_rollout (csrc/fb_rollout.hpp), read from the compiler's kernel-resource-usage
remarks that __graft_entry__.build_hip() stores under tests/_emu (no GPU needed)."""
from test_build_resources import LDS_PER_CU, usage  # noqa: F401  (the remark parser is a fixture of that module)


def test_rollout_kernel_residency(usage):  # noqa: F811
    ks = [k for k in usage if 'k_rollout' in k]
    assert len(ks) == 1, list(usage)
    k = usage[ks[0]]
    fly = usage[[n for n in usage if 'k_flyId' in n][0]]
    assert k['Occupancy'] == fly['Occupancy'] == 2 and k['VGPRs'] <= 256      # the step kernel's launch bounds: 2 waves per SIMD = 8 rollouts in flight per CU
    assert k['LDS Size'] == fly['LDS Size']                                   # the step kernel's LDS layout: one pool + the tree tables per wave
    assert 8*(-(-k['LDS Size'] // 1280)*1280) <= LDS_PER_CU                   # ... LDS for all 8 (allocated in 1280-byte granules)
    assert k['ScratchSize'] <= 384                                            # spills of the shared stages' call frames: 376 at the first clean build, rounded up to the next 32 bytes
