"""Residency of the inverse-kinematics kernel k_ik (csrc/fb_ik.hpp), read from the compiler's kernel-resource-usage remarks
that __graft_entry__.build_hip() stores under tests/_emu (no GPU needed)."""
from test_build_resources import LDS_PER_CU, usage  # noqa: F401  (the remark parser is a fixture of that module)


def test_ik_kernel_residency(usage):  # noqa: F811
    ks = [k for k in usage if 'k_ik' in k]
    assert len(ks) == 1, list(usage)
    k = usage[ks[0]]
    assert k['Occupancy'] == 2 and k['VGPRs'] <= 256                     # 2 waves per SIMD = 8 frames per CU
    assert k['LDS Size'] == 1536*8                                       # FB_IK_POOL FP64 reals per frame, one frame per workgroup
    assert 8*(-(-k['LDS Size'] // 1280)*1280) <= LDS_PER_CU              # ... LDS for all 8 (allocated in 1280-byte granules)
    assert k['ScratchSize'] <= 256                                       # register spills of the position stages at 256 VGPRs (measured 208)
