"""Residency of the ray-casting kernel (csrc/fb_ray.hpp: k_raycast), read from the compiler's kernel-resource-usage remarks of
the one compilation __graft_entry__.build_hip() stores under tests/_emu (no GPU needed).

The first clean build gave: FP64 124 VGPRs, 0 AGPRs, no scratch, 13 056 B of LDS (96 records of 136 B), 4 waves per SIMD; FP32 71 VGPRs, no
scratch, 6 912 B (96 x 72 B), 7 waves per SIMD.  Pinned as the other resource tests pin: the register granule the build sits in (128 resp. 72 VGPRs) and its waves per SIMD (4 resp. 7)."""
from test_build_resources import LDS_PER_CU, usage  # noqa: F401  (the remark parser is a fixture of that module)

CHUNK = 96                      # FB_RAY_CHUNK


def _one(usage, tag):  # noqa: F811
    ks = [k for k in usage if 'k_raycast' in k and tag in k]
    assert len(ks) == 1, list(usage)
    return usage[ks[0]]


def test_one_ray_kernel_per_precision(usage):  # noqa: F811
    assert len([k for k in usage if 'k_raycast' in k]) == 2
    _one(usage, 'k_raycastId'); _one(usage, 'k_raycastIf')


def test_fp64_ray_kernel(usage):  # noqa: F811
    k = _one(usage, 'k_raycastId')
    assert k['ScratchSize'] == 0 and k['AGPRs'] == 0                    # a lane's ray, its best hit and the terrain walk live in registers
    assert k['LDS Size'] == CHUNK*(16*8 + 8)                            # the staged geoms and nothing else
    assert k['VGPRs'] <= 128 and k['Occupancy'] == 4
    assert 8*k['LDS Size'] <= LDS_PER_CU                                # LDS never limits the 8 workgroups per CU the waves allow


def test_fp32_ray_kernel(usage):  # noqa: F811
    k = _one(usage, 'k_raycastIf')
    assert k['ScratchSize'] == 0 and k['AGPRs'] == 0
    assert k['LDS Size'] == CHUNK*(16*4 + 8)
    assert k['VGPRs'] <= 72 and k['Occupancy'] == 7
