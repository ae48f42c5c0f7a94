"""Residency of the kernels beside k_fly that run in its frame (csrc/fb_side.hpp), read from the compiler's
kernel-resource-usage remarks of ONE compilation, which __graft_entry__.build_hip() stores under tests/_emu (no GPU needed): the step
kernel's launch bounds -- 2 waves per SIMD = 8 frames, tickets or rollouts in flight per CU -- and its LDS layout, one pool + the tree
tables per wave and nothing beside it.  (k_ik has a layout of its own: tests/test_ik_resources.py.)"""
from test_build_resources import LDS_PER_CU, usage  # noqa: F401  (the remark parser is a fixture of that module)
import pytest

# Scratch is the register spills of the shared stages' call frames, per lane.
#   k_inverse: measured 296 B.
#   k_transition_fd: 344 B at the first clean build, rounded up to the next 32 bytes.
#   k_rollout: 376 B at the first clean build, rounded up to the next 32 bytes.
#   k_closedloop_rollout: the feedback stage is a call like the others, the kernel's frame does not grow: no more than k_rollout's.
# (kernel, absolute scratch bound or None, the kernel whose scratch it must not exceed or None)
KERNELS = [
    ('k_inverse', 320, None),
    ('k_transition_fd', 352, None),
    ('k_rollout', 384, None),
    ('k_closedloop_rollout', None, 'k_rolloutId'),
]


def _one(usage, tag):  # noqa: F811
    ks = [k for k in usage if tag in k]
    assert len(ks) == 1, list(usage)
    return usage[ks[0]]


@pytest.mark.parametrize('tag,scratch,not_over', KERNELS, ids=[k[0] for k in KERNELS])
def test_side_kernel_residency(usage, tag, scratch, not_over):  # noqa: F811
    k = _one(usage, tag)
    fly = _one(usage, 'k_flyId')
    assert k['Occupancy'] == fly['Occupancy'] == 2 and k['VGPRs'] <= 256      # the step kernel's launch bounds
    assert k['LDS Size'] == fly['LDS Size']                                   # the step kernel's LDS layout (closed loop: dx lives in registers)
    assert 8*(-(-k['LDS Size'] // 1280)*1280) <= LDS_PER_CU                   # ... LDS for all 8 (allocated in 1280-byte granules)
    assert scratch is None or k['ScratchSize'] <= scratch
    if not_over:
        other = _one(usage, not_over)
        assert k['LDS Size'] == other['LDS Size'] and k['ScratchSize'] <= other['ScratchSize']


def test_assemble_kernel_is_light(usage):  # noqa: F811
    k = _one(usage, 'k_fd_assemble')
    assert k['LDS Size'] == 0 and k['ScratchSize'] == 0
