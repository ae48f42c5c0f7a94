"""Residency of the closed-loop rollout kernel k_closedloop_rollout (csrc/fb_rollout.hpp) beside k_rollout's, both read
from the compiler's kernel-resource-usage remarks of ONE compilation, which __graft_entry__.build_hip() stores under tests/_emu (no GPU
needed)."""
from test_build_resources import LDS_PER_CU, usage  # noqa: F401  (the remark parser is a fixture of that module)


def test_closed_loop_rollout_kernel_residency(usage):  # noqa: F811
    ks = [k for k in usage if 'k_closedloop_rollout' in k]
    assert len(ks) == 1, list(usage)
    k = usage[ks[0]]
    fly = usage[[n for n in usage if 'k_flyId' in n][0]]
    roll = usage[[n for n in usage if 'k_rolloutId' in n][0]]
    assert k['LDS Size'] == fly['LDS Size'] == roll['LDS Size']               # the step kernel's LDS layout and nothing beside it: dx lives in registers
    assert k['Occupancy'] == fly['Occupancy'] == 2 and k['VGPRs'] <= 256      # what the launch bounds ask for: 2 waves per SIMD = 8 rollouts in flight per CU
    assert 8*(-(-k['LDS Size'] // 1280)*1280) <= LDS_PER_CU
    assert k['ScratchSize'] <= roll['ScratchSize']                            # the feedback stage is a call like the others: the kernel's frame does not grow
