"""The gfx950 build keeps the residency the design relies on: read from the compiler's own
kernel-resource-usage remarks, which __graft_entry__.build_hip() stores next to the emulation build (no GPU needed)."""
import re

import pytest

LDS_PER_CU = 163840


@pytest.fixture(scope='module')
def usage():
    import __graft_entry__ as g
    g.build_hip()
    out, cur = {}, None
    for line in open(g.HIP_RES):
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            cur = m.group(1); out[cur] = {}
            continue
        m = re.search(r'remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)', line)
        if m and cur:
            out[cur][m.group(1).strip()] = int(m.group(2))
    return out


def _kernel(usage, tag):
    ks = [k for k in usage if 'k_fly' in k and tag in k]
    assert len(ks) == 1, list(usage)
    return usage[ks[0]]


def test_fp32_kernel_residency(usage):
    k = _kernel(usage, 'k_flyIf')
    assert k['VGPRs'] <= 128 and k['Occupancy'] == 4                     # 4 waves per SIMD = 16 environments per CU
    assert 4 * (-(-k['LDS Size'] // 1280) * 1280) <= LDS_PER_CU          # 4 workgroups of 4 environments
    assert k['ScratchSize'] <= 1024                                      # register spills only: no pointer tables in scratch


def test_fp64_kernel_residency(usage):
    k = _kernel(usage, 'k_flyId')
    assert k['VGPRs'] <= 256 and k['Occupancy'] == 2                     # 2 waves per SIMD = 8 environments per CU
    assert 8 * (-(-k['LDS Size'] // 1280) * 1280) <= LDS_PER_CU          # 8 single-environment workgroups, LDS allocated in granules (<= 1280 B)
    assert k['ScratchSize'] <= 1536


def test_order_kernel_is_tiny(usage):
    ks = [k for k in usage if 'k_order' in k]
    assert len(ks) == 1 and usage[ks[0]]['LDS Size'] <= 4096 and usage[ks[0]]['ScratchSize'] == 0


def test_build_flags_are_part_of_the_source_hash():
    """The engine's extra compiler flags live in csrc/fb_build_flags.h: every build recipe reads them from there, and the file is
    hashed with the sources, so a library built with other flags is rebuilt (its embedded hash no longer matches)."""
    import os
    import __graft_entry__ as g
    from flybody_amd import engine
    flags = g.hip_flags()
    assert flags and all(isinstance(f, str) for f in flags)
    path = os.path.join(g.ROOT, 'flybody_amd', 'csrc', 'fb_build_flags.h')
    assert ' '.join(flags) in open(path).read()
    assert path in g._csrc()                                              # hashed by engine.source_hash()
    for script in ('tools/build_variant.sh', 'tools/build_profile_lib.sh'):
        assert 'fb_build_flags.h' in open(os.path.join(g.ROOT, script)).read()
    assert len(engine.source_hash()) == 12


# The engine's kernel sources and the FB_* names their preprocessor conditionals may test: the ones a committed build, test or tool sets
# (__graft_entry__.py: FB_F64_DENSE, FB_EMULATE, FB_BUILD_ID; tools/build_profile_lib.sh: FB_PROFILE; tools/collision_stats.py: FB_STATS;
# tests/test_kernel_emulation.py: FB_SCHED_SPIN_CAP), FB_MPR_PAIRED (derived from FB_EMULATE in fb_collide.hpp) and FB_TICKET_SPLIT (0:
# folding its arithmetic changes k_fly's code).  A new switch lands together with the build, test or tool that sets it.
ENGINE_KERNEL_SOURCES = ('fb_collide.hpp', 'fb_constraint.hpp', 'fb_math.hpp', 'fb_newton.hpp', 'fb_smooth.hpp', 'fb_step.hpp', 'fb_types.hpp',
                         'fb_ik.hpp', 'fb_inverse.hpp', 'fb_forces.hpp', 'fb_law.hpp', 'fb_task.hpp', 'fb_host.hpp', 'fb_model.hpp', 'fb_engine.hip')
KEPT_SWITCHES = {'FB_EMULATE', 'FB_PROFILE', 'FB_STATS', 'FB_F64_DENSE', 'FB_SCHED_SPIN_CAP', 'FB_BUILD_ID', 'FB_MPR_PAIRED', 'FB_TICKET_SPLIT'}


def test_kernel_sources_test_only_switches_a_build_sets():
    import os
    import __graft_entry__ as g
    found = {}
    for name in ENGINE_KERNEL_SOURCES:
        for n, line in enumerate(open(os.path.join(g.ROOT, 'flybody_amd', 'csrc', name)), 1):
            m = re.match(r'\s*#\s*(if|ifdef|ifndef|elif)\b(.*)', line)
            if m:
                for sw in re.findall(r'\bFB_\w+', m.group(2)):
                    found.setdefault(sw, []).append('%s:%d' % (name, n))
                if m.group(1) == 'ifndef':
                    assert 'FB_MPR_PAIRED' not in m.group(2), '%s:%d: FB_MPR_PAIRED follows FB_EMULATE, it is not overridable' % (name, n)
    assert 'FB_EMULATE' in found and 'FB_PROFILE' in found
    stray = {sw: where for sw, where in found.items() if sw not in KEPT_SWITCHES}
    assert not stray, 'switches no build, test or tool sets: %s' % stray
