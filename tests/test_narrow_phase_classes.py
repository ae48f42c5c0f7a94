"""The convex narrow phase (fb_collide.hpp: mpr_penetration) on posed scenes.

In the FP64 builds the portal refinement runs its two phases in one loop with the phase as lane state, so the pairs of a pass that miss (all
their iterations in the first phase) and the pairs that penetrate (nearly all in the second) iterate side by side instead of one group after
the other.  What a pair computes must not depend on that: same portal, same directions, same support points, in the same order.  (FP32 keeps
the two loops: there the compiler contracts the loops' copies of the portal algebra differently, and one loop cannot reproduce both.)

The poses fold legs, wings and proboscis onto the body (conftest.random_state with a large joint spread, the thorax near the floor).  The
condition the poses are chosen for, and the tests assert: among their contacts, read back as geom ids through the pair table, EVERY class
combination of the model's pair table that reaches the refinement (everything except plane pairs and the closed forms sphere-sphere,
sphere-capsule, capsule-capsule) occurs at least once with positive penetration.  The poses were found on the CPU with the oracle alone.

  * CPU: the kernel source in the host emulation (one lane per pair, both shapes on the lane) against the oracle, which refines one pair at a
    time in two loops.  Tolerance: 1e-9 relative on distance, position and normal, the figure tests/test_gpu_parity.py and
    tests/test_kernel_emulation.py use for contact quantities.
  * GPU: lane pairs, one shape per lane (narrow_mpr_pair), on the default FP64 build, the 12-per-CU build and in FP32: the contact rows equal
    TO THE BIT the rows recorded on the MI355X with the libraries of the commit before the one-loop refinement (a2c4b7d;
    tests/golden/narrow_phase_contacts.npz), and the FP64 rows against the oracle at the tolerance above.

Sphere-cylinder contacts are left out of the ORACLE comparison, and only of that one: the sphere (the proboscis tip) sits at a cylinder's rim,
where the refinement's choice of the portal edge to replace hangs on the last bit of a cross product, and two compilations of the same
algorithm end on different portals.  Emulation of a2c4b7d against the oracle on such contacts: 3e-13 in some poses, 1e-2 to 2e-1 in most.
That is how the parent behaves too; the bitwise comparisons include these contacts."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, random_state

PLANE, SPHERE, CAPSULE, ELLIPSOID, CYLINDER = 0, 2, 3, 4, 5
CLOSED_FORM = {(SPHERE, SPHERE), (SPHERE, CAPSULE), (CAPSULE, CAPSULE)}
POSES = [(0, 0.5, 0.125), (0, 0.8, 0.12), (0, 1.0, 0.13), (2, 0.8, 0.12), (9, 1.0, 0.13)]      # (seed, joint spread, height of the root)
CONTACT_TOL = 1e-9
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'narrow_phase_contacts.npz')


def _classes(arrays, g1, g2):
    gt = arrays['geom_type']
    return tuple(sorted((int(gt[g1]), int(gt[g2]))))


@pytest.fixture(scope='module')
def posed(walk_arrays, oracle_model):
    """[(qpos, oracle contacts)] of the poses, computed once."""
    from oracle import fbo
    od = fbo.OracleData(oracle_model)
    out = []
    for seed, spread, z in POSES:
        q, _ = random_state(walk_arrays, np.random.default_rng(seed), spread=spread, z=z)
        od.field('qpos')[:] = q; od.field('qvel')[:] = 0; od.call('forward')
        out.append((q, od.contacts().copy()))
    return out


def _refined_combinations(arrays):
    t = {_classes(arrays, g1, g2) for g1, g2 in zip(arrays['pair_geom1'], arrays['pair_geom2'])}
    return {c for c in t if PLANE not in c and c not in CLOSED_FORM}


def test_poses_cover_every_refined_class_combination(walk_arrays, posed):
    """The reference alone: every combination of the pair table that reaches the refinement penetrates in some pose."""
    want = _refined_combinations(walk_arrays)
    assert {(ELLIPSOID, ELLIPSOID), (CAPSULE, ELLIPSOID), (CAPSULE, CYLINDER), (ELLIPSOID, CYLINDER)} <= want
    got = set()
    for _, con in posed:
        assert 0 < len(con) < 64                                    # (the contact cap would hide contacts)
        got |= {_classes(walk_arrays, int(c[7]), int(c[8])) for c in con if c[0] < -1e-6}
    missing = sorted(want - got)
    assert not missing, 'class combinations without a penetrating contact: %s' % missing


def _forward(batch, arrays, posed):
    q = np.array([p for p, _ in posed])
    batch.set('QPOS', q); batch.set('QVEL', np.zeros((len(posed), len(arrays['dof_bodyid'])))); batch.forward(); batch.synchronize()
    return batch.get('NCON').copy(), batch.get('CONTACT').copy(), batch.get('WARN').copy()


def _check_against_oracle(ncon, contact, warn, arrays, posed):
    ncon = ncon.ravel(); con = contact.reshape(len(posed), 64, 8)
    assert (warn == 0).all()
    seen = set()
    for e, (_, oc) in enumerate(posed):
        assert int(ncon[e]) == len(oc), (e, int(ncon[e]), len(oc))
        gc = con[e, :len(oc)]
        pair = gc[:, 7].astype(int)
        g1, g2 = arrays['pair_geom1'][pair], arrays['pair_geom2'][pair]
        assert np.array_equal(g1, oc[:, 7].astype(int)) and np.array_equal(g2, oc[:, 8].astype(int)), e
        cls = [_classes(arrays, a, b) for a, b in zip(g1, g2)]
        keep = np.array([c != (SPHERE, CYLINDER) for c in cls])     # (see the module's docstring)
        err = np.abs(gc[keep, :7] - oc[keep, :7]).max()/np.abs(oc[keep, :7]).max()
        print('pose %d: %d contacts (%d compared), relative error %.2e' % (e, len(oc), int(keep.sum()), err))
        assert err < CONTACT_TOL, (e, err)
        seen |= {c for c, row in zip(cls, gc) if row[0] < -1e-6}
    assert _refined_combinations(arrays) <= seen


def test_emulation_contacts_match_the_oracle(walk_arrays, posed):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    from flybody_amd import engine
    M = engine.Model(walk_arrays, lib_path=g.build_emu())
    _check_against_oracle(*_forward(engine.Batch(M, len(posed), precision=64), walk_arrays, posed), walk_arrays, posed)


@pytest.mark.gpu
@pytest.mark.parametrize('build,dense,precision', [('default64', False, 64), ('dense64', True, 64), ('default32', False, 32)])
def test_gpu_contacts_equal_the_recorded_rows(walk_arrays, posed, build, dense, precision):
    from flybody_amd import engine
    M = engine.Model.from_asset('walk_imitation', dense=dense)
    ncon, contact, warn = _forward(engine.Batch(M, len(posed), device=0, precision=precision), walk_arrays, posed)
    gold = np.load(GOLDEN)
    assert np.array_equal(ncon, gold['ncon_' + build]) and np.array_equal(warn, gold['warn_' + build])
    assert np.array_equal(contact, gold['contact_' + build]), build
    if precision == 64:
        _check_against_oracle(ncon, contact, warn, walk_arrays, posed)
