"""Substep control laws (csrc/fb_law.hpp, the step kernel k_step_law, fb_batch_set_control_law) through the kernel-source emulation
build.  The oracle knows no law, so parity is reached through identities (tests/law_helpers.py): a zero law is the forces kernel, the
acceleration-level identity with the oracle's mass matrix, a position law against an oracle with stiffer joints, an actuator gain against
an oracle with stronger motors, a bias against qfrc_applied, and the reference's control-callback test written as a law.  No GPU needed."""
import sys

import numpy as np
import pytest

from conftest import ROOT
import law_helpers as H
from law_helpers import rel

# the bounds of tests/test_kernel_emulation.py (states after control steps) and of tests/test_forces_emulation.py (M dqacc against the oracle)
TOL_QPOS, TOL_QVEL, TOL_JAC = 1e-9, 1e-8, 5.86e-13


@pytest.fixture(scope='module')
def emu_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    return g.build_emu()


@pytest.fixture(scope='module')
def emu_model(walk_arrays, emu_lib):
    from flybody_amd import engine
    return engine.Model(walk_arrays, lib_path=emu_lib)


def _hinge(arrays):
    return np.asarray(arrays['jnt_type'])[np.asarray(arrays['dof_jntid'])] == 3


def _random_law(arrays, rng, n_rows=None, scale=1.0):
    """All four terms random, of the size of the model's own spring / damper / actuator constants."""
    nv = len(arrays['dof_jntid']); shape = (nv,) if n_rows is None else (n_rows, nv)
    k = float(np.median(arrays['jnt_stiffness'][arrays['jnt_stiffness'] > 0])); d = float(np.median(arrays['dof_damping'][arrays['dof_damping'] > 0]))
    return dict(bias=rng.normal(size=shape)*k*0.1*scale, act_gain=rng.uniform(-0.5, 0.5, shape)*scale, pos_gain=rng.uniform(0, 2*k, shape)*_hinge(arrays)*scale,
                pos_ref=rng.uniform(-0.3, 0.3, shape), vel_gain=rng.uniform(0, 2*d, shape)*scale)


def _law_force(arrays, law, q, v, fa, row=None):
    """The formula on the host."""
    r = {k: (x if row is None or np.ndim(x) == 1 else x[row]) for k, x in law.items()}
    qa = np.asarray(arrays['jnt_qposadr'])[np.asarray(arrays['dof_jntid'])]
    return r['bias'] + r['act_gain']*fa - r['pos_gain']*(q[qa] - r['pos_ref']) - r['vel_gain']*v


def test_zero_law_equals_the_forces_kernel_and_the_plain_kernel(emu_lib, walk_arrays, reference_traj, monkeypatch):
    """(a) An all-zero law: every output of six control steps through an auto-reset equals k_step_forces' with zero forces and k_fly's,
    under the substep scheduler and with one environment per wave; clearing the law returns the batch to k_fly."""
    from flybody_amd import engine
    qp, qv = reference_traj
    acts = np.random.default_rng(9).uniform(-1, 1, (7, 5, 59)).astype(np.float32)
    fields = ('QPOS', 'QVEL', 'OBS', 'REWARD', 'DISCOUNT', 'STEP_TYPE', 'QACC', 'SENSORDATA')
    for flag in (None, '1'):
        if flag is None: monkeypatch.delenv('FB_NO_TICKETS', raising=False)
        else: monkeypatch.setenv('FB_NO_TICKETS', flag)
        M = engine.Model(walk_arrays, lib_path=emu_lib)
        P, F, L = (engine.Batch(M, 5, precision=64) for _ in range(3))
        assert L.substep_scheduler == (flag is None)
        F.set('XFRC_APPLIED', 0.0)
        assert not L.control_law_active and not L.forces_active
        L.set_control_law()
        assert L.control_law_active and L.forces_active and not F.control_law_active
        for B in (P, F, L):
            B.set_reference(qp[:8], qv[:8], future_steps=2, terminal_com_dist=float('inf')); B.reset()
        types = []
        for k in range(6):
            a = np.ascontiguousarray(acts[k])
            for B in (P, F, L):
                B.step_ptr(a.ctypes.data)
            for name in fields:
                assert np.array_equal(F.get(name), L.get(name)) and np.array_equal(P.get(name), L.get(name)), (flag, k, name)
            assert not L.get('QFRC_LAW').any()
            types.append(L.get('STEP_TYPE').ravel())
        types = np.array(types)
        assert (types == 2).any() and (types == 0).any()
        L.clear_control_law()                                                # the law allocated the force arrays itself: back on k_fly
        assert not L.control_law_active and not L.forces_active
        with pytest.raises(engine.EngineError, match='no control law'):
            L.get('QFRC_LAW')
        a = np.ascontiguousarray(acts[6])
        P.step_ptr(a.ctypes.data); L.step_ptr(a.ctypes.data)
        for name in fields:
            assert np.array_equal(P.get(name), L.get(name)), (flag, 'cleared', name)
        # a law set on a batch whose forces the caller touched leaves them where they are when it goes
        F.set_control_law(); F.clear_control_law()
        assert F.forces_active
        del P, F, L, M


def test_acceleration_level_identity(emu_model, oracle_model, walk_arrays, reference_traj):
    """(b) M (qacc_smooth with - without the law) = u with the oracle's mul_m, all four terms random, at a state with contacts, motion and
    actuator forces; FB_QFRC_LAW is the formula evaluated on the host from fb_batch_forward's fields."""
    from flybody_amd import engine
    from oracle import fbo
    qp, qv = reference_traj
    B = engine.Batch(emu_model, 1, precision=64)
    B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    rng = np.random.default_rng(21)
    for _ in range(4):
        a = rng.uniform(-0.6, 0.6, (1, 59)).astype(np.float32); B.step_ptr(a.ctypes.data)
    assert int(B.get('NCON')[0, 0]) > 0
    B.forward()
    q, v, fa = B.get('QPOS')[0].copy(), B.get('QVEL')[0].copy(), B.get('QFRC_ACTUATOR')[0].copy()
    without = B.get('QACC_SMOOTH')[0].copy()
    assert np.abs(fa).max() > 0 and np.abs(v).max() > 0
    law = _random_law(walk_arrays, rng)
    B.set_control_law(**law)
    B.forward()
    u = B.get('QFRC_LAW')[0].copy()
    expect = _law_force(walk_arrays, law, q, v, fa)
    assert np.array_equal(B.get('QFRC_ACTUATOR')[0], fa)                     # the actuators' own force stays what it was
    assert rel(u, expect) < 1e-14
    terms = [law['bias'], law['act_gain']*fa, law['pos_gain'], law['vel_gain']*v]
    assert all(np.abs(t).max() > 1e-3*np.abs(u).max() for t in terms)          # every term takes part
    od = fbo.OracleData(oracle_model)
    od.field('qpos')[:] = q; od.field('qvel')[:] = v; od.call('forward')
    gap = rel(od.mul_m(B.get('QACC_SMOOTH')[0] - without), expect)
    print('law: M dqacc_smooth vs u: relative gap %.3g; FB_QFRC_LAW vs the formula %.3g' % (gap, rel(u, expect)))
    assert gap < TOL_JAC


@pytest.mark.parametrize('which', ['stiffness', 'motors'])
def test_law_against_an_oracle_with_changed_constants(emu_lib, which):
    """(c) pos_gain = 0.5 jnt_stiffness with pos_ref = qpos_spring, plus a spring on two hinges that have none, against an oracle whose
    jnt_stiffness says the same; (d) act_gain = 0.2 on every dof against an oracle whose gains, biases and force ranges are x 1.2
    (law_helpers.motor_pair: exact for every actuator, adhesion included).  Three control steps; without the law the engine does not
    follow that oracle."""
    pair = H.stiffness_pair() if which == 'stiffness' else H.motor_pair()
    eq, ev = H.law_rollout(emu_lib, pair, 2, 3, on_gpu=False)
    nq, nv_ = H.law_rollout(emu_lib, pair, 1, 3, on_gpu=False, with_law=False)
    print('%s identity, 3 control steps: qpos %.2e qvel %.2e (without the law: %.2e %.2e)' % (which, eq, ev, nq, nv_))
    assert eq < TOL_QPOS and ev < TOL_QVEL
    assert nq > 1e-4 and nv_ > 1e-3


def test_bias_equals_qfrc_applied(emu_model, reference_traj, walk_arrays):
    """(e) bias = c is QFRC_APPLIED = c."""
    from flybody_amd import engine
    qp, qv = reference_traj
    rng = np.random.default_rng(5)
    c = rng.normal(size=(2, 108))*1e-3
    A, L, Z = (engine.Batch(emu_model, 2, precision=64) for _ in range(3))
    A.set('QFRC_APPLIED', c); L.set_control_law(bias=c)
    for B in (A, L, Z):
        B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    for k in range(3):
        a = rng.uniform(-0.5, 0.5, (2, 59)).astype(np.float32)
        for B in (A, L, Z):
            B.step_ptr(a.ctypes.data)
    gq, gv = rel(L.get('QPOS'), A.get('QPOS')), rel(L.get('QVEL'), A.get('QVEL'))
    print('bias vs qfrc_applied: qpos %.2e qvel %.2e' % (gq, gv))
    assert gq < 1e-13 and gv < 1e-13
    assert np.array_equal(L.get('QFRC_LAW'), c)
    assert rel(Z.get('QVEL'), A.get('QVEL')) > 1e-6                          # (the force matters: the plain batch is elsewhere)


def test_reference_ctrl_callback_as_a_law(emu_model, reference_traj):
    """(f) The reference's test_ctrl_callback (tests/test_core.py:72-100): qfrc_applied[dofs] = qfrc_actuator[dofs] * sin(arange(29)).
    After each of 20 control steps FB_QFRC_LAW equals FB_QFRC_ACTUATOR * noise there and is zero elsewhere."""
    from flybody_amd import engine
    from flybody_amd.control_laws import ControlLaw
    noise = np.sin(np.arange(len(H.CALLBACK_DOFS)))
    law = ControlLaw.from_dofs(emu_model, H.CALLBACK_DOFS, act_gain=noise)
    comp = [i for i in range(108) if i not in H.CALLBACK_DOFS]
    qp, qv = reference_traj
    B = engine.Batch(emu_model, 1, precision=64)
    B.set_control_law(**law.rows())
    B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    assert not B.get('QFRC_LAW').any()
    rng = np.random.default_rng(0)
    for _ in range(20):
        a = rng.uniform(-1, 1, (1, 59)).astype(np.float32); B.step_ptr(a.ctypes.data)
        u, fa = B.get('QFRC_LAW')[0], B.get('QFRC_ACTUATOR')[0]
        assert np.abs(fa[H.CALLBACK_DOFS]).max() > 0
        assert np.allclose(u[H.CALLBACK_DOFS], fa[H.CALLBACK_DOFS]*noise, rtol=1e-14, atol=0)
        assert (u[comp] == 0).all()


def test_a_partial_reset_zeroes_the_law_force_of_its_environments(emu_model, reference_traj):
    """fb_batch_reset of some environments skips the law for them and leaves their FB_QFRC_LAW rows zero; the others keep theirs."""
    from flybody_amd import engine
    qp, qv = reference_traj
    B = engine.Batch(emu_model, 4, precision=64)
    B.set_control_law(act_gain=np.full(108, 0.1), bias=np.full(108, 1e-4))
    B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    a = np.random.default_rng(3).uniform(-0.5, 0.5, (4, 59)).astype(np.float32)
    B.step_ptr(a.ctypes.data)
    before = B.get('QFRC_LAW').copy()
    assert (np.abs(before).max(1) > 0).all()
    B.reset([2, 0])
    after = B.get('QFRC_LAW')
    assert not after[[0, 2]].any() and np.array_equal(after[[1, 3]], before[[1, 3]])
    assert B.get('STEP_TYPE').ravel().tolist() == [0, 1, 0, 1]
    B.reset()
    assert not B.get('QFRC_LAW').any()
    # a second law of another row count replaces the first; the batch stays on the law kernel throughout
    B.set_control_law(bias=np.full((4, 108), 2e-4)); assert B.control_law_active and B.control_law_rows == 4
    B.step_ptr(a.ctypes.data)
    assert (B.get('QFRC_LAW') == 2e-4).all()


def test_per_environment_rows(emu_model, walk_arrays, reference_traj):
    """(g) One law per environment equals five batches of one environment with one law each, to the bit."""
    from flybody_amd import engine
    qp, qv = reference_traj
    rng = np.random.default_rng(8)
    law = _random_law(walk_arrays, rng, n_rows=5, scale=0.3)
    acts = rng.uniform(-0.5, 0.5, (3, 5, 59)).astype(np.float32)
    B = engine.Batch(emu_model, 5, precision=64)
    B.set_control_law(**law); assert B.control_law_rows == 5
    B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    for k in range(3):
        a = np.ascontiguousarray(acts[k]); B.step_ptr(a.ctypes.data)
    for e in range(5):
        S = engine.Batch(emu_model, 1, precision=64)
        S.set_control_law(**{k: x[e] for k, x in law.items()}); assert S.control_law_rows == 1
        S.set_reference(qp, qv, terminal_com_dist=float('inf')); S.reset()
        for k in range(3):
            a = np.ascontiguousarray(acts[k][e:e + 1]); S.step_ptr(a.ctypes.data)
        for name in ('QPOS', 'QVEL', 'QFRC_LAW', 'OBS'):
            assert np.array_equal(S.get(name)[0], B.get(name)[e]), (e, name)
    assert not np.array_equal(B.get('QVEL')[0], B.get('QVEL')[1])


def test_refusals_and_validation(emu_model, emu_lib, walk_arrays, reference_traj):
    """(h)"""
    import ctypes as C
    from flybody_amd import engine
    qp, qv = reference_traj
    nv = 108
    B = engine.Batch(emu_model, 3, precision=64)
    # pos_gain on a dof that is no hinge's: the free root
    pg = np.zeros(nv); pg[4] = 1.0
    with pytest.raises(engine.EngineError, match='pos_gain of dof 4 .*free joint'):
        B.set_control_law(pos_gain=pg)
    bad = np.zeros((3, nv)); bad[2, 7] = np.nan
    with pytest.raises(engine.EngineError, match=r'vel_gain of dof 7 \(row 2\) is not finite'):
        B.set_control_law(vel_gain=bad)
    assert not B.control_law_active and not B.forces_active               # a rejected law allocates nothing
    law = engine._ControlLaw(None, None, None, None, None, 2)
    with pytest.raises(engine.EngineError, match='n_rows must be 1 .* or n_env = 3'):
        engine._check(B.L, B.L.fb_batch_set_control_law(B.h, C.byref(law)))
    with pytest.raises(ValueError, match='control law row bias'):
        B.set_control_law(bias=np.zeros((2, nv)))
    with pytest.raises(engine.EngineError, match='null batch'):
        engine._check(B.L, B.L.fb_batch_set_control_law(None, None))
    # walk_on_ball: the ball's dofs are no hinge's either
    ball = dict(engine.load_npz(engine.os.path.join(engine.ASSETS, 'walk_on_ball.npz')))
    Mb = engine.Model(ball, lib_path=emu_lib); Bb = engine.Batch(Mb, 1, precision=64)
    nvb = Mb.dim('nv'); pgb = np.zeros(nvb); pgb[nvb - 1] = 2.0
    with pytest.raises(engine.EngineError, match='pos_gain of dof %d .*ball joint' % (nvb - 1)):
        Bb.set_control_law(pos_gain=pgb)
    # a grouped batch
    G = engine.Batch(engine.ModelGroup([walk_arrays, walk_arrays], lib_path=emu_lib), 2, precision=64)
    with pytest.raises(engine.EngineError, match='grouped batch.*fb_batch_create'):
        G.set_control_law()
    # stage / ik / inverse / clear_forces while a law is set
    B.set_control_law(vel_gain=np.full(nv, 1e-6))
    B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    a = np.zeros((3, 59), np.float32)
    for call in (lambda: B.stage(engine.ST['PRE'], a.ctypes.data), lambda: B.ik([0], [], np.zeros((3, 1, 3))), lambda: B.inverse(), lambda: B.clear_forces()):
        with pytest.raises(engine.EngineError, match=r'fb_batch_set_control_law\(batch, NULL\)'):
            call()
    # read-only output, and the block is not a per-environment field
    with pytest.raises(engine.EngineError, match='read-only'):
        B.set('QFRC_LAW', 0.0)
    with pytest.raises(engine.EngineError, match='FB_CONTROL_LAW'):
        B.get('CONTROL_LAW')
    assert engine.FIELDS['QFRC_LAW'][0] == 43 and engine.FIELDS['CONTROL_LAW'][0] == 44
    B.clear_control_law(); B.stage(engine.ST['PRE'], a.ctypes.data)
    # FP32 batches carry the law at their own precision and stay finite
    B32 = engine.Batch(emu_model, 2, precision=32)
    B32.set_control_law(**_random_law(walk_arrays, np.random.default_rng(2), scale=0.3))
    B32.set_reference(qp, qv, terminal_com_dist=float('inf')); B32.reset()
    for k in range(2):
        B32.step_ptr(a[:2].ctypes.data)
    assert np.isfinite(B32.get('QPOS')).all() and B32.get('QFRC_LAW').any()


def test_control_laws_module(emu_model, walk_arrays):
    from flybody_amd import control_laws as cl
    names = [str(n) for n in walk_arrays['names_jnt']]
    coxae = [n for n in names if n.startswith('coxa_abduct')]
    assert len(coxae) == 6
    s = cl.joint_spring(emu_model, coxae, 0.5)
    dofs = cl.hinge_dofs(emu_model, coxae)
    assert (s.pos_gain[dofs] == 0.5).all() and np.count_nonzero(s.pos_gain) == 6
    qa = np.asarray(walk_arrays['jnt_qposadr'])[[names.index(n) for n in coxae]]
    assert np.array_equal(s.pos_ref[dofs], walk_arrays['qpos_spring'][qa])
    d = cl.joint_damper(emu_model, coxae[:2], [1e-3, 2e-3])
    both = s + d + cl.motor_scale(emu_model, 0.1)
    assert both.vel_gain[dofs[1]] == 2e-3 and (both.act_gain == 0.1).all() and np.array_equal(both.pos_ref, s.pos_ref)
    with pytest.raises(ValueError, match='not hinge joints'):
        cl.hinge_dofs(emu_model, [names[0]])
    with pytest.raises(KeyError):
        cl.hinge_dofs(emu_model, ['no_such_joint'])
    with pytest.raises(IndexError):
        cl.ControlLaw.from_dofs(emu_model, [108])


def test_symbols_and_kernel_names(emu_lib):
    import re
    import subprocess
    import __graft_entry__ as g
    lib = g.build_hip()
    syms = subprocess.check_output(['nm', '-D', '--defined-only', lib], text=True)
    for s in ('fb_batch_set_control_law', 'fb_batch_control_law_active', 'fb_batch_end_episode'):
        assert ' ' + s in syms
    names = [re.search(r'Function Name: (\S+)', l).group(1) for l in open(g.HIP_RES) if 'Function Name' in l]
    assert sum('k_step_law' in n for n in names) == 2 and sum('k_step_forces' in n for n in names) == 2 and sum('k_flyI' in n for n in names) == 2
