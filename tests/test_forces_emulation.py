"""External forces (FB_QFRC_APPLIED / FB_XFRC_APPLIED: csrc/fb_forces.hpp, the step kernel k_step_forces) through the kernel-source
emulation build.  The oracle cannot take applied forces, so oracle parity is reached through identities:
  * zero forces: the forces kernel equals the plain one, under both schedulers and through an auto-reset;
  * M (qacc_smooth with - without) = qfrc_applied + sum_b J_b(xipos_b)' [f; tau] with the oracle's mass matrix and Jacobians;
  * gravity: an oracle whose gravity is g + D equals the engine at gravity g with xfrc_applied[b, :3] = body_mass[b] D on every body --
    accelerations, constraint forces, sensors (the force sensors through cfrc_ext) and three control steps of substeps, on
    walk_imitation and with flight_imitation's fluid forces;
  * motors: with force actuators, the oracle's actuator force applied as qfrc_applied with the actuators off gives the same motion;
  * a reset ignores the forces, and the host validates what it is given.
No GPU needed."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, random_state

_rel = lambda a, b: np.abs(np.asarray(a).ravel() - np.asarray(b).ravel()).max() / max(np.abs(np.asarray(b)).max(), 1e-300)

# M (qacc_smooth_with - qacc_smooth_without) against the oracle's Jacobians: measured 5.86e-15 of the largest entry on the emulation
# build; the bound is 100 x that, well inside the 1e-9 the emulation tests hold for geometric quantities.
TOL_JAC = 5.86e-13
# the bounds of tests/test_kernel_emulation.py: test_forward_stage_parity (forward evaluation) and test_env_steps_match_oracle_and_golden
TOL_FWD, TOL_QPOS, TOL_QVEL = 1e-6, 1e-9, 1e-8


@pytest.fixture(scope='module')
def emu_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    return g.build_emu()


@pytest.fixture(scope='module')
def emu_model(walk_arrays, emu_lib):
    from flybody_amd import engine
    return engine.Model(walk_arrays, lib_path=emu_lib)


def _asset(name):
    from flybody_amd import engine
    return dict(engine.load_npz(os.path.join(engine.ASSETS, name + '.npz')))


def test_zero_forces_equal_the_plain_kernel(emu_lib, walk_arrays, reference_traj, monkeypatch):
    """Arrays allocated and all zero: every output of six control steps (an auto-reset among them) equals the plain kernel's, with the
    substep scheduler (the emulation build's two slots put a 5-environment batch on tickets) and with one environment per wave.
    After clear_forces() the batch is back on k_fly and steps like one that never had forces."""
    from flybody_amd import engine
    qp, qv = reference_traj
    acts = np.random.default_rng(9).uniform(-1, 1, (7, 5, 59)).astype(np.float32)
    fields = ('QPOS', 'QVEL', 'OBS', 'REWARD', 'STEP_TYPE')
    for flag in (None, '1'):
        if flag is None: monkeypatch.delenv('FB_NO_TICKETS', raising=False)
        else: monkeypatch.setenv('FB_NO_TICKETS', flag)
        M = engine.Model(walk_arrays, lib_path=emu_lib)
        P, F = engine.Batch(M, 5, precision=64), engine.Batch(M, 5, precision=64)
        assert P.substep_scheduler == (flag is None)
        assert not F.forces_active
        F.set('XFRC_APPLIED', 0.0)
        assert F.forces_active and not P.forces_active
        assert not F.get('QFRC_APPLIED').any() and F.get('XFRC_APPLIED').shape == (5, 6*M.dim('nbody'))
        types = []
        for B in (P, F):
            B.set_reference(qp[:8], qv[:8], future_steps=2, terminal_com_dist=float('inf')); B.reset()       # a short episode: LAST -> FIRST inside
        for k in range(6):
            a = np.ascontiguousarray(acts[k])
            P.step_ptr(a.ctypes.data); F.step_ptr(a.ctypes.data)
            for name in fields:
                assert np.array_equal(P.get(name), F.get(name)), (flag, k, name)
            types.append(P.get('STEP_TYPE').ravel())
        types = np.array(types)
        assert (types == 2).any() and (types == 0).any()
        assert not F.get('XFRC_APPLIED').any() and not F.get('QFRC_APPLIED').any()      # the kernel never writes them
        F.clear_forces()
        assert not F.forces_active
        with pytest.raises(engine.EngineError, match='no applied forces'):
            F.get('QFRC_APPLIED')
        a = np.ascontiguousarray(acts[6])
        P.step_ptr(a.ctypes.data); F.step_ptr(a.ctypes.data)
        for name in fields:
            assert np.array_equal(P.get(name), F.get(name)), (flag, 'cleared', name)
        del P, F, M


def _contact_state(emu_model, reference_traj, seed, nsteps=4):
    """(batch of 1, qpos, qvel) after a short random-action rollout on the ground."""
    from flybody_amd import engine
    qp, qv = reference_traj
    B = engine.Batch(emu_model, 1, precision=64)
    B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    rng = np.random.default_rng(seed)
    for _ in range(nsteps):
        a = rng.uniform(-0.6, 0.6, (1, 59)).astype(np.float32)
        B.step_ptr(a.ctypes.data)
    return B, B.get('QPOS')[0].copy(), B.get('QVEL')[0].copy()


def test_generalised_force_against_the_oracle_jacobian(emu_model, oracle_model, walk_arrays, reference_traj):
    """Random wrenches on seven bodies (thorax, head, a femur, a tarsus, a claw-bearing segment, a wing, the abdomen's end) and a random
    qfrc_applied, at a state with contacts: M (qacc_smooth with - without) = qfrc_applied + sum_b jac(xipos_b, b)' [f; tau]."""
    from flybody_amd.perturbations import body_ids
    from oracle import fbo
    B, q, v = _contact_state(emu_model, reference_traj, seed=21)
    assert int(B.get('NCON')[0, 0]) > 0
    nv, nb = emu_model.dim('nv'), emu_model.dim('nbody')
    names = ['thorax', 'head', 'femur_T2_left', 'tarsus_T1_left', 'tarsus4_T3_right', 'wing_left', 'abdomen_7']
    names = [n for n in names if n in set(map(str, walk_arrays['names_body']))]
    ids = body_ids(emu_model, names)
    assert len(ids) >= 5 and {'thorax', 'tarsus_T1_left', 'wing_left'} <= set(names)
    rng = np.random.default_rng(22)
    B.forward()
    without = B.get('QACC_SMOOTH')[0].copy()
    scale = np.abs(B.get('QFRC_BIAS')[0]).max()
    xf = np.zeros((nb, 6)); xf[ids] = rng.normal(size=(len(ids), 6))*scale
    xf[0] = rng.normal(size=6)*scale                                       # the world body's row is ignored
    qf = rng.normal(size=nv)*scale
    B.set('XFRC_APPLIED', xf.reshape(1, -1)); B.set('QFRC_APPLIED', qf[None])
    B.forward()
    with_ = B.get('QACC_SMOOTH')[0].copy()
    od = fbo.OracleData(oracle_model)
    od.field('qpos')[:] = q; od.field('qvel')[:] = v; od.call('forward')
    expect = qf.copy()
    xipos = od.field('xipos').reshape(nb, 3)
    for b in ids:
        jp, jr = od.jac(xipos[b], int(b))
        expect += jp.T @ xf[b, :3] + jr.T @ xf[b, 3:]
    got = od.mul_m(with_ - without)
    gap = _rel(got, expect)
    print('generalised force vs oracle Jacobian: relative gap %.3g' % gap)
    assert gap < TOL_JAC
    # fb_batch_inverse needs no change: qfrc_inverse - qfrc_actuator of this forward pass is the applied generalised force, up to
    # what noslip (not inverted) and the Newton stop test leave -- the sharp version of this runs on the GPU with noslip off
    assert np.array_equal(B.get('QFRC_APPLIED')[0], qf) and np.array_equal(B.get('XFRC_APPLIED')[0], xf.ravel())


def _gravity_pair(arrays, emu_lib, delta):
    """(engine model at the shipped gravity, oracle model at gravity + delta, per-body wrench rows of body_mass x delta)."""
    from flybody_amd import engine
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    tilted = dict(arrays); tilted['opt_gravity'] = np.asarray(arrays['opt_gravity'], float) + delta
    xf = np.zeros((len(arrays['body_mass']), 6)); xf[:, :3] = np.asarray(arrays['body_mass'])[:, None]*delta[None]
    return engine.Model(arrays, lib_path=emu_lib), fbo.OracleModel(pack_model(tilted)), xf


def _gravity_check(name, arrays, emu_lib, q, v, ctrl, act, delta, nstep=3):
    """Forward evaluation and `nstep` control steps of raw substeps: engine with xfrc_applied = m D against the oracle at g + D."""
    from flybody_amd import engine
    from oracle import fbo
    M, om, xf = _gravity_pair(arrays, emu_lib, delta)
    nsub, na = M.dim('nsubstep'), M.dim('na')
    B = engine.Batch(M, 2, precision=64)
    od = fbo.OracleData(om)
    for fld, val in (('QPOS', q), ('QVEL', v), ('CTRL', ctrl)) + ((('ACT', act),) if na else ()):
        B.set(fld, val)
    od.field('qpos')[:] = q; od.field('qvel')[:] = v; od.field('ctrl')[:] = ctrl
    if na:
        od.field('act')[:na] = act
    B.set('XFRC_APPLIED', xf.reshape(1, -1))
    B.forward(); od.call('forward')
    ncon, nefc = int(od.scalar('ncon')), int(od.scalar('nefc'))
    assert int(B.get('NCON')[0, 0]) == ncon and int(B.get('NEFC')[0, 0]) == nefc and ncon > 0
    sens, osens = B.get('SENSORDATA')[0].copy(), od.field('sensordata').copy()
    # the accelerometer tells gravity from a push: the oracle's reads -(g + D), the engine's -g; add R' D back to the oracle's
    s = int(arrays['sensor_site_thorax'])
    R = od.field('site_xmat').reshape(-1, 3, 3)[s]
    assert _rel(sens[:3], osens[:3]) > 1e-3                                   # (it does tell them apart)
    osens[:3] += R.T @ delta
    nforce = M.dim('nforce')
    figs = dict(qacc=_rel(B.get('QACC')[0], od.field('qacc')), efc=_rel(B.get('EFC_FORCE')[0][:nefc], od.field('efc_force')[:nefc]),
                sens=_rel(sens, osens), accel=_rel(sens[:3], osens[:3]))
    if nforce:
        figs['force_sensors'] = _rel(sens[9:9 + 3*nforce], osens[9:9 + 3*nforce])
        assert np.abs(osens[9:9 + 3*nforce]).max() > 0
    print('%s gravity identity, forward (ncon %d, nefc %d): %s' % (name, ncon, nefc, {k: '%.2e' % x for k, x in figs.items()}))
    for k, x in figs.items():
        assert x < TOL_FWD, (name, k, x)
    assert np.array_equal(B.get('QACC')[0], B.get('QACC')[1])
    # control steps of raw substeps (mj_step2, integration, mj_step1 per substep on both sides)
    for k in range(nstep):
        B.substep(nsub)
        for _ in range(nsub):
            od.call('step2'); od.call('step1')
        assert int(od.scalar('ncon')) < 64 and int(od.scalar('nefc')) < 192      # the oracle alone stays within the caps
    assert not B.get('WARN_EVER').any()
    eq, ev = _rel(B.get('QPOS')[0], od.field('qpos')), _rel(B.get('QVEL')[0], od.field('qvel'))
    print('%s gravity identity, %d control steps of substeps: qpos %.2e qvel %.2e' % (name, nstep, eq, ev))
    assert eq < TOL_QPOS and ev < TOL_QVEL, (name, eq, ev)
    # ... and without the forces the engine does NOT follow the tilted oracle (the check can fail)
    return B, od


def test_gravity_identity_walk(emu_lib, walk_arrays):
    """Oracle at gravity g + D (D horizontal, 10 % of |g|) = engine at g with xfrc_applied[b, :3] = body_mass[b] D on every body."""
    rng = np.random.default_rng(1)
    q, v = random_state(walk_arrays, rng, z=0.125)
    ctrl = rng.uniform(-0.3, 0.3, 59); act = rng.uniform(-0.2, 0.2, 59)
    g = np.linalg.norm(walk_arrays['opt_gravity'])
    delta = 0.1*g*np.array([np.cos(0.7), np.sin(0.7), 0.0])
    B, od = _gravity_check('walk_imitation', walk_arrays, emu_lib, q, v, ctrl, act, delta)
    # the check can fail: the same engine without the forces is not the tilted oracle
    B.clear_forces()
    B.set('QPOS', q); B.set('QVEL', v); B.set('CTRL', ctrl); B.set('ACT', act)
    B.forward(); B.substep(3*B.model.dim('nsubstep'))
    assert _rel(B.get('QVEL')[0], od.field('qvel')) > 1e-4


def test_gravity_identity_flight_with_fluid_forces(emu_lib):
    """The same on flight_imitation: wings beating in the fluid model (ellipsoid forces), retracted legs in contact with the body."""
    a = _asset('flight_imitation')
    rng = np.random.default_rng(4)
    q, v = random_state(a, rng, spread=0.0, z=1.0, vel=1.0)
    lim = [j for j in range(len(a['jnt_type'])) if a['jnt_type'][j] == 3 and a['jnt_limited'][j]]
    lo, hi = a['jnt_range'][lim].T
    qa = a['jnt_qposadr'][lim]
    q[qa] = np.clip(q[qa], lo + 0.01*(hi - lo), hi - 0.01*(hi - lo))
    v = v*10
    nu = len(a['actuator_trntype'])
    ctrl = rng.uniform(-0.3, 0.3, nu)
    g = np.linalg.norm(a['opt_gravity'])
    delta = 0.1*g*np.array([np.cos(2.1), np.sin(2.1), 0.0])
    na = int(sum(1 for x in a['actuator_actadr'] if x >= 0))
    _, od = _gravity_check('flight_imitation', a, emu_lib, q, v, ctrl, rng.uniform(-0.2, 0.2, na) if na else None, delta)
    assert np.abs(od.field('qfrc_fluid')).max() > 1e-3*np.abs(od.field('qfrc_passive')).max()


def test_motor_identity_for_qfrc_applied(emu_lib):
    """force_actuators=True: the actuator force is gain x activation with no position bias.  The variant's actuators all carry
    filter state (dyntype filter), so the force follows the ACTIVATION, not ctrl: the oracle gets activation = ctrl = u (the filter at
    rest, act_dot = 0), the engine gets activation = ctrl = 0 and qfrc_applied = the oracle's qfrc_actuator.  One substep then gives the
    same qacc and qvel.  (The adhesion actuators act through the contacts, not through qfrc_actuator alone: they stay off on both sides.)"""
    from flybody_amd import engine, model_zoo
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    a = model_zoo.get_model(model_zoo.task_config('walk_imitation', force_actuators=True), allow_compile=False)
    assert (np.asarray(a['actuator_biastype']) == 0).all() and not np.asarray(a['actuator_biasprm']).any()
    M, om = engine.Model(a, lib_path=emu_lib), fbo.OracleModel(pack_model(a))
    rng = np.random.default_rng(6)
    q, v = random_state(a, rng, z=0.125)
    nu = len(a['actuator_trntype'])
    u = rng.uniform(-0.8, 0.8, nu); u[np.asarray(a['actuator_trntype']) == 5] = 0
    od = fbo.OracleData(om)
    od.field('qpos')[:] = q; od.field('qvel')[:] = v; od.field('ctrl')[:] = u; od.field('act')[:nu] = u
    od.call('forward')
    fa = od.field('qfrc_actuator').copy()
    assert np.abs(fa).max() > 0 and int(od.scalar('ncon')) > 0
    oqacc = od.field('qacc').copy()
    od.call('step2'); od.call('step1')
    B = engine.Batch(M, 1, precision=64)
    B.set('QPOS', q); B.set('QVEL', v); B.set('CTRL', 0.0); B.set('ACT', 0.0)
    B.set('QFRC_APPLIED', fa[None])
    B.forward()
    assert not B.get('QFRC_ACTUATOR').any()
    ea = _rel(B.get('QACC')[0], oqacc)
    B.substep(1)
    ev = _rel(B.get('QVEL')[0], od.field('qvel'))
    print('motor identity: qacc %.2e, qvel after one substep %.2e' % (ea, ev))
    assert ea < TOL_FWD and ev < TOL_FWD
    assert _rel(B.get('QPOS')[0], od.field('qpos')) < TOL_QPOS


def test_reset_ignores_forces_and_inputs_are_validated(emu_model, emu_lib, reference_traj):
    from flybody_amd import engine
    qp, qv = reference_traj
    nv, nb = emu_model.dim('nv'), emu_model.dim('nbody')
    rng = np.random.default_rng(3)
    P, F = engine.Batch(emu_model, 3, precision=64), engine.Batch(emu_model, 3, precision=64)
    F.set('XFRC_APPLIED', rng.normal(size=(3, 6*nb))*1e-3); F.set('QFRC_APPLIED', rng.normal(size=(3, nv))*1e-3)
    for B in (P, F):
        B.set_reference(qp[:8], qv[:8], future_steps=2, terminal_com_dist=float('inf')); B.reset()
    # a FIRST observation is the same with and without forces: the host-side reset ...
    for name in ('OBS', 'QPOS', 'QVEL', 'SENSORDATA', 'QACC', 'STEP_TYPE'):
        assert np.array_equal(P.get(name), F.get(name)), name
    # ... and the auto-reset of an environment whose last step was LAST (the forces act on the steps in between)
    acts = rng.uniform(-1, 1, (8, 3, 59)).astype(np.float32)
    seen_first = False
    for k in range(8):
        a = np.ascontiguousarray(acts[k]); P.step_ptr(a.ctypes.data); F.step_ptr(a.ctypes.data)
        first = P.get('STEP_TYPE').ravel() == 0
        assert np.array_equal(P.get('STEP_TYPE'), F.get('STEP_TYPE'))
        if first.any():
            seen_first = True
            assert np.array_equal(P.get('OBS')[first], F.get('OBS')[first]) and np.array_equal(P.get('SENSORDATA')[first], F.get('SENSORDATA')[first])
        else:
            assert not np.array_equal(P.get('QVEL'), F.get('QVEL'))
    assert seen_first
    assert F.get('XFRC_APPLIED').any()                                       # nothing cleared them: the caller owns them
    # validation
    with pytest.raises(engine.EngineError, match='size mismatch.*FB_QFRC_APPLIED'):
        engine._check(F.L, F.L.fb_batch_set(F.h, engine.FIELDS['QFRC_APPLIED'][0], np.zeros(4).ctypes.data, 32))
    bad = np.zeros((3, 6*nb)); bad[2, 5] = np.nan
    with pytest.raises(engine.EngineError, match='FB_XFRC_APPLIED of environment 2 is not finite'):
        F.set('XFRC_APPLIED', bad)
    bad = np.zeros((3, nv)); bad[1, 0] = np.inf
    with pytest.raises(engine.EngineError, match='FB_QFRC_APPLIED of environment 1 is not finite'):
        F.set('QFRC_APPLIED', bad)
    G = engine.Batch(emu_model, 2, precision=64)
    with pytest.raises(engine.EngineError, match='not finite'):
        G.set('QFRC_APPLIED', np.full((2, nv), np.nan))
    assert not G.forces_active                                               # a rejected set allocates nothing
    # single-stage profiling runs k_fly: refused while forces are active, with a message
    a = np.ascontiguousarray(acts[0])
    with pytest.raises(engine.EngineError, match='fb_batch_clear_forces'):
        F.stage(engine.ST['PRE'], a.ctypes.data)
    F.clear_forces(); F.stage(engine.ST['PRE'], a.ctypes.data)
    # FP32 batches carry the arrays at their own precision
    B32 = engine.Batch(emu_model, 2, precision=32)
    x = rng.normal(size=(2, 6*nb))
    B32.set('XFRC_APPLIED', x)
    assert np.array_equal(B32.get('XFRC_APPLIED'), x.astype(np.float32).astype(np.float64)) and B32.forces_active
    with pytest.raises(engine.EngineError, match='null batch'):
        engine._check(F.L, F.L.fb_batch_clear_forces(None))


def test_symbols_fields_and_sources(emu_lib):
    """The new entry points are exported by the gfx950 library, the fields have the header's ids, the new kernel source tests no
    preprocessor switch of its own, and the new kernel's name leaves the step kernel's name unique."""
    import re
    import __graft_entry__ as g
    from flybody_amd import engine
    lib = g.build_hip()
    syms = subprocess.check_output(['nm', '-D', '--defined-only', lib], text=True)
    assert ' fb_batch_clear_forces' in syms and ' fb_batch_forces_active' in syms
    assert engine.FIELDS['QFRC_APPLIED'][0] == 40 and engine.FIELDS['XFRC_APPLIED'][0] == 41
    src = open(os.path.join(ROOT, 'flybody_amd', 'csrc', 'fb_forces.hpp')).read()
    for line in src.splitlines():
        m = re.match(r'\s*#\s*(if|ifdef|ifndef|elif)\b(.*)', line)
        assert not (m and re.findall(r'\bFB_\w+', m.group(2))), line
    names = [re.search(r'Function Name: (\S+)', l).group(1) for l in open(g.HIP_RES) if 'Function Name' in l]
    assert sum('k_step_forces' in n for n in names) == 2 and not any('k_fly' in n and 'forces' in n for n in names)
    assert sum('k_flyI' in n for n in names) == 2
