"""fb_batch_ik (csrc/fb_ik.hpp: multi-site inverse kinematics, the reference's qpos_from_site_xpos) through the kernel-source emulation
build, against the FP64 restatement of the reference algorithm on the CPU oracle (tests/ik_reference.py) and against finite differences
of the objective on oracle site positions.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ik_reference as ikr  # noqa: E402

# Measured emulation-vs-restatement gap (FP64 sum-order differences only): <= 8e-16 in qpos and ~2e-15 relative in the objective after
# 200 - 300 iterations on the 12 leg sites / 66 leg hinges + root.  The tolerances below leave three orders of magnitude to it.
TOL_QPOS = 1e-12
TOL_ERR = 1e-11


@pytest.fixture(scope='module')
def emu_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    return g.build_emu()


@pytest.fixture(scope='module')
def walk(emu_lib):
    from flybody_amd import engine
    return engine.Model.from_asset('walk_imitation', lib_path=emu_lib)


def _leg_problem(model, n, seed, scale=0.5):
    """12 leg sites (tarsi, claws), the 66 leg hinges; targets = site positions of seeded poses within the leg joint ranges."""
    from flybody_amd import engine
    a = model.arrays
    names = [str(s) for s in a['names_site']]
    sites = [names.index(s) for s in names if s.startswith(('tarsus_', 'claw_'))]
    legs = [int(j) for j in a['leg_joints']]
    lo, hi = a['jnt_range'][legs].T
    tq = np.tile(a['qpos0'], (n, 1))
    tq[:, a['jnt_qposadr'][legs]] = np.random.default_rng(seed).uniform(scale*lo, scale*hi, (n, len(legs)))
    B = engine.Batch(model, n, precision=64)
    B.set('QPOS', tq); B.forward()
    return sites, legs, B.get('SITE_XPOS').reshape(n, -1, 3)[:, sites].copy()


def _oracle(model):
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    return fbo.OracleData(fbo.OracleModel(pack_model(model.arrays)))


def _run_both(model, q0, sites, joints, T, **kw):
    """fb_batch_ik on every frame vs the restatement frame by frame."""
    from flybody_amd import engine
    n = len(T)
    B = engine.Batch(model, n, precision=64)
    B.set('QPOS', q0)
    B.ik(sites, joints, T, **kw)
    got = (B.get('QPOS'), B.get('IK_ERR'), B.get('IK_STEPS'))
    od = _oracle(model)
    include = kw.pop('include', None)
    ref = []
    for e in range(n):
        od.field('qpos')[:] = np.broadcast_to(q0, (n, len(model.arrays['qpos0'])))[e]
        ref.append(ikr.qpos_from_site_xpos(od, model.arrays, sites, T[e], joints, include=include, **kw))
    return got, ref


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def test_site_xpos_field_matches_oracle(walk):
    from flybody_amd import engine
    from conftest import random_state
    rng = np.random.default_rng(5)
    B = engine.Batch(walk, 3, precision=64)
    q, _ = random_state(walk.arrays, rng)
    B.set('QPOS', q); B.forward()
    od = _oracle(walk)
    od.field('qpos')[:] = q; od.call('kinematics')
    assert np.abs(B.get('SITE_XPOS')[1] - od.field('site_xpos')).max() < 1e-12


@pytest.mark.parametrize('reg', [0.0, 0.05])
def test_first_step_is_minus_lr_times_finite_difference_gradient(walk, reg):
    """One step with beta = 0 moves qpos by -lr x grad; grad by central differences of the objective on oracle site positions (leg
    hinges + the root's six dofs, through the same mj_integratePos the kernel restates)."""
    a = walk.arrays
    sites, legs, T = _leg_problem(walk, 1, 11)
    joints = [0] + legs
    q0 = a['qpos0'].copy()
    q0[3:7] = [0.98, 0.05, -0.1, 0.12]; q0[3:7] /= np.linalg.norm(q0[3:7])           # a tilted root: rotations are not about the world axes
    lr = 1e-3
    from flybody_amd import engine
    B = engine.Batch(walk, 1, precision=64)
    B.set('QPOS', q0)
    B.ik(sites, joints, T, reg_strength=reg, lr=lr, beta=0.0, progress_threshold=0.0, max_steps=1)
    q1 = B.get('QPOS')[0]
    od = _oracle(walk)
    hq = [int(a['jnt_qposadr'][j]) for j in legs]
    nv = len(a['dof_bodyid'])

    def f(q):
        od.field('qpos')[:] = q; od.call('kinematics')
        s = od.field('site_xpos').reshape(-1, 3)[sites]
        return np.sum((s - T[0])**2) + reg*np.sum(q[hq]**2)

    dofs = ikr.joint_dofs(a, joints)
    h = 1e-6
    g = np.zeros(nv)
    for i in dofs:
        e = np.zeros(nv); e[i] = h
        qp = q0.copy(); ikr.integrate_pos(a, qp, e)
        qm = q0.copy(); ikr.integrate_pos(a, qm, -e)
        g[i] = (f(qp) - f(qm)) / (2*h)
    expect = q0.copy(); ikr.integrate_pos(a, expect, -lr*g)
    dq_k, dq_fd = q1 - q0, expect - q0
    assert np.abs(dq_fd).max() > 1e-6                                                  # the step moves something
    assert np.abs(dq_k - dq_fd).max() <= 1e-6*np.abs(dq_fd).max()


def test_fixed_step_run_matches_restatement(walk):
    sites, legs, T = _leg_problem(walk, 8, 3)
    (Q, E, S), ref = _run_both(walk, walk.arrays['qpos0'], sites, [0] + legs, T, reg_strength=1e-4, progress_threshold=0.0, max_steps=250)
    for e, (q, err, first, steps, ok) in enumerate(ref):
        assert np.abs(Q[e] - q).max() < TOL_QPOS
        assert _rel(E[e, 0], err) < TOL_ERR and _rel(E[e, 1], first) < TOL_ERR
        assert (S[e, 0], S[e, 1]) == (steps, int(ok)) == (249, 0)


@pytest.mark.parametrize('thr,max_steps', [(0.1, 301), (0.05, 201)])
def test_converging_run_steps_and_success_match(walk, thr, max_steps):
    sites, legs, T = _leg_problem(walk, 8, 3)
    (Q, E, S), ref = _run_both(walk, walk.arrays['qpos0'], sites, [0] + legs, T, progress_threshold=thr, max_steps=max_steps)
    got = [(int(s), int(k)) for s, k in S]
    want = [(r[3], int(r[4])) for r in ref]
    assert got == want
    assert 0 < sum(k for _, k in want) < len(want)                                     # some frames converge, some run out
    for e, r in enumerate(ref):
        assert np.abs(Q[e] - r[0]).max() < TOL_QPOS and _rel(E[e, 0], r[1]) < TOL_ERR and _rel(E[e, 1], r[2]) < TOL_ERR


def test_include_mask_xy_only(walk):
    sites, legs, T = _leg_problem(walk, 3, 9)
    inc = np.tile([1, 1, 0], len(sites))
    (Q, E, S), ref = _run_both(walk, walk.arrays['qpos0'], sites, legs, T, include=inc, progress_threshold=0.0, max_steps=120)
    for e, r in enumerate(ref):
        assert np.abs(Q[e] - r[0]).max() < TOL_QPOS and _rel(E[e, 0], r[1]) < TOL_ERR and _rel(E[e, 1], r[2]) < TOL_ERR
    # the excluded components do not enter at all: moving every z target changes no bit
    from flybody_amd import engine
    Tz = T.copy(); Tz[:, :, 2] += 0.05
    B = engine.Batch(walk, 3, precision=64)
    B.ik(sites, legs, Tz, include=inc, progress_threshold=0.0, max_steps=120)
    assert np.array_equal(B.get('QPOS'), Q) and np.array_equal(B.get('IK_ERR'), E)


def test_flight_model_frame(emu_lib):
    from flybody_amd import engine
    M = engine.Model.from_asset('flight_imitation', lib_path=emu_lib)
    a = M.arrays
    jn = [str(j) for j in a['names_jnt']]; sn = [str(s) for s in a['names_site']]
    joints = [jn.index(j) for j in ('root', 'head_abduct', 'head_twist', 'head', 'abdomen_abduct', 'abdomen')]
    sites = [sn.index(s) for s in ('thorax', 'head', 'claw_T1_left', 'claw_T3_right')]
    tq = a['qpos0'].copy()
    tq[0:3] += [0.01, -0.02, 0.005]
    for j, v in zip(joints[1:], (0.1, -0.1, 0.2, 0.05, -0.1)):
        tq[a['jnt_qposadr'][j]] = v
    B = engine.Batch(M, 1, precision=64); B.set('QPOS', tq); B.forward()
    T = B.get('SITE_XPOS').reshape(1, -1, 3)[:, sites]
    (Q, E, S), ref = _run_both(M, a['qpos0'], sites, joints, T, reg_strength=1e-3, progress_threshold=0.0, max_steps=150)
    assert np.abs(Q[0] - ref[0][0]).max() < TOL_QPOS and _rel(E[0, 0], ref[0][1]) < TOL_ERR and _rel(E[0, 1], ref[0][2]) < TOL_ERR


def test_python_api_scalar_and_chunked(walk):
    """flybody_amd.inverse_kinematics on the emulation build: one frame gives scalars, batch_size chunking is bit-identical."""
    from flybody_amd.inverse_kinematics import qpos_from_site_xpos
    a = walk.arrays
    sites, legs, T = _leg_problem(walk, 5, 21)
    sn = [str(s) for s in a['names_site']]; jn = [str(j) for j in a['names_jnt']]
    snames = [sn[s] for s in sites]; jnames = [jn[j] for j in legs]
    kw = dict(progress_threshold=0.0, max_steps=60)
    one = qpos_from_site_xpos(walk, snames, T[2], jnames, **kw)
    assert isinstance(one.err_norm, float) and isinstance(one.steps, int) and isinstance(one.success, bool) and one.qpos.shape == (len(a['qpos0']),)
    full = qpos_from_site_xpos(walk, snames, T, jnames, **kw)
    chunk = qpos_from_site_xpos(walk, snames, T, jnames, batch_size=2, **kw)
    for f in full._fields:
        assert np.array_equal(getattr(full, f), getattr(chunk, f)), f
    assert np.array_equal(one.qpos, full.qpos[2]) and one.err_norm == full.err_norm[2]
    with pytest.raises(ValueError):
        qpos_from_site_xpos(walk, snames[:-1] + ['no_such_site'], T[0], jnames)
    with pytest.raises(ValueError):
        qpos_from_site_xpos(walk, snames, T[0], jnames + [jnames[0]])
    with pytest.raises(ValueError):
        qpos_from_site_xpos(walk, snames[:1] + snames[:1], T[0, :2], jnames)


def test_validation(walk, emu_lib):
    from flybody_amd import engine
    a = walk.arrays
    sites, legs, T = _leg_problem(walk, 2, 1)
    B = engine.Batch(walk, 2, precision=64)
    ok = dict(progress_threshold=0.0, max_steps=2)
    B.ik(sites, legs, T, **ok)                                                          # the baseline call is valid

    def bad(msg, s=sites, j=legs, t=T, **kw):
        args = dict(ok); args.update(kw)
        with pytest.raises(engine.EngineError, match=msg):
            B.ik(s, j, t, **args)

    bad('site id out of range', s=[walk.dim('nsite')] + sites[1:])
    bad('site id out of range', s=[-1] + sites[1:])
    bad('duplicate site', s=[sites[0]] + sites[:-1])
    bad('joint id out of range', j=legs[:-1] + [walk.dim('njnt')])
    bad('duplicate joint', j=legs[:-1] + [legs[0]])
    bad('at least one site', s=[], t=T[:, :0])
    for name in ('reg_strength', 'lr', 'beta', 'progress_threshold'):
        bad('finite', **{name: float('nan')})
        bad('finite', **{name: float('inf')})
    bad('max_steps', max_steps=0)
    tn = T.copy(); tn[1, 3, 2] = np.nan
    bad('NaN', t=tn)
    bad('0 or 1', include=np.full(3*len(sites), 2))
    L = walk.L
    assert L.fb_batch_ik(B.h, None, T.ctypes.data, None) != 0
    B32 = engine.Batch(walk, 2, precision=32)
    with pytest.raises(engine.EngineError, match='FP64'):
        B32.ik(sites, legs, T, **ok)
    # nothing of the rejected calls reached the state
    assert np.array_equal(B.get('IK_STEPS')[:, 0], [1, 1])
    with pytest.raises(engine.EngineError, match='not allocated'):
        engine.Batch(walk, 2, precision=64).get('IK_ERR')
