"""fb_batch_inverse (csrc/fb_inverse.hpp: MuJoCo's mj_inverse, one frame per wavefront) through the kernel-source emulation build, against
the CPU oracle: the smooth terms against the oracle's own M qacc + qfrc_bias - qfrc_passive, the constraint forces by inverting the
oracle's forward pass (a converged solve of the forward problem is an inverse of it), the discrete flag against one oracle Euler step,
differentiate_pos against the engine's position integration, and argument validation.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, random_state

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ik_reference as ikr  # noqa: E402

_rel = lambda a, b: np.abs(np.asarray(a).ravel() - np.asarray(b).ravel()).max() / max(np.abs(np.asarray(b)).max(), 1e-300)

# The smooth part of the inverse is M qacc + qfrc_bias - qfrc_passive, the oracle's sums in another order: measured 1.2e-16 (relative to
# the largest entry) on walk_imitation; three orders of magnitude of margin.
TOL_SMOOTH = 1e-13
# Forward (oracle, Newton, noslip off) then inverse: the gap is the Newton stop test's (opt.tolerance 1e-8 on the scaled improvement,
# fb_newton.hpp): f(J qacc - aref) at the solver's qacc differs from the solver's own forces by what the last iteration left.  Measured over
# the 8 states of the test below (nefc 20 - 102): at most 7.9e-7 of max |qfrc_actuator| (median 3.7e-11), 1.04e-8 of max |efc_force|.
TOL_ROUNDTRIP = 1e-5
TOL_EFC = 1e-7
# The same through FB_INV_DISCRETE from one oracle Euler step's (qvel+ - qvel) / h: measured 7.9e-7 as well (the solve dominates; the
# subtraction of velocities costs ~1e-12).
TOL_DISCRETE = 1e-5


@pytest.fixture(scope='module')
def emu_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    return g.build_emu()


def _arrays(name, noslip=True):
    from flybody_amd import engine
    a = dict(engine.load_npz(os.path.join(engine.ASSETS, name + '.npz')))
    if not noslip:
        a['opt_noslip_iterations'] = np.array(0)          # noslip is not inverted (fb_inverse.hpp): forward with it off
    return a


@pytest.fixture(scope='module')
def walk0(emu_lib):
    """walk_imitation with noslip off: engine model (emulation build) and oracle model."""
    from flybody_amd import engine
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    a = _arrays('walk_imitation', noslip=False)
    return engine.Model(a, lib_path=emu_lib), fbo.OracleModel(pack_model(a))


def _oracle_state(om, q, v, ctrl=None):
    from oracle import fbo
    od = fbo.OracleData(om)
    od.field('qpos')[:] = q; od.field('qvel')[:] = v
    if ctrl is not None:
        od.field('ctrl')[:] = ctrl
    return od


@pytest.mark.parametrize('name', ['walk_imitation', 'flight_imitation'])
def test_smooth_part_is_M_qacc_plus_bias_minus_passive(emu_lib, name):
    """Random qacc, fly in the air with its joints inside their ranges: qfrc_inverse + qfrc_constraint = oracle mul_m(qacc) + qfrc_bias -
    qfrc_passive (springs, dampers, and on flight_imitation the ellipsoid fluid forces of the wings).  walk_imitation has no constraint
    row there (qfrc_constraint = 0, no contact force); flight_imitation's retracted legs touch the abdomen."""
    from flybody_amd import engine
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    a = _arrays(name)
    model, om = engine.Model(a, lib_path=emu_lib), fbo.OracleModel(pack_model(a))
    rng = np.random.default_rng(4)
    n = 3
    Q, V, A = [], [], []
    for _ in range(n):
        q, v = random_state(a, rng, spread=0.0, z=2.0)
        lim = [j for j in range(len(a['jnt_type'])) if a['jnt_type'][j] == 3 and a['jnt_limited'][j]]
        lo, hi = a['jnt_range'][lim].T
        qa = a['jnt_qposadr'][lim]
        q[qa] = np.clip(q[qa], lo + 0.01*(hi - lo), hi - 0.01*(hi - lo))        # (flight's qpos0 sits on wing limits)
        Q.append(q); V.append(v*10); A.append(rng.normal(size=len(v))*100)
    B = engine.Batch(model, n, precision=64)
    B.set('QPOS', np.array(Q)); B.set('QVEL', np.array(V)); B.set('QACC', np.array(A))
    B.inverse()
    got = B.get('QFRC_INVERSE') + B.get('QFRC_CONSTRAINT')
    for e in range(n):
        od = _oracle_state(om, Q[e], V[e]); od.call('fwd_position'); od.call('fwd_velocity')
        expect = od.mul_m(A[e]) + od.field('qfrc_bias') - od.field('qfrc_passive')
        assert _rel(got[e], expect) < TOL_SMOOTH, e
        if name == 'flight_imitation':
            assert np.abs(od.field('qfrc_fluid')).max() > 1e-3*np.abs(expect).max()
    if name == 'walk_imitation':
        assert not B.get('NEFC').any() and not B.get('QFRC_CONSTRAINT').any() and not B.get('CONTACT_FORCE').any()
    assert np.array_equal(B.get('QACC'), np.array(A))                # read, not written


def test_forward_then_inverse_recovers_actuator_and_constraint_forces(walk0):
    """Contacts and joint limits (nefc 20 - 114, the one-row-per-lane and the wide J'f paths of the forward pass): the oracle's forward
    qacc goes in, its qfrc_actuator and efc_force come out.  CONTACT_FORCE holds the rows of each contact."""
    from flybody_amd import engine
    model, om = walk0
    a = model.arrays
    states, ods = [], []
    for seed in range(8):
        r = np.random.default_rng(100 + seed)
        q, v = random_state(a, r, z=r.uniform(0.115, 0.14))
        od = _oracle_state(om, q, v, r.uniform(-0.3, 0.3, 59)); od.call('forward')
        states.append((q, v, od.field('qacc').copy())); ods.append(od)
    B = engine.Batch(model, len(states), precision=64)
    for k, name in enumerate(('QPOS', 'QVEL', 'QACC')):
        B.set(name, np.array([s[k] for s in states]))
    B.inverse()
    qi, ef, nefc = B.get('QFRC_INVERSE'), B.get('EFC_FORCE'), B.get('NEFC')[:, 0]
    cf, ncon = B.get('CONTACT_FORCE').reshape(-1, 64, 3), B.get('NCON')[:, 0]
    assert max(nefc) > 64 and min(nefc) < 32
    for e, od in enumerate(ods):
        n = int(od.scalar('nefc'))
        assert nefc[e] == n and ncon[e] == int(od.scalar('ncon'))
        assert _rel(qi[e], od.field('qfrc_actuator')) < TOL_ROUNDTRIP, e
        assert _rel(ef[e][:n], od.field('efc_force')[:n]) < TOL_EFC, e
        oc = od.contacts()
        for c in range(64):
            if c < len(oc) and oc[c, 10] >= 0:
                adr, dim = int(oc[c, 10]), int(oc[c, 9])
                assert np.array_equal(cf[e, c, :dim], ef[e, adr:adr + dim]) and not cf[e, c, dim:].any()
            else:
                assert not cf[e, c].any()
    # the contact-frame normal force of a frictional contact is >= 0, and the cone holds
    live = cf[..., 0] != 0
    assert live.any() and (cf[..., 0] >= 0).all()


def test_discrete_flag_inverts_one_euler_step(walk0):
    """FB_INV_DISCRETE: qacc = (qvel+ - qvel) / h of one oracle substep (semi-implicit Euler, implicit joint damping) gives back that
    substep's qfrc_actuator; read as a continuous acceleration it does not (the damping term h D is missing)."""
    from flybody_amd.inverse_dynamics import inverse_dynamics
    model, om = walk0
    a = model.arrays
    h = float(a['opt_timestep'])
    for seed in (0, 1, 4):
        r = np.random.default_rng(100 + seed)
        q, v = random_state(a, r, z=r.uniform(0.115, 0.14))
        od = _oracle_state(om, q, v, r.uniform(-0.3, 0.3, 59)); od.call('step1'); od.call('step2')
        fa = od.field('qfrc_actuator').copy(); acc = (od.field('qvel') - v)/h
        res = inverse_dynamics(model, q, v, acc, discrete=True)
        assert _rel(res.qfrc_inverse, fa) < TOL_DISCRETE, seed
        assert _rel(inverse_dynamics(model, q, v, acc).qfrc_inverse, fa) > 1e3*TOL_DISCRETE, seed


def test_differentiate_pos_inverts_integrate_pos(walk0):
    """integratePos(q, differentiate_pos(q, q') h) == q' for the free joint (tilted, more than half a turn apart) and the hinges."""
    from flybody_amd.inverse_dynamics import differentiate_pos
    model, _ = walk0
    a = model.arrays
    rng = np.random.default_rng(3)
    h = float(a['opt_timestep'])
    for _ in range(4):
        qa, _ = random_state(a, rng); qb, _ = random_state(a, rng)
        qb[3:7] = rng.normal(size=4); qb[3:7] /= np.linalg.norm(qb[3:7])
        v = differentiate_pos(model, qa, qb, h)
        q = qa.copy(); ikr.integrate_pos(a, q, v*h)
        qn = q[3:7] * np.sign(q[3]*qb[3] + np.dot(q[4:7], qb[4:7]))       # (q and -q are one rotation)
        assert np.abs(np.r_[q[:3], qn, q[7:]] - qb).max() < 1e-14
        assert np.abs(np.linalg.norm(v[3:6])*h) <= np.pi + 1e-12      # the shorter way round
    # batched form = per-frame form; hinge entries are plain differences
    qa, _ = random_state(a, rng); qb, _ = random_state(a, rng)
    V = differentiate_pos(model, np.array([qa, qb]), np.array([qb, qa]), h)
    assert np.allclose(V[0], differentiate_pos(model, qa, qb, h), rtol=0, atol=1e-9) and np.allclose(V[0, 6:], -V[1, 6:], rtol=1e-12)


def test_trajectory_inverse_dynamics_on_oracle_substeps(walk0):
    """qpos recorded substep by substep (oracle, fixed ctrl): frames 1 .. T-2 give back each substep's qfrc_actuator."""
    from flybody_amd.inverse_dynamics import trajectory_inverse_dynamics
    model, om = walk0
    a = model.arrays
    h = float(a['opt_timestep'])
    q, v = random_state(a, np.random.default_rng(7), z=0.125)
    od = _oracle_state(om, q, v, np.random.default_rng(8).uniform(-0.3, 0.3, 59)); od.call('step1')
    Q, FA = [od.field('qpos').copy()], []
    for _ in range(8):
        od.call('step2'); FA.append(od.field('qfrc_actuator').copy()); od.call('step1'); Q.append(od.field('qpos').copy())
    tr = trajectory_inverse_dynamics(model, np.array(Q), h)
    assert tr.frames.tolist() == list(range(1, 8)) and tr.result.qfrc_inverse.shape == (7, len(a['dof_bodyid']))
    # measured: at most 2.1e-5 of max |qfrc_actuator| per frame (finite differences of positions through stiff contacts, and the solver's
    # stop test); the bound leaves a factor 10
    for k, f in enumerate(tr.frames):
        assert _rel(tr.result.qfrc_inverse[k], FA[f]) < 2e-4, f
    names = [str(n) for n in a['names_jnt']]
    j = next(i for i, t in enumerate(a['jnt_type']) if t == 3)
    assert np.array_equal(tr.joint_torques[names[j]], tr.result.qfrc_inverse[:, int(a['jnt_dofadr'][j])])
    assert tr.joint_torques[names[0]].shape == (7, 6) and np.array_equal(tr.result.root_residual, tr.result.qfrc_inverse[:, :6])


def test_single_frame_and_chunking(walk0):
    from flybody_amd.inverse_dynamics import inverse_dynamics
    model, _ = walk0
    a = model.arrays
    rng = np.random.default_rng(9)
    S = [random_state(a, rng, z=0.125) for _ in range(5)]
    Q = np.array([s[0] for s in S]); V = np.array([s[1] for s in S]); A = rng.normal(size=V.shape)*50
    full = inverse_dynamics(model, Q, V, A)
    chunked = inverse_dynamics(model, Q, V, A, batch_size=2)
    for f in full._fields:
        assert np.array_equal(getattr(full, f), getattr(chunked, f)), f
    one = inverse_dynamics(model, Q[3], V[3], A[3])
    assert np.array_equal(one.qfrc_inverse, full.qfrc_inverse[3]) and one.ncon == full.ncon[3] and one.root_residual.shape == (6,)
    live = np.arange(64) < full.ncon[:, None]
    assert (full.contact_geoms[live] >= 0).all() and (full.contact_geoms[~live] == -1).all()
    assert np.allclose(np.linalg.norm(full.contact_normal[live], axis=-1), 1)


def test_argument_validation(walk0, emu_lib):
    from flybody_amd import engine
    model, _ = walk0
    B = engine.Batch(model, 2, precision=64)
    with pytest.raises(engine.EngineError, match='run fb_batch_inverse first'):
        B.get('QFRC_INVERSE')
    with pytest.raises(engine.EngineError, match='unknown flags'):
        _check = engine._check
        _check(B.L, B.L.fb_batch_inverse(B.h, 2, None))
    acc = np.zeros((2, model.dim('nv'))); acc[1, 7] = np.nan
    B.set('QACC', acc)
    with pytest.raises(engine.EngineError, match='environment 1 is not finite'):
        B.inverse()
    acc[1, 7] = np.inf; B.set('QACC', acc)
    with pytest.raises(engine.EngineError, match='not finite'):
        B.inverse(discrete=True)
    with pytest.raises(engine.EngineError, match='field is read-only'):
        B.set('CONTACT_FORCE', np.zeros((2, 192)))
    B32 = engine.Batch(model, 2, precision=32)
    with pytest.raises(engine.EngineError, match='FP64 batch'):
        B32.inverse()
    with pytest.raises(engine.EngineError, match='null batch'):
        engine._check(B.L, B.L.fb_batch_inverse(None, 0, None))
    acc[1, 7] = 0; B.set('QACC', acc)
    B.inverse()
    assert np.isfinite(B.get('QFRC_INVERSE')).all()
    from flybody_amd.inverse_dynamics import inverse_dynamics, trajectory_inverse_dynamics
    a = model.arrays
    with pytest.raises(ValueError):
        inverse_dynamics(model, a['qpos0'], np.zeros(3), np.zeros(3))
    with pytest.raises(ValueError):
        trajectory_inverse_dynamics(model, np.tile(a['qpos0'], (2, 1)), 1e-4)
