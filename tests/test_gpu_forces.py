"""External forces (FB_QFRC_APPLIED / FB_XFRC_APPLIED, the step kernel k_step_forces: csrc/fb_forces.hpp) on the MI355X: the gravity
identity against the CPU oracle over a long rollout on both engine builds, the substep scheduler against one environment per wave,
zero forces against k_fly, forward-then-inverse, an FP32 batch, and the reference's control-callback test restated."""
import os

import numpy as np
import pytest

from conftest import ROOT

_rel = lambda a, b: np.abs(np.asarray(a).ravel() - np.asarray(b).ravel()).max() / max(np.abs(np.asarray(b)).max(), 1e-300)

# Gravity identity, 64 environments x 100 control steps: the bound tests/test_gpu_parity.py holds for FP64 rollouts against the oracle.
TOL_ROLLOUT = 1e-6
GRAVITY_STEPS = 100
# forward then inverse: the Newton stop gap the inverse tests document for the emulation build (tests/test_inverse_emulation.py)
TOL_INVERSE = 7.9e-7


def gravity_rollout(lib_path, n, steps, on_gpu=True, trace=None):
    """n walk_imitation environments, `steps` control steps of U(-0.5, 0.5) actions (the reference env test's), gravity tilted by a
    horizontal D of 10 % of |g|: the ORACLE runs a model whose opt_gravity is g + D, the engine the shipped model with
    xfrc_applied[b, :3] = body_mass[b] D on every body.  Returns (max relative qpos gap, qvel gap over the environments, engine
    WARN_EVER any, oracle sizes within caps, median drift along D).  trace: a list that receives (step, qpos gap, qvel gap) every 10
    steps.  lib_path: an engine library (None: the default build); on_gpu False: the emulation build."""
    from flybody_amd import engine
    from flybody_amd.model_blob import load_npz, pack_model
    from flybody_amd.reference import default_walking_reference
    from oracle import fbo
    a = dict(load_npz(os.path.join(ROOT, 'flybody_amd', 'assets', 'walk_imitation.npz')))
    g = np.linalg.norm(a['opt_gravity'])
    delta = 0.1*g*np.array([np.cos(0.7), np.sin(0.7), 0.0])
    tilted = dict(a); tilted['opt_gravity'] = np.asarray(a['opt_gravity'], float) + delta
    om = fbo.OracleModel(pack_model(tilted))
    qp, qv = default_walking_reference()
    M = engine.Model(a, lib_path=lib_path)
    B = engine.Batch(M, n, precision=64)
    B.set_reference(qp, qv, terminal_com_dist=float('inf'))
    xf = np.zeros((len(a['body_mass']), 6)); xf[:, :3] = np.asarray(a['body_mass'])[:, None]*delta[None]
    B.set('XFRC_APPLIED', xf.reshape(1, -1))
    B.reset()
    ods = []
    for _ in range(n):
        od = fbo.OracleData(om); od.configure_env(qp, qv, terminal_com_dist=float('inf')); od.env_reset(); ods.append(od)
    # the reset ignored the forces and gravity does not enter a FIRST observation's positions: same start on both sides
    assert _rel(B.get('QPOS')[0], ods[0].field('qpos')) < 1e-12
    rngs = [np.random.default_rng(2000 + e) for e in range(n)]
    caps_ok = True
    if on_gpu:
        import torch
    for k in range(steps):
        act = np.stack([r.uniform(-0.5, 0.5, 59) for r in rngs]).astype(np.float32)
        if on_gpu:
            t = torch.from_numpy(act).cuda(); B.step_ptr(t.data_ptr(), torch.cuda.current_stream().cuda_stream); torch.cuda.synchronize()
        else:
            B.step_ptr(np.ascontiguousarray(act).ctypes.data)
        fbo.step_batch(ods, act.astype(np.float64))
        caps_ok = caps_ok and all(int(od.scalar('ncon')) < 64 and int(od.scalar('nefc')) < 192 for od in ods)
        if trace is not None and (k + 1) % 10 == 0:
            Q, V = B.get('QPOS'), B.get('QVEL')
            trace.append((k + 1, max(_rel(Q[e], ods[e].field('qpos')) for e in range(n)), max(_rel(V[e], ods[e].field('qvel')) for e in range(n))))
    Q, V = B.get('QPOS'), B.get('QVEL')
    eq = max(_rel(Q[e], ods[e].field('qpos')) for e in range(n))
    ev = max(_rel(V[e], ods[e].field('qvel')) for e in range(n))
    assert B.get('STEP_TYPE').ravel().tolist() == [int(od.scalar('step_type')) for od in ods]
    # displacement along D, reported only (the claws' adhesion holds a standing fly against a 10 % tilt)
    drift = (Q[:, :2] - qp[0, :2]) @ (delta[:2]/np.linalg.norm(delta))
    return eq, ev, bool(B.get('WARN_EVER').any()), caps_ok, float(np.median(drift))


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('dense', [False, True])
def test_gravity_identity_rollout_matches_oracle(dense):
    """64 environments, 100 control steps, both engine builds, against the oracle (never against the engine itself).  The emulation
    build measures 3.7e-10 / 4.3e-10 on qpos / qvel for this rollout at step 100 (at most 6.8e-10 / 6.4e-9 at any tenth step), below the
    1e-7 the horizon is chosen by.  The gap is not rounding: the two sides reach the same physics by different sums, and
    where that flips a Newton iteration count the results differ by what the stop test (opt.tolerance 1e-8) leaves."""
    from flybody_amd import engine
    trace = []
    eq, ev, warned, caps_ok, drift = gravity_rollout(engine.HIP_LIB_DENSE if dense else None, 64, GRAVITY_STEPS, trace=trace)
    print('gravity identity, (step, qpos gap, qvel gap):', ' '.join('(%d %.1e %.1e)' % t for t in trace))
    print('gravity identity %s build, %d control steps: qpos %.2e qvel %.2e, median drift along D %.3f' % ('12-per-CU' if dense else 'default', GRAVITY_STEPS, eq, ev, drift))
    assert caps_ok and not warned
    assert eq < TOL_ROLLOUT and ev < TOL_ROLLOUT, (eq, ev)


def _walk_batch(n, dense=False, precision=64, arrays=None):
    from flybody_amd import engine
    from flybody_amd.reference import default_walking_reference
    M = engine.Model(arrays, dense=dense) if arrays is not None else engine.Model.from_asset('walk_imitation', dense=dense)
    B = engine.Batch(M, n, precision=precision)
    qp, qv = default_walking_reference()
    B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    return M, B


def _rollout(B, steps, seed, first=0):
    import torch
    act = torch.empty(B.n_env, B.model.dim('nact'), device='cuda')
    for k in range(first, first + steps):
        B.random_actions(act.data_ptr(), k, seed=seed, dist=1)
        B.step_ptr(act.data_ptr())
    torch.cuda.synchronize()


def _random_wrenches(M, n, rng, scale=2.0):
    """[n][nbody][6]: forces of about `scale` body weights and torques of that force x 0.01 (model length units) on every body."""
    a = M.arrays
    w = np.asarray(a['body_mass'])[None, :, None]*np.linalg.norm(a['opt_gravity'])*scale
    x = rng.normal(size=(n, len(a['body_mass']), 6))*w
    x[:, :, 3:] *= 0.01
    return x


@pytest.mark.parametrize('dense', [False, True])
def test_substep_scheduler_bit_equal_to_per_wave_with_forces(dense, monkeypatch):
    """4096 environments with random wrenches and generalised forces: the ticket scheduler (substeps of an environment on different
    waves, the force arrays read by whichever wave holds the ticket) gives the results of FB_NO_TICKETS=1 to the bit."""
    rng = np.random.default_rng(5)
    out = []
    for tickets in (True, False):
        if tickets: monkeypatch.delenv('FB_NO_TICKETS', raising=False)
        else: monkeypatch.setenv('FB_NO_TICKETS', '1')
        M, B = _walk_batch(4096, dense=dense)
        assert B.substep_scheduler == tickets
        if not out:
            x = _random_wrenches(M, 4096, rng); qf = rng.normal(size=(4096, M.dim('nv')))*1e-3
        B.set('XFRC_APPLIED', x.reshape(4096, -1)); B.set('QFRC_APPLIED', qf)
        _rollout(B, 12, seed=7)
        out.append([B.get(f).copy() for f in ('QPOS', 'QVEL', 'OBS', 'REWARD', 'STEP_TYPE', 'SENSORDATA')])
        del B, M
    assert np.isfinite(out[0][0]).all()
    for u, v in zip(*out):
        assert np.array_equal(u, v)


@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('n', [256, 4096])
def test_zero_forces_equal_k_fly(n, dense):
    """Arrays allocated, all zero: k_step_forces gives k_fly's results (== ; per-wave launch at 256, tickets at 4096)."""
    M, P = _walk_batch(n, dense=dense)
    _, F = _walk_batch(n, dense=dense)
    F.set('QFRC_APPLIED', 0.0)
    assert F.forces_active and not P.forces_active
    for B in (P, F):
        _rollout(B, 12, seed=11)
    for f in ('QPOS', 'QVEL', 'OBS', 'REWARD', 'STEP_TYPE', 'SENSORDATA', 'QACC'):
        assert np.array_equal(P.get(f), F.get(f)), f
    F.clear_forces()
    for B in (P, F):
        _rollout(B, 3, seed=11, first=12)
    for f in ('QPOS', 'QVEL', 'OBS'):
        assert np.array_equal(P.get(f), F.get(f)), f


def _inverse_round_trip(tolerance):
    """Forward-with-forces then inverse on 64 flies on the ground after a 20-step rollout; opt_tolerance = `tolerance` (None: the
    shipped 1e-8), noslip off.  Per environment: max |qfrc_inverse - qfrc_actuator - applied| relative to max |qfrc_actuator| (what the
    inverse tests' 7.9e-7 is a fraction of) and relative to max |qfrc_actuator + applied| (the force the inverse recovers here); the
    applied generalised force is formed from the ORACLE's Jacobians at the same state.  Also the nefc range and the OR of FB_WARN."""
    from flybody_amd import engine
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    a = dict(engine.load_npz(f'{engine.ASSETS}/walk_imitation.npz')); a['opt_noslip_iterations'] = np.array(0)
    if tolerance is not None:
        a['opt_tolerance'] = np.array(float(tolerance))
    n = 64
    M, B = _walk_batch(n, arrays=a)
    _rollout(B, 20, seed=13)
    rng = np.random.default_rng(14)
    nv, nb = M.dim('nv'), M.dim('nbody')
    x = _random_wrenches(M, n, rng); qf = rng.normal(size=(n, nv))*1e-3
    B.set('XFRC_APPLIED', x.reshape(n, -1)); B.set('QFRC_APPLIED', qf)
    B.forward()
    fa, Q, V = B.get('QFRC_ACTUATOR'), B.get('QPOS'), B.get('QVEL')
    warn = int(np.bitwise_or.reduce(B.get('WARN').ravel()))
    B.inverse()
    got = B.get('QFRC_INVERSE') - fa
    om = fbo.OracleModel(pack_model(a))
    by_act, by_total = [], []
    for e in range(n):
        od = fbo.OracleData(om); od.field('qpos')[:] = Q[e]; od.field('qvel')[:] = V[e]; od.call('fwd_position')
        xi = od.field('xipos').reshape(nb, 3)
        expect = qf[e].copy()
        for b in range(1, nb):
            jp, jr = od.jac(xi[b], b)
            expect += jp.T @ x[e, b, :3] + jr.T @ x[e, b, 3:]
        err = np.abs(got[e] - expect).max()
        by_act.append(err/np.abs(fa[e]).max()); by_total.append(err/np.abs(fa[e] + expect).max())
    assert B.get('NCON').max() > 0 and np.abs(fa).max(axis=1).min() > 0
    return np.array(by_act), np.array(by_total), (int(B.get('NEFC').min()), int(B.get('NEFC').max())), warn


def _report(tag, by_act, by_total, nefc, warn):
    print('inverse round trip with forces, %s: gap / max|qfrc_actuator| max %.2e median %.2e; gap / max|qfrc_actuator + applied| max %.2e '
          'median %.2e (nefc %d-%d, WARN %d)' % (tag, by_act.max(), np.median(by_act), by_total.max(), np.median(by_total), nefc[0], nefc[1], warn))


def test_inverse_round_trip_returns_the_applied_force():
    """The issue's case: noslip off (it is not inverted), the shipped solver tolerance.  64 flies on the ground after a 20-step rollout,
    random wrenches and generalised forces of body-weight scale; a forward evaluation with the forces, then fb_batch_inverse on its
    qacc: qfrc_inverse - qfrc_actuator is the applied generalised force qfrc_applied + sum_b J_b' xfrc_b.  Bound: the 7.9e-7 of
    max |qfrc_actuator| the inverse tests document for the emulation build, normalised as they normalise it.

    Measured on the MI355X over these 64 states (nefc 7 - 20): at most 7.34e-7 of max |qfrc_actuator| (median 1.3e-10); relative to
    max |qfrc_actuator + applied|, the force the inverse recovers here, 9.97e-7 (median 9.6e-11).  The margin to the bound is small and
    is not the force path's: what an inverse of a forward pass leaves is the forward solver's stop gap (fb_newton.hpp, opt_tolerance
    1e-8 on the scaled improvement) -- the plain round trip without forces measures 7.7e-6 on the GPU's 64 oracle states and 1.7e-6 over
    4096 environments (tests/test_gpu_inverse.py) -- and the same states with the solver converged give 5.1e-9 (the next test)."""
    by_act, by_total, nefc, warn = _inverse_round_trip(None)
    _report('opt_tolerance 1e-8 (shipped)', by_act, by_total, nefc, warn)
    assert by_act.max() < TOL_INVERSE


def test_inverse_round_trip_with_converged_solver():
    """The same states and forces with the forward solver converged (opt_tolerance 1e-12, a model option like noslip): the stop gap is
    gone and what is left is the force path itself, held to the same 7.9e-7 of max |qfrc_actuator|.  Measured on the MI355X: at most
    5.14e-9 (median 4.2e-13)."""
    by_act, by_total, nefc, warn = _inverse_round_trip(1e-12)
    _report('opt_tolerance 1e-12', by_act, by_total, nefc, warn)
    assert by_act.max() < TOL_INVERSE


def test_fp32_batch_with_forces_runs_and_stays_finite():
    M, B = _walk_batch(512, precision=32)
    rng = np.random.default_rng(8)
    B.set('XFRC_APPLIED', _random_wrenches(M, 512, rng, scale=1.0).reshape(512, -1))
    B.set('QFRC_APPLIED', rng.normal(size=(512, M.dim('nv')))*1e-3)
    _, P = _walk_batch(512, precision=32)
    _rollout(B, 20, seed=3); _rollout(P, 20, seed=3)
    for f in ('QPOS', 'QVEL', 'OBS', 'REWARD', 'SENSORDATA'):
        assert np.isfinite(B.get(f)).all(), f
    assert not np.array_equal(B.get('QPOS'), P.get('QPOS'))                 # the forces act
    assert (B.get('STEP_TYPE') == 1).all()


def test_control_callback_restates_the_reference_ctrl_callback_test():
    """The reference's test_ctrl_callback (tests/test_core.py): a control callback writes qfrc_applied = qfrc_actuator x sin(arange) on 29
    of the 108 dofs; after every one of 100 steps QFRC_APPLIED holds that product there and zero elsewhere.  Here the callback runs once
    per control step (before it), so the product is of the qfrc_actuator the callback read."""
    import torch
    from flybody_amd import fly_envs, perturbations
    dof_ids = [*range(6, 9), *range(42, 53), *range(75, 90)]
    rest = [i for i in range(108) if i not in dof_ids]
    noise = np.sin(np.arange(len(dof_ids)))
    seen = []

    def callback(env):
        fa = env.batch.get('QFRC_ACTUATOR')
        v = env.applied_forces()['qfrc_applied']
        v[:, dof_ids] = torch.from_numpy(fa[:, dof_ids]*noise).to(v)
        seen.append(fa[:, dof_ids]*noise)

    env = fly_envs.BatchedFlyEnv(n_env=4, control_callback=callback)
    assert env.model.dim('nv') == 108
    views = env.applied_forces()
    assert views['qfrc_applied'].shape == (4, 108) and views['xfrc_applied'].shape == (4, 68, 6) and views['qfrc_applied'].dtype == torch.float64
    env.reset()
    rng = np.random.default_rng(0)
    moved = 0.0
    for k in range(100):
        action = rng.uniform(-1.0, 1.0, (4, 59))
        if k % 2:
            env.step(action)
        else:
            env.step_tensor(torch.from_numpy(action.astype(np.float32)).cuda()); torch.cuda.synchronize()
        qa = env.batch.get('QFRC_APPLIED')
        assert len(seen) == k + 1
        assert np.allclose(qa[:, dof_ids], seen[-1], rtol=1e-15, atol=0) and (qa[:, rest] == 0).all()
        moved = max(moved, np.abs(qa).max())
    assert moved > 0
    # the host-side reset zeroes the arrays (MuJoCo's reset clears them); perturbations.set_body_wrench / clear
    env.control_callback = None
    perturbations.set_body_wrench(env, ['thorax', 'wing_left'], force=[0.0, 0.0, 1e-3], env_ids=[1, 3])
    xa = env.batch.get('XFRC_APPLIED').reshape(4, 68, 6)
    ids = perturbations.body_ids(env.model, ['thorax', 'wing_left'])
    assert (xa[[1, 3]][:, ids, 2] == 1e-3).all() and np.count_nonzero(xa) == 4
    env.reset()
    assert not env.batch.get('XFRC_APPLIED').any() and not env.batch.get('QFRC_APPLIED').any() and env.batch.forces_active
    perturbations.clear(env)
    assert not env.batch.forces_active
    env.step(rng.uniform(-1.0, 1.0, (4, 59)))
