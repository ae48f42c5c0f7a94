"""fb_batch_inverse (inverse dynamics, csrc/fb_inverse.hpp) on the MI355X: parity with the CPU oracle's forward pass, forward-then-inverse
round trips after random-action rollouts on all three tasks and both engine binaries, trajectory inverse dynamics on substep-by-substep
recordings, and a control step after an inverse."""
import numpy as np
import pytest

from conftest import random_state

pytestmark = pytest.mark.gpu

_rel = lambda a, b: np.abs(np.asarray(a).ravel() - np.asarray(b).ravel()).max() / max(np.abs(np.asarray(b)).max(), 1e-300)

# GPU vs the oracle's forward pass (noslip off): the Newton stop test's gap.  Measured on MI355X over these 64 states (nefc 15 - 121):
# at most 7.7e-6 of max |qfrc_actuator| (median 1.1e-9), 5.0e-8 of max |efc_force|; the bounds leave a factor 10 (the emulation build,
# tests/test_inverse_emulation.py, measured 7.9e-7 / 1.0e-8 on its 8 states)
TOL_ORACLE = 1e-4
TOL_ORACLE_EFC = 5e-7
# Round trip forward -> inverse on the engine itself, per environment, relative to the environment's max |qfrc_actuator| / max |efc_force|:
# (qfrc bound, efc bound).  Measured on MI355X over 4096 environments after the 30-step random-action rollout below, identical on both
# engine builds: walk_imitation 1.7e-6 / 8.9e-7 (nefc 4 - 23), flight_imitation 8.0e-13 / 2.2e-12 (nefc 0 - 6, mean 0.6),
# walk_on_ball 6.8e-7 / 3.6e-7 (nefc 3 - 31).  Bounds: about 10 x that.
_ROUNDTRIP = {'walk_imitation': (2e-5, 1e-5), 'flight_imitation': (1e-11, 3e-11), 'walk_on_ball': (1e-5, 5e-6)}


def _arrays(name, noslip=False):
    from flybody_amd import engine
    a = dict(engine.load_npz(f'{engine.ASSETS}/{name}.npz'))
    if not noslip:
        a['opt_noslip_iterations'] = np.array(0)          # noslip is not inverted (fb_inverse.hpp)
    return a


def _batch(name, n, dense=False, noslip=False):
    from flybody_amd import engine
    from flybody_amd.reference import constant_speed_trajectory, default_walking_reference
    M = engine.Model(_arrays(name, noslip), dense=dense)
    B = engine.Batch(M, n, precision=64)
    if name == 'walk_imitation':
        qp, qv = default_walking_reference()
        B.set_reference(qp, qv, terminal_com_dist=float('inf'))
    elif name == 'flight_imitation':
        from flybody_amd.wbpg import build_tables
        B.set_wbpg(build_tables(), seed=0)
        qp, qv = constant_speed_trajectory(200, 20.0, init_pos=(0, 0, 1), body_rot_angle_y=-47.5, control_timestep=2e-4)
        B.set_reference(qp, qv, future_steps=5, terminal_com_dist=2.0, time_limit=0.6)
    else:
        B.set_time_limit(2.0)
    B.reset()
    return M, B


def _rollout(B, steps, seed):
    import torch
    act = torch.empty(B.n_env, B.model.dim('nact'), device='cuda')
    for k in range(steps):
        B.random_actions(act.data_ptr(), k, seed=seed, dist=1)
        B.step_ptr(act.data_ptr())
    torch.cuda.synchronize()


def test_parity_with_oracle_64_frames():
    from flybody_amd import engine
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    a = _arrays('walk_imitation')
    om = fbo.OracleModel(pack_model(a))
    ods, Q, V = [], [], []
    for e in range(64):
        r = np.random.default_rng(1000 + e)
        q, v = random_state(a, r, z=r.uniform(0.115, 0.14))
        od = fbo.OracleData(om); od.field('qpos')[:] = q; od.field('qvel')[:] = v; od.field('ctrl')[:] = r.uniform(-0.3, 0.3, 59)
        od.call('forward')
        ods.append(od); Q.append(q); V.append(v)
    B = engine.Batch(engine.Model(a), 64, precision=64)
    B.set('QPOS', np.array(Q)); B.set('QVEL', np.array(V)); B.set('QACC', np.array([od.field('qacc') for od in ods]))
    B.inverse()
    qi, ef, nefc = B.get('QFRC_INVERSE'), B.get('EFC_FORCE'), B.get('NEFC')[:, 0]
    gaps = []
    for e, od in enumerate(ods):
        n = int(od.scalar('nefc'))
        assert nefc[e] == n, e
        gaps.append((_rel(qi[e], od.field('qfrc_actuator')), _rel(ef[e][:n], od.field('efc_force')[:n]) if n else 0.0))
    g = np.array(gaps)
    print('oracle parity: qfrc max %.2e median %.2e | efc max %.2e, nefc %d-%d' % (g[:, 0].max(), np.median(g[:, 0]), g[:, 1].max(), nefc.min(), nefc.max()))
    assert g[:, 0].max() < TOL_ORACLE and g[:, 1].max() < TOL_ORACLE_EFC


@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('task', ['walk_imitation', 'flight_imitation', 'walk_on_ball'])
def test_round_trip_4096_after_rollout(task, dense):
    """forward then inverse returns QFRC_ACTUATOR and EFC_FORCE, at the states of a 30-step random-action rollout (varied contacts)."""
    M, B = _batch(task, 4096, dense=dense)
    _rollout(B, 30, seed=5)
    B.forward()
    fa, ef0, nefc = B.get('QFRC_ACTUATOR'), B.get('EFC_FORCE'), B.get('NEFC')[:, 0]
    qacc = B.get('QACC')
    B.inverse()
    qi, ef = B.get('QFRC_INVERSE'), B.get('EFC_FORCE')
    assert np.array_equal(B.get('QACC'), qacc) and np.array_equal(B.get('NEFC')[:, 0], nefc)
    scale = np.maximum(np.abs(fa).max(axis=1), 1e-300)
    gq = np.abs(qi - fa).max(axis=1)/scale
    mask = np.arange(ef.shape[1])[None, :] < nefc[:, None]
    d = np.where(mask, np.abs(ef - ef0), 0).max(axis=1)
    ge = np.where(nefc > 0, d/np.maximum(np.where(mask, np.abs(ef0), 0).max(axis=1), 1e-300), 0)
    print('%s %s: nefc %d-%d (mean %.1f) | qfrc gap max %.2e p99 %.2e median %.2e | efc gap max %.2e p99 %.2e'
          % (task, 'dense' if dense else 'default', nefc.min(), nefc.max(), nefc.mean(), gq.max(), np.quantile(gq, 0.99), np.median(gq),
             ge.max(), np.quantile(ge, 0.99)))
    tq, te = _ROUNDTRIP[task]
    assert np.isfinite(qi).all() and gq.max() < tq and ge.max() < te


def test_trajectory_inverse_dynamics_on_substeps():
    """qpos recorded substep by substep from a rollout: trajectory_inverse_dynamics (diff / diff, FB_INV_DISCRETE) recovers every substep's
    qfrc_actuator; the root residual is what the actuators put on the root (the adhesion wrench), nothing unexplained."""
    import torch
    from flybody_amd.inverse_dynamics import trajectory_inverse_dynamics
    M, B = _batch('walk_imitation', 16)
    _rollout(B, 5, seed=9)
    act = torch.empty(16, M.dim('nact'), device='cuda')
    B.random_actions(act.data_ptr(), 5, seed=9, dist=1); B.step_ptr(act.data_ptr()); torch.cuda.synchronize()
    Q, FA = [B.get('QPOS')], []
    for _ in range(12):
        B.substep(1)
        FA.append(B.get('QFRC_ACTUATOR')); Q.append(B.get('QPOS'))
    Q, FA = np.array(Q), np.array(FA)              # Q[t]: after t substeps; FA[t]: the force of substep t + 1 (computed at Q[t])
    h = float(M.arrays['opt_timestep'])
    worst, root = 0.0, 0.0
    for e in range(16):
        tr = trajectory_inverse_dynamics(M, Q[:, e], h)
        for k, f in enumerate(tr.frames):
            s = np.abs(FA[f, e]).max()
            worst = max(worst, np.abs(tr.result.qfrc_inverse[k] - FA[f, e]).max()/s)
            root = max(root, np.abs(tr.result.root_residual[k] - FA[f, e, :6]).max()/s)
    print('trajectory: qfrc gap max %.2e, root residual - actuator root force max %.2e' % (worst, root))
    # measured on MI355X: 1.6e-6 for both (16 environments x 11 frames: finite differences of positions, the solver's stop test)
    assert worst < 2e-5 and root < 2e-5


@pytest.mark.parametrize('task', ['walk_imitation', 'flight_imitation'])
def test_inverse_then_step_is_bit_identical(task):
    """An inverse on an environment's own state changes nothing the next control step reads (noslip on: the shipped model)."""
    import torch
    runs = []
    for do_inverse in (False, True):
        M, B = _batch(task, 512, noslip=True)
        _rollout(B, 3, seed=2)
        if do_inverse:
            B.inverse()
            B.synchronize()
        act = torch.empty(512, M.dim('nact'), device='cuda')
        for k in range(3, 5):
            B.random_actions(act.data_ptr(), k, seed=2, dist=1); B.step_ptr(act.data_ptr())
        torch.cuda.synchronize()
        runs.append({n: B.get(n) for n in ('QPOS', 'QVEL', 'ACT', 'QACC', 'OBS', 'REWARD', 'EFC_FORCE', 'SENSORDATA')})
    for n in runs[0]:
        assert np.array_equal(runs[0][n], runs[1][n]), n
