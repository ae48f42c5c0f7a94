"""GPU parity: the HIP engine (through the C-ABI) against the FP64 CPU oracle on identical inputs.

Tolerances (written here, as the task statement requires):
  * FP64 kernel vs FP64 oracle, single forward evaluation:  1e-9 relative on every smooth-dynamics
    stage output (different summation orders only) and 1e-6 on solver-dependent outputs (the Newton
    solver -- the model's default, fb_newton.hpp / fbo_constraint.c: solve_newton -- stops on a 1e-8
    bound on the scaled cost decrement, so the last iteration may differ; Newton runs at EVERY system size on both sides since
    round 5 -- d_newton_wide beyond one row per lane -- and block PGS, behind opt_solver = 0, stops on the same threshold: it is held
    against the oracle's PGS at these tolerances in tests/test_pgs_solver.py, CPU emulation and GPU);
  * FP64 kernel vs oracle over 20 ... 100 control steps (contacts, Newton, noslip):  1e-6 relative
    on qpos / qvel (contact-rich dynamics amplify rounding differences; measured ~1e-11);
  * FP32 kernel vs oracle, single forward evaluation:  2e-3 relative on accelerations.
"""
import numpy as np
import pytest

from conftest import random_state

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a = np.asarray(a, float).ravel(); b = np.asarray(b, float).ravel()
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope='module')
def gpu_model(walk_arrays):
    from flybody_amd import engine
    return engine.Model(walk_arrays)


def _oracle(oracle_model):
    from oracle import fbo
    return fbo.OracleData(oracle_model)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_forward_stage_parity_fp64(gpu_model, oracle_model, walk_arrays, seed):
    from flybody_amd import engine
    rng = np.random.default_rng(seed)
    B = engine.Batch(gpu_model, 8, precision=64)
    od = _oracle(oracle_model)
    q, v = random_state(walk_arrays, rng)
    ctrl = rng.uniform(-0.3, 0.3, gpu_model.dim('nu')); act = rng.uniform(-0.2, 0.2, gpu_model.dim('na'))
    B.set('QPOS', q); B.set('QVEL', v); B.set('CTRL', ctrl); B.set('ACT', act)
    od.field('qpos')[:] = q; od.field('qvel')[:] = v; od.field('ctrl')[:] = ctrl; od.field('act')[:] = act
    B.forward(); B.synchronize(); od.call('forward')
    assert int(B.get('NCON')[0, 0]) == int(od.scalar('ncon'))
    assert int(B.get('NEFC')[0, 0]) == int(od.scalar('nefc'))
    n = int(od.scalar('nefc'))
    for name, of, tol in [('XPOS', 'xpos', 1e-9), ('XQUAT', 'xquat', 1e-9), ('QM', 'qM', 1e-9), ('QFRC_BIAS', 'qfrc_bias', 1e-9),
                          ('QFRC_PASSIVE', 'qfrc_passive', 1e-9), ('QFRC_ACTUATOR', 'qfrc_actuator', 1e-9),
                          ('QACC_SMOOTH', 'qacc_smooth', 1e-9), ('QFRC_CONSTRAINT', 'qfrc_constraint', 1e-6),
                          ('QACC', 'qacc', 1e-6), ('SENSORDATA', 'sensordata', 1e-6)]:
        g = B.get(name)
        assert _rel(g[0], od.field(of)) < tol, name
        assert np.array_equal(g[0], g[-1]), name + ' differs between identical environments'
    assert _rel(B.get('EFC_FORCE')[0][:n], od.field('efc_force')[:n]) < 1e-6
    oc = od.contacts(); gc = B.get('CONTACT')[0].reshape(64, 8)[:len(oc)]
    assert _rel(gc[:, :7], oc[:, :7]) < 1e-9


def test_rollout_parity_fp64(gpu_model, oracle_model, reference_traj):
    """The north_star tolerance, for EVERY environment: the FP64 build against the FP64 oracle over 20 control steps
    (200 physics steps; the statement asks for 100) of the reference's env-test workload (tests/test_walking_env.py:60-72:
    U(-0.5, 0.5) actions, terminal_com_dist = inf), eight environments with their own action sequences.
    Tolerance asserted: 1e-6 relative on qpos and qvel (north_star: 1e-4; measured: ~1e-11)."""
    import torch
    from flybody_amd import engine
    qp, qv = reference_traj
    n = 9                                                      # environment 8 repeats the actions of environment 0
    B = engine.Batch(gpu_model, n, precision=64)
    B.set_reference(qp, qv, terminal_com_dist=float('inf'))
    B.reset()
    ods = []
    for e in range(n - 1):
        od = _oracle(oracle_model); od.configure_env(qp, qv, terminal_com_dist=float('inf')); od.env_reset(); ods.append(od)
    assert np.allclose(B.get('OBS')[0], ods[0].field('obs'), rtol=1e-5, atol=1e-4)
    rng = np.random.default_rng(0)
    for k in range(20):
        a = rng.uniform(-0.5, 0.5, (n, 59)).astype(np.float32)     # tests/test_walking_env.py:71
        a[n - 1] = a[0]
        act = torch.from_numpy(a).cuda()
        B.step_ptr(act.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for e in range(n - 1):
            ods[e].env_step(a[e].astype(np.float64))
        assert B.get('REWARD')[0, 0] == 1.0                   # inference mode: reward == 1
        assert [int(v) for v in B.get('STEP_TYPE')[:n - 1, 0]] == [int(od.scalar('step_type')) for od in ods]
    Q, V = B.get('QPOS'), B.get('QVEL')
    for e in range(n - 1):
        assert _rel(Q[e], ods[e].field('qpos')) < 1e-6, e
        assert _rel(V[e], ods[e].field('qvel')) < 1e-6, e
    assert np.allclose(B.get('OBS')[0], ods[0].field('obs'), rtol=1e-4, atol=1e-3)
    assert np.array_equal(Q[0], Q[n - 1])                     # same actions, same trajectory, bit for bit


def _oracle_envs(oracle_model, n, qp, qv, **kw):
    ods = []
    for _ in range(n):
        od = _oracle(oracle_model); od.configure_env(qp, qv, **kw); od.env_reset(); ods.append(od)
    return ods


def _clipped_normal(rng, shape):
    return np.clip(rng.normal(size=shape), -1.0, 1.0)


def test_rollout_parity_fp64_100_control_steps(gpu_model, oracle_model, reference_traj):
    """The stated contract at its stated length: 100 control steps (1000 physics steps) for 64 environments with their own
    action streams -- half under the reference env-test's U(-0.5, 0.5) (tests/test_walking_env.py:71), half under the
    bench's clipped N(0, 1) -- with the longest-first launch order (k_order) active from the second step on.
    Asserted: 1e-6 relative on qpos and qvel of EVERY environment at steps 50 and 100 (north_star: 1e-4), observation
    rtol 1e-5, reward / step type equal at every step."""
    import torch
    from oracle import fbo
    from flybody_amd import engine
    qp, qv = reference_traj
    n = 64
    B = engine.Batch(gpu_model, n, precision=64)
    B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    ods = _oracle_envs(oracle_model, n, qp, qv, terminal_com_dist=float('inf'))
    rngs = [np.random.default_rng(1000 + e) for e in range(n)]
    st = torch.cuda.current_stream().cuda_stream
    for k in range(1, 101):
        a = np.stack([rngs[e].uniform(-0.5, 0.5, 59) if e < n // 2 else _clipped_normal(rngs[e], 59) for e in range(n)]).astype(np.float32)
        act = torch.from_numpy(a).cuda()
        B.step_ptr(act.data_ptr(), st)
        fbo.step_batch(ods, a.astype(np.float64))
        if k % 10 == 0 or k == 1:
            torch.cuda.synchronize()
            assert (B.get('REWARD') == 1.0).all()
            assert B.get('STEP_TYPE').ravel().tolist() == [int(od.scalar('step_type')) for od in ods]
        if k in (50, 100):
            Q, V = B.get('QPOS'), B.get('QVEL')
            eq = np.array([_rel(Q[e], ods[e].field('qpos')) for e in range(n)])
            ev = np.array([_rel(V[e], ods[e].field('qvel')) for e in range(n)])
            assert eq.max() < 1e-6 and ev.max() < 1e-6, (k, eq.max(), int(eq.argmax()), ev.max(), int(ev.argmax()))
    order = B.get('LAUNCH_ORDER').ravel()
    assert sorted(order.tolist()) == list(range(n)) and not np.array_equal(order, np.arange(n))      # the re-ordered launch ran
    obs = B.get('OBS')
    for e in range(n):
        assert np.allclose(obs[e], ods[e].field('obs'), rtol=1e-5, atol=2e-6), e


def test_rollout_parity_across_auto_reset_fp64(gpu_model, oracle_model, reference_traj):
    """An episode boundary inside the compared rollout: the default snippet ends after 235 control steps (LAST with discount
    1), step 236 is the auto-reset (FIRST) and the next episode starts.  Step types, rewards and discounts are compared at
    every step; states at step 100 (1e-6), at the end of the episode (north_star's 1e-4: 2350 physics steps of chaotic
    contact dynamics) and five steps into the second episode (1e-6 again: the reset wipes the accumulated divergence)."""
    import torch
    from oracle import fbo
    from flybody_amd import engine
    qp, qv = reference_traj
    n = 8
    B = engine.Batch(gpu_model, n, precision=64)
    B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    ods = _oracle_envs(oracle_model, n, qp, qv, terminal_com_dist=float('inf'))
    rng = np.random.default_rng(7)
    st = torch.cuda.current_stream().cuda_stream
    seen = []
    for k in range(1, 242):
        a = (rng.uniform(-0.5, 0.5, (n, 59)) if k % 2 else _clipped_normal(rng, (n, 59))).astype(np.float32)
        act = torch.from_numpy(a).cuda()
        B.step_ptr(act.data_ptr(), st)
        fbo.step_batch(ods, a.astype(np.float64))
        torch.cuda.synchronize()
        stg = B.get('STEP_TYPE').ravel().tolist()
        assert stg == [int(od.scalar('step_type')) for od in ods], k
        assert np.array_equal(B.get('DISCOUNT').ravel(), np.array([od.scalar('discount') for od in ods], np.float32)), k
        seen.append(stg[0])
        if k in (100, 235, 241):
            tol = 1e-4 if k == 235 else 1e-6
            Q, V = B.get('QPOS'), B.get('QVEL')
            for e in range(n):
                assert _rel(Q[e], ods[e].field('qpos')) < tol and _rel(V[e], ods[e].field('qvel')) < tol, (k, e)
        if k == 236:
            obs = B.get('OBS')
            for e in range(n):
                assert np.allclose(obs[e], ods[e].field('obs'), rtol=1e-5, atol=2e-6), e          # the reset observation
    assert seen[234] == 2 and seen[235] == 0 and seen[236] == 1 and seen.count(2) == 1
    assert (B.get('STEP_COUNT').ravel() == 5).all()


def test_numeric_guards_on_gpu(gpu_model, oracle_model, reference_traj):
    """The two numeric guards of the task, on the GPU against the oracle: NaN actions are zeroed
    (tasks/walk_imitation.py:148) and a blown-up state terminates the episode with discount 0 (tasks/base.py:222-225,
    ||qacc|| > 1e14 or non-finite), after which the auto-reset restores a finite state."""
    import torch
    from flybody_amd import engine
    qp, qv = reference_traj
    n = 4
    B = engine.Batch(gpu_model, n, precision=64)
    B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    ods = _oracle_envs(oracle_model, n, qp, qv, terminal_com_dist=float('inf'))
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(3)
    a = rng.uniform(-0.5, 0.5, (n, 59)).astype(np.float32)
    a[1, ::3] = np.nan; a[2, :] = np.nan                     # env 1: some NaN entries, env 2: all NaN
    for _ in range(3):
        act = torch.from_numpy(a).cuda()
        B.step_ptr(act.data_ptr(), st); torch.cuda.synchronize()
        for e in range(n):
            ods[e].env_step(a[e].astype(np.float64))
    Q = B.get('QPOS')
    assert np.isfinite(Q).all() and np.isfinite(B.get('OBS')).all()
    for e in range(n):
        assert _rel(Q[e], ods[e].field('qpos')) < 1e-9, e
    z = np.where(np.isnan(a), 0, a)                           # the same rollout with explicit zeros gives the same state
    B2 = engine.Batch(gpu_model, n, precision=64); B2.set_reference(qp, qv, terminal_com_dist=float('inf')); B2.reset()
    for _ in range(3):
        actz = torch.from_numpy(z).cuda()
        B2.step_ptr(actz.data_ptr(), st); torch.cuda.synchronize()
    assert np.array_equal(B2.get('QPOS'), Q)
    # blow-up: env 3 gets an absurd joint velocity -> ||qacc|| > 1e14 (or non-finite) -> LAST with discount 0
    V = B.get('QVEL'); V[3, 20:40] = 1e18; B.set('QVEL', V)
    ods[3].field('qvel')[20:40] = 1e18
    a0 = np.zeros((n, 59), np.float32)
    act0 = torch.from_numpy(a0).cuda()
    B.step_ptr(act0.data_ptr(), st); torch.cuda.synchronize()
    for e in range(n):
        ods[e].env_step(a0[e].astype(np.float64))
    stg = B.get('STEP_TYPE').ravel().tolist(); disc = B.get('DISCOUNT').ravel().tolist()
    assert stg == [1, 1, 1, 2] and disc == [1.0, 1.0, 1.0, 0.0]
    assert int(ods[3].scalar('step_type')) == 2 and ods[3].scalar('discount') == 0.0
    act0 = torch.from_numpy(a0).cuda()
    B.step_ptr(act0.data_ptr(), st); torch.cuda.synchronize()
    ods[3].env_step(a0[3].astype(np.float64))
    assert B.get('STEP_TYPE').ravel().tolist() == [1, 1, 1, 0] and int(ods[3].scalar('step_type')) == 0
    assert np.isfinite(B.get('QPOS')).all() and np.isfinite(B.get('OBS')).all()
    assert _rel(B.get('QPOS')[3], ods[3].field('qpos')) < 1e-9


def test_forward_parity_fp32(gpu_model, oracle_model, walk_arrays):
    from flybody_amd import engine
    rng = np.random.default_rng(3)
    B = engine.Batch(gpu_model, 4, precision=32)
    od = _oracle(oracle_model)
    q, v = random_state(walk_arrays, rng, z=0.14)
    q = q.astype(np.float32).astype(np.float64); v = v.astype(np.float32).astype(np.float64)
    B.set('QPOS', q); B.set('QVEL', v)
    od.field('qpos')[:] = q; od.field('qvel')[:] = v
    B.forward(); B.synchronize(); od.call('forward')
    assert _rel(B.get('XPOS')[0], od.field('xpos')) < 1e-5
    assert _rel(B.get('QM')[0], od.field('qM')) < 1e-4
    assert _rel(B.get('QACC_SMOOTH')[0], od.field('qacc_smooth')) < 2e-3


def test_full_size_properties(gpu_model, reference_traj):
    """BASELINE config 2 size (4096 envs): size-independent properties."""
    import torch
    from flybody_amd import engine
    qp, qv = reference_traj
    n = 4096
    B = engine.Batch(gpu_model, n, precision=32)
    B.set_reference(qp, qv, terminal_com_dist=float('inf'))
    B.reset()
    obs0 = B.get('OBS')
    assert np.array_equal(obs0[0], obs0[-1])
    g = torch.Generator(device='cuda'); g.manual_seed(0)
    acts = torch.randn(n, 59, device='cuda', generator=g).clamp_(-1, 1)
    acts[n // 2:] = acts[:n // 2]                      # second half replays the first half
    for _ in range(5):
        B.step_ptr(acts.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    q = B.get('QPOS')
    assert np.isfinite(q).all()
    assert np.array_equal(q[:n // 2], q[n // 2:])      # env-index independence (sharding invariant)
    assert np.abs(np.linalg.norm(q[:, 3:7], axis=1) - 1).max() < 1e-5
    assert (B.get('STEP_COUNT') == 5).all()
    assert (q[:, 2] > 0.02).all() and (q[:, 2] < 0.5).all()   # flies stay on the floor
    # partial reset only touches the listed environments
    ids = np.arange(0, n, 2, dtype=np.int32)
    B.reset(ids); B.synchronize()
    sc = B.get('STEP_COUNT').ravel()
    assert (sc[0::2] == 0).all() and (sc[1::2] == 5).all()


def test_rollout_tolerance_fp32(gpu_model, oracle_model, reference_traj):
    """FP32 build vs FP64 oracle, eight environments with their own U(-0.5, 0.5) action sequences: a STATISTICAL bound.

    A fly standing on six legs under random actions makes and breaks contacts every few steps, and each such event
    amplifies a rounding-level difference by ~1000x -- between FP32 and FP64, and just as much between two FP32 builds
    that differ only in FMA contraction (the host emulation of the same kernel source shows the same spread).  So for
    the FP32 build the north_star tolerance (1e-4 relative after 100 physics steps = 10 control steps) is asserted on the
    MEDIAN environment, with loose bounds on the worst one and at 500 physics steps; they catch systematic errors, not
    chaos.  The every-environment statement of the tolerance is test_rollout_parity_fp64 (1e-6 asserted, ~1e-11 measured),
    which is why bench.py's headline leg is the FP64 build."""
    import torch
    from flybody_amd import engine
    qp, qv = reference_traj
    n = 8
    B = engine.Batch(gpu_model, n, precision=32)
    B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    ods = []
    for e in range(n):
        od = _oracle(oracle_model); od.configure_env(qp, qv, terminal_com_dist=float('inf')); od.env_reset(); ods.append(od)
    rng = np.random.default_rng(0)
    for k in range(1, 51):
        a = rng.uniform(-0.5, 0.5, (n, 59)).astype(np.float32)
        act = torch.from_numpy(a).cuda()
        B.step_ptr(act.data_ptr(), torch.cuda.current_stream().cuda_stream)
        for e in range(n):
            ods[e].env_step(a[e].astype(np.float64))
        if k in (10, 50):
            torch.cuda.synchronize()
            Q, V = B.get('QPOS'), B.get('QVEL')
            eq = np.array([_rel(Q[e], ods[e].field('qpos')) for e in range(n)])
            ev = np.array([_rel(V[e], ods[e].field('qvel')) for e in range(n)])
            if k == 10:
                assert np.median(eq) < 1e-4 and np.median(ev) < 1e-3 and eq.max() < 5e-3, (eq, ev)
            else:
                assert np.median(eq) < 5e-3 and np.median(ev) < 1e-1 and eq.max() < 5e-2, (eq, ev)


def test_fp32_control_step_every_environment(gpu_model, reference_traj):
    """A bound on EVERY environment for the FP32 build (the one train_dmpo.py trains on), free of the chaotic amplification that forces
    test_rollout_tolerance_fp32 onto the median: 256 environments are rolled out for 25 control steps on the FP64 build, their
    states (rounded to FP32) are injected into an FP32 and an FP64 batch, and ONE control step (10 physics steps: collision, constraint
    solve, noslip, integration, observation epilogue) is taken from identical states with identical actions.  The local error of the
    FP32 step is asserted per environment (`training physics has no per-env bound`)."""
    import torch
    from flybody_amd import engine
    qp, qv = reference_traj
    n = 256
    st = torch.cuda.current_stream().cuda_stream
    B64 = engine.Batch(gpu_model, n, precision=64); B32 = engine.Batch(gpu_model, n, precision=32)
    for B in (B64, B32):
        B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    g = torch.Generator(device='cuda'); g.manual_seed(11)
    a = torch.empty(n, 59, device='cuda')
    for _ in range(25):
        a.normal_(generator=g).clamp_(-1, 1)
        B64.step_ptr(a.data_ptr(), st); B32.step_ptr(a.data_ptr(), st)        # (the FP32 batch only advances its episode clock)
    torch.cuda.synchronize()
    r32 = lambda x: x.astype(np.float32).astype(np.float64)
    q, v, act = r32(B64.get('QPOS')), r32(B64.get('QVEL')), r32(B64.get('ACT'))
    q[:, 3:7] /= np.linalg.norm(q[:, 3:7], axis=1, keepdims=True)
    for B in (B64, B32):
        B.set('QPOS', q); B.set('QVEL', v); B.set('ACT', act); B.forward()
    a.normal_(generator=g).clamp_(-1, 1)
    B64.step_ptr(a.data_ptr(), st); B32.step_ptr(a.data_ptr(), st); torch.cuda.synchronize()
    Q64, Q32, V64, V32 = B64.get('QPOS'), B32.get('QPOS'), B64.get('QVEL'), B32.get('QVEL')
    assert np.isfinite(Q32).all() and np.isfinite(V32).all()
    eq = np.abs(Q32 - Q64).max(axis=1)/np.abs(Q64).max(axis=1); ev = np.abs(V32 - V64).max(axis=1)/np.abs(V64).max(axis=1)
    print('fp32 one-control-step error: qpos median %.2e p99 %.2e max %.2e; qvel median %.2e p99 %.2e max %.2e'
          % (np.median(eq), np.quantile(eq, 0.99), eq.max(), np.median(ev), np.quantile(ev, 0.99), ev.max()))
    assert int(B32.get('WARN').max()) == 0
    # Measured (256 environments): qpos median 1.5e-7 / p99 4.0e-5 / max 8.9e-4, qvel median 6.9e-6 / p99 2.4e-3 / max 7.3e-2.  The
    # north_star tolerance (1e-4 relative on qpos) therefore holds for 99 % of the environments after these 10 physics steps; the
    # worst ones are contacts that close one substep earlier or later in FP32 (a leg joint velocity then differs by percents of the
    # largest velocity).  Asserted for EVERY environment: 5e-3 / 0.3, an order above the measured maxima -- a systematic FP32 error
    # (wrong constant, missing term) moves all of them far beyond that.
    assert np.median(eq) < 2e-6 and np.quantile(eq, 0.99) < 1e-4 and eq.max() < 5e-3, (np.median(eq), eq.max())
    assert np.median(ev) < 1e-4 and np.quantile(ev, 0.99) < 1e-2 and ev.max() < 0.3, (np.median(ev), ev.max())


def flight_rollout_vs_oracle(lib_path, n, steps, checkpoints, on_gpu=True):
    """n flight_imitation environments with their own U(-1, 1)^12 action streams and initial wing-beat phases against n oracle
    environments: step type, discount and reward at every step, state and observation at the checkpoints {step: tolerance}.
    Returns the [steps][n] matrix of step types.  (Also run on the kernel-source emulation by tests/test_kernel_emulation.py.)"""
    import os
    from conftest import ROOT
    from flybody_amd import engine
    from flybody_amd.mjcf_compile import qrot
    from flybody_amd.model_blob import load_npz, pack_model
    from flybody_amd.reference import constant_speed_trajectory
    from flybody_amd.wbpg import build_tables
    from oracle import fbo
    arr = load_npz(os.path.join(ROOT, 'flybody_amd', 'assets', 'flight_imitation.npz'))
    M = engine.Model(arr, lib_path=lib_path); B = engine.Batch(M, n, precision=64)
    om = fbo.OracleModel(pack_model(arr))
    tabs = build_tables(); B.set_wbpg(tabs, seed=5)
    cq, cv = constant_speed_trajectory(200, 20.0, init_pos=(0, 0, 1), body_rot_angle_y=-47.5, control_timestep=2e-4)
    root = cq.copy()
    for i in range(len(root)):
        root[i, :3] = cq[i, :3] + qrot(cq[i, 3:], -arr['com_offset'])
    B.set_reference(root, cv, future_steps=5, terminal_com_dist=2.0, time_limit=0.6)
    ods = []
    for e in range(n):
        od = fbo.OracleData(om); od.set_wbpg(tabs, seed=5); od.set_env_id(e)
        od.configure_env(root, cv, future_steps=5, terminal_com_dist=2.0, time_limit=0.6); od.env_reset(); ods.append(od)
    B.reset()
    q0 = B.get('QPOS')
    assert len({tuple(np.round(q, 12)) for q in q0}) > n // 2                   # the environments start at different wing-beat phases
    for e in range(n):
        assert _rel(q0[e], ods[e].field('qpos')) < 1e-12, e
    rng = np.random.default_rng(1)
    types = []
    for k in range(1, steps + 1):
        a = rng.uniform(-1, 1, (n, 12)).astype(np.float32)
        if on_gpu:
            import torch
            act = torch.from_numpy(a).cuda()
            B.step_ptr(act.data_ptr(), torch.cuda.current_stream().cuda_stream); torch.cuda.synchronize()
        else:
            B.step_ptr(a.ctypes.data)
        fbo.step_batch(ods, a.astype(np.float64))
        stg = B.get('STEP_TYPE').ravel().tolist()
        assert stg == [int(od.scalar('step_type')) for od in ods], k
        assert np.array_equal(B.get('DISCOUNT').ravel(), np.array([od.scalar('discount') for od in ods], np.float32)), k
        assert np.abs(B.get('REWARD').ravel() - np.array([od.scalar('reward') for od in ods])).max() < 1e-5, k
        types.append(stg)
        if k in checkpoints:
            tol = checkpoints[k]
            Q, V, obs = B.get('QPOS'), B.get('QVEL'), B.get('OBS')
            for e in range(n):
                assert _rel(Q[e], ods[e].field('qpos')) < tol and _rel(V[e], ods[e].field('qvel')) < tol, (k, e)
                assert np.allclose(obs[e], ods[e].field('obs'), rtol=max(1e-5, 10*tol), atol=max(1e-5, 10*tol)), (k, e)
    assert (B.get('WARN_EVER') == 0).all()
    return np.array(types)


def test_flight_rollout_parity_fp64():
    """flight_imitation (BASELINE configs[3]) on the GPU against the oracle: 32 environments with their own U(-1, 1)^12 action
    streams and their own initial wing-beat phases (flight_imitation.py:128-129), through the full episode
    of 194 control steps, LAST -> FIRST (auto-reset) and into the second episode -- every environment compared: wing-beat
    generator, ellipsoid wing fluid forces, reward / step type / discount at every step; qpos / qvel at 1e-6 (step 50) and 1e-4
    (steps 150 and 200: up to 776 physics steps of wing-beat dynamics since the last reset), observations likewise."""
    t = flight_rollout_vs_oracle(None, 32, 200, {50: 1e-6, 150: 1e-4, 200: 1e-4})
    assert (t == 2).sum() >= 32                                   # every environment ended an episode (trajectory end or a crash) ...
    for e in range(t.shape[1]):
        last = np.where(t[:-1, e] == 2)[0]
        assert len(last) >= 1 and (t[last + 1, e] == 0).all(), e   # ... and restarted with FIRST on the next step


@pytest.mark.parametrize('dense', [False, True])
def test_flight_batch_substep_scheduler_bit_equal_to_per_wave(dense, monkeypatch):
    """BASELINE configs[3] at its bench size: 8192 flight_imitation environments exceed the resident wave slots of both builds, so
    the batch is stepped by the substep scheduler (round 4: flight as well -- profiles/r4/flight_variants.txt).  Same keyed U(-1, 1)
    actions, 12 control steps (48 physics steps, own wing-beat phases): state, observations and rewards are bit-identical to the
    one-wave-per-environment path (FB_NO_TICKETS=1), whose rollouts test_flight_rollout_parity_fp64 holds against the oracle."""
    import os
    import torch
    from conftest import ROOT
    from flybody_amd import engine
    from flybody_amd.mjcf_compile import qrot
    from flybody_amd.model_blob import load_npz
    from flybody_amd.reference import constant_speed_trajectory
    from flybody_amd.wbpg import build_tables
    arr = load_npz(os.path.join(ROOT, 'flybody_amd', 'assets', 'flight_imitation.npz'))
    cq, cv = constant_speed_trajectory(200, 20.0, init_pos=(0, 0, 1), body_rot_angle_y=-47.5, control_timestep=2e-4)
    root = cq.copy()
    for i in range(len(root)):
        root[i, :3] = cq[i, :3] + qrot(cq[i, 3:], -arr['com_offset'])
    tabs = build_tables(); n = 8192; out = []
    for tickets in (True, False):
        if tickets: monkeypatch.delenv('FB_NO_TICKETS', raising=False)
        else: monkeypatch.setenv('FB_NO_TICKETS', '1')
        M = engine.Model(arr, lib_path=engine.HIP_LIB_DENSE if dense else None)
        B = engine.Batch(M, n, precision=64)
        assert B.substep_scheduler == tickets and B.resident_slots == (3072 if dense else 2048)
        B.set_wbpg(tabs, seed=5); B.set_reference(root, cv, future_steps=5, terminal_com_dist=2.0, time_limit=0.6); B.reset()
        a = torch.empty(n, 12, device='cuda'); st = torch.cuda.current_stream().cuda_stream
        for k in range(12):
            B.random_actions(a.data_ptr(), k, seed=9, dist=1, stream=st); B.step_ptr(a.data_ptr(), st)
        B.synchronize(st)
        assert (B.get('WARN_EVER') == 0).all()
        out.append([B.get(f).copy() for f in ('QPOS', 'QVEL', 'ACT', 'OBS', 'REWARD', 'STEP_COUNT')])
        del B, M
    assert np.isfinite(out[0][0]).all() and len({tuple(np.round(q, 9)) for q in out[0][0][:256]}) > 128
    for x, y in zip(*out):
        assert np.array_equal(x, y)


def test_launch_order_on_gpu(gpu_model, reference_traj):
    """Scheduling state of the step kernel: every environment records the duration of its control step (100 MHz ticks),
    and k_order sorts the next launch longest-first.  Results do not depend on the order (same actions, same states)."""
    import torch
    from flybody_amd import engine
    qp, qv = reference_traj
    n = 512
    B = engine.Batch(gpu_model, n, precision=64)
    B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    a = torch.from_numpy(np.tile(np.random.default_rng(0).uniform(-0.3, 0.3, 59).astype(np.float32), (n, 1))).cuda()
    for _ in range(3):
        B.step_ptr(a.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    order = B.get('LAUNCH_ORDER').ravel(); ticks = B.get('STEP_TICKS').ravel()
    assert sorted(order.tolist()) == list(range(n))
    assert ticks.min() > 1000 and ticks.max() < 100_000_000            # between 10 us and 1 s
    c = ticks[order].astype(np.int64)
    assert np.all(c[:-1] >= c[1:] - (ticks.max() // 255 + 1))
    q = B.get('QPOS')
    assert np.array_equal(q, np.tile(q[0], (n, 1)))


@pytest.mark.parametrize('precision', [64, 32])
def test_solver_paths_by_system_size_gpu(gpu_model, oracle_model, walk_arrays, precision):
    """Same as tests/test_kernel_emulation.py::test_solver_paths_by_system_size, on the GPU: Delassus matrix in LDS, small
    system from the global row, wide system (> 64 rows) -- all three against the oracle's constraint forces."""
    from flybody_amd import engine
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    from conftest import random_state
    cases = [(1, 0.14), (1, 0.135), (1, 0.13), (1, 0.125), (3, 0.12), (1, 0.05)]     # nefc 24, 36, 54, 66, 114, 192 (the row cap)
    # Round 5: Newton at every size (d_newton_wide beyond one row per lane) against the UNcapped oracle -- rounds 3-4 ran block PGS
    # beyond 64 rows and were compared with an oracle capped the same way; VERDICT r4 item 5 asked for exactly this comparison at 1e-6.
    B = engine.Batch(gpu_model, len(cases), precision=precision)
    ods, Q, V = [], [], []
    for seed, z in cases:
        q, v = random_state(walk_arrays, np.random.default_rng(seed), z=z)
        if precision == 32:
            q = q.astype(np.float32).astype(float); v = v.astype(np.float32).astype(float)
        od = _oracle(oracle_model); od.field('qpos')[:] = q; od.field('qvel')[:] = v; od.call('forward')
        ods.append(od); Q.append(q); V.append(v)
    B.set('QPOS', np.array(Q)); B.set('QVEL', np.array(V))
    B.forward()
    nefc = [int(od.scalar('nefc')) for od in ods]
    assert min(nefc) <= 29 and any(36 < n <= 64 for n in nefc) and any(64 < n < 192 for n in nefc) and max(nefc) == 192
    assert not (B.get('WARN').ravel() & engine.WARN_BITS['SOLVER_FALLBACK']).any()          # cannot be raised any more
    if precision == 64:
        assert B.get('NEFC').ravel().tolist() == nefc
        assert B.get('SOLVER_NITER').ravel().tolist() == [int(od.scalar('solver_niter')) for od in ods]
    for e, od in enumerate(ods):
        n = nefc[e]
        assert _rel(B.get('QACC')[e], od.field('qacc')) < (1e-6 if precision == 64 else 3e-2), (e, n)
        if precision == 64:
            assert _rel(B.get('EFC_FORCE')[e][:n], od.field('efc_force')[:n]) < 1e-6, (e, n)
    if precision == 64:
        # the size statistics the bench reports (FB_SIZE_STATS) saw these systems
        ss = B.get('SIZE_STATS').reshape(-1, 4)
        assert ss[:, 1].tolist() == nefc and ss[:, 3].tolist() == [int(n > 64) for n in nefc] and ss[:, 2].tolist() == [int(n > 32) for n in nefc]
        assert (ss[:, 0] == B.get('NCON').ravel()).all()


@pytest.mark.gpu
def test_dense_residency_build_matches_the_oracle(oracle_model, reference_traj):
    """The FB_F64_DENSE build of the same sources (12 FP64 environments per CU: 23-row LDS Delassus matrix, LDS overlay for wider
    systems, 168-VGPR stage budget -- engine.HIP_LIB_DENSE, used by bench.py's pipelined_dense_mode) against the FP64 oracle:
    1e-6 on qpos / qvel of every one of 32 environments after 40 control steps of N(0, 1) actions."""
    import torch
    from oracle import fbo
    from flybody_amd import engine
    n, steps = 128, 40
    M = engine.Model.from_asset('walk_imitation', dense=True)
    assert 'flybody_engine' in M.L.fb_version().decode()
    B = engine.Batch(M, n, precision=64)
    qp, qv = reference_traj
    B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    ods = _oracle_envs(oracle_model, n, qp, qv, terminal_com_dist=float('inf'))
    rng = np.random.default_rng(17)
    st = torch.cuda.current_stream().cuda_stream
    widest = 0
    for k in range(steps):
        a = np.clip(rng.normal(size=(n, 59)), -1, 1).astype(np.float32)
        act = torch.from_numpy(a).cuda()
        B.step_ptr(act.data_ptr(), st)
        fbo.step_batch(ods, a.astype(np.float64))
        torch.cuda.synchronize()
        widest = max(widest, int(B.get('NEFC').max()))
    Q, V = B.get('QPOS'), B.get('QVEL')
    for e in range(n):
        assert _rel(Q[e], ods[e].field('qpos')) <= 1e-6 and _rel(V[e], ods[e].field('qvel')) <= 1e-6, e
    assert widest > 23                                             # (some systems did not fit the 23-row matrix: the overlay path ran)


# ------------------------------------------------------------------ the headline configuration itself
def _headline_run(models, sizes, steps, oracle_model, reference_traj, seed, streams):
    """`len(sizes)` sub-batches (own fb_batch handle, own HIP stream) stepping `steps` control steps of the bench's clipped
    N(0, 1) actions; 64 sampled environments spread over every sub-batch (first / last ids, ids around the residency boundary
    of 2048 resident FP64 environments, random ones) are replayed on the CPU oracle.  Returns the worst relative errors and the
    launch-order positions the sampled environments had."""
    import torch
    from oracle import fbo
    from flybody_amd import engine
    qp, qv = reference_traj
    rng = np.random.default_rng(seed)
    batches, samples, ods, positions = [], [], [], []
    per = 64 // len(sizes)
    for p, n in enumerate(sizes):
        B = engine.Batch(models[p], n, precision=64)
        B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
        batches.append(B)
        fixed = [0, 1, n - 2, n - 1] + ([2047, 2048, 2049, 3071, 3072] if n > 3072 else [n // 2 - 1, n // 2])
        ids = sorted(set(fixed) | set(rng.choice(n, per - len(fixed), replace=False).tolist()))
        samples.append(np.array(ids)); ods.append(_oracle_envs(oracle_model, len(ids), qp, qv, terminal_com_dist=float('inf')))
        positions.append([])
    torch.cuda.synchronize()
    for k in range(steps):
        acts = [np.clip(rng.normal(size=(n, 59)), -1, 1).astype(np.float32) for n in sizes]
        devs = []
        for p, B in enumerate(batches):
            with torch.cuda.stream(streams[p]):
                d = torch.from_numpy(acts[p]).cuda(non_blocking=False); devs.append(d)
                B.step_ptr(d.data_ptr(), streams[p].cuda_stream)
        for p in range(len(sizes)):
            fbo.step_batch(ods[p], acts[p][samples[p]].astype(np.float64))
        torch.cuda.synchronize()
        for p, B in enumerate(batches):
            # (a batch beyond the resident slots is stepped by the substep scheduler: no launch order, every environment shares the slots)
            order = np.arange(sizes[p]) if B.substep_scheduler else B.get('LAUNCH_ORDER').ravel()
            if k > 0:
                pos = np.empty(sizes[p], np.int64); pos[order] = np.arange(sizes[p]); positions[p].append(pos[samples[p]])
    eq = ev = 0.0
    for p, B in enumerate(batches):
        Q, V = B.get('QPOS'), B.get('QVEL')
        assert np.isfinite(Q).all()
        assert (B.get('WARN_EVER') == 0).all(), np.unique(B.get('WARN_EVER'))          # no cap was hit, no solver ran out of iterations
        for i, e in enumerate(samples[p]):
            eq = max(eq, _rel(Q[e], ods[p][i].field('qpos'))); ev = max(ev, _rel(V[e], ods[p][i].field('qvel')))
        obs = B.get('OBS')
        for i, e in enumerate(samples[p]):
            assert np.allclose(obs[e], ods[p][i].field('obs'), rtol=1e-5, atol=2e-6), (p, e)
    return eq, ev, [np.array(x) for x in positions]


@pytest.mark.parametrize('sched', ['substep', 'per_wave'])
@pytest.mark.parametrize('dense', [False, True])
def test_headline_batch_parity_fp64(gpu_model, oracle_model, reference_traj, dense, sched, monkeypatch):
    """BENCH configuration, checked against the oracle: FP64, 4096 environments in lock-step = twice the 2048 resident FP64
    environments (default build; the 12-per-CU build holds 3072), 30 control steps of the bench's clipped N(0, 1) actions.
    Both ways a control step of such a batch can be scheduled: `substep` -- the default: waves draw (environment, substep)
    tickets, consecutive substeps of an environment run on different waves and CUs of its XCD -- and `per_wave` (FB_NO_TICKETS=1:
    one environment per wave from the first to the last substep, two residency rounds in longest-first launch order).  64 sampled
    environments -- ids on both sides of the residency boundary, environments launched in the second round -- against the CPU
    oracle at 1e-6."""
    import torch
    from flybody_amd import engine
    if sched == 'per_wave': monkeypatch.setenv('FB_NO_TICKETS', '1')
    else: monkeypatch.delenv('FB_NO_TICKETS', raising=False)
    M = engine.Model.from_asset('walk_imitation', dense=True) if dense else gpu_model
    probe = engine.Batch(M, 4096, precision=64)
    assert probe.substep_scheduler == (sched == 'substep') and probe.resident_slots == (3072 if dense else 2048), (probe.substep_scheduler, probe.resident_slots)
    del probe
    eq, ev, pos = _headline_run([M], [4096], 30, oracle_model, reference_traj, seed=11, streams=[torch.cuda.current_stream()])
    assert eq < 1e-6 and ev < 1e-6, (eq, ev)
    resident = 3072 if dense else 2048
    second_round = (pos[0] >= resident)
    assert second_round.any(axis=0).sum() >= 16, second_round.any(axis=0).sum()        # sampled environments did run in the second round
    assert (~second_round).any(axis=0).sum() >= 16


@pytest.mark.parametrize('dense,parts', [(False, 2), (True, 3)])
def test_pipelined_sub_batches_parity_fp64(gpu_model, oracle_model, reference_traj, dense, parts):
    """bench.py's secondary legs (two_stream_mode: 2 x 2048 on two HIP streams, default build; pipelined_dense_mode: 3 sub-batches
    on three streams, 12-per-CU build) against the ORACLE, not against each other: sub-batches that overlap on the GPU share CUs,
    LDS and the L2 with launches of other handles -- 1e-6 on sampled environments of every sub-batch after 30 control steps."""
    import torch
    from flybody_amd import engine
    M = engine.Model.from_asset('walk_imitation', dense=True) if dense else gpu_model
    sizes = [4096 // parts + (1 if p < 4096 % parts else 0) for p in range(parts)]
    streams = [torch.cuda.Stream() for _ in range(parts)]
    eq, ev, _ = _headline_run([M]*parts, sizes, 30, oracle_model, reference_traj, seed=12, streams=streams)
    assert eq < 1e-6 and ev < 1e-6, (eq, ev)


@pytest.mark.parametrize('precision', [64, 32])
def test_neighbour_list_equals_testing_every_pair_gpu(reference_traj, precision, monkeypatch):
    """The collision mid phase's neighbour list (round 6, fb_collide.hpp) on the GPU, at the headline size under the substep scheduler (the list lives
    in the environment's row and is handed from wave to wave with it): 4096 environments x 40 control steps of the bench's action streams with the
    list and with FB_NO_NEIGHBOUR_LIST=1 (read at model load) -- every state word, contact count and row count identical."""
    import torch
    from flybody_amd import engine
    qp, qv = reference_traj
    out = []
    for flag in (None, '1'):
        if flag is None: monkeypatch.delenv('FB_NO_NEIGHBOUR_LIST', raising=False)
        else: monkeypatch.setenv('FB_NO_NEIGHBOUR_LIST', flag)
        M = engine.Model.from_asset('walk_imitation', dense=(precision == 64))
        B = engine.Batch(M, 4096, precision=precision)
        B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
        a = torch.empty(4096, M.dim('nact'), device='cuda'); st = torch.cuda.current_stream().cuda_stream
        for k in range(40):
            B.random_actions(a.data_ptr(), 500 + k, seed=3, stream=st); B.step_ptr(a.data_ptr(), st)
        torch.cuda.synchronize()
        out.append((B.get('QPOS').copy(), B.get('QVEL').copy(), B.get('NCON').copy(), B.get('NEFC').copy()))
        del B, M
    assert np.isfinite(out[0][0]).all() and int(out[0][2].max()) > 4
    for x, y in zip(*out):
        assert np.array_equal(x, y)


def test_random_actions_keyed_by_global_id(gpu_model):
    """fb_random_actions on the GPU: a shard sees the rows of the whole batch, explicit id lists likewise (tests/test_random_actions.py
    pins the generator itself on the host build)."""
    import torch
    from flybody_amd import engine
    B = engine.Batch(gpu_model, 8, precision=64)
    nact = gpu_model.dim('nact')
    whole = torch.empty(4096, nact, device='cuda'); lo = torch.empty(1000, nact, device='cuda'); hi = torch.empty(3096, nact, device='cuda')
    B.random_actions(whole.data_ptr(), 7, seed=5, env_id_base=100, n=4096)
    B.random_actions(lo.data_ptr(), 7, seed=5, env_id_base=100, n=1000); B.random_actions(hi.data_ptr(), 7, seed=5, env_id_base=1100, n=3096)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([lo, hi]), whole) and bool((whole.abs() <= 1).all())
    ids = torch.tensor([4195, 100, 2000], dtype=torch.int32, device='cuda'); pick = torch.empty(3, nact, device='cuda')
    B.random_actions(pick.data_ptr(), 7, seed=5, env_ids_dev_ptr=ids.data_ptr(), n=3); torch.cuda.synchronize()
    assert torch.equal(pick, whole[[4095, 0, 1900]])
    inside = whole[whole.abs() < 1]
    assert abs(float(inside.mean())) < 0.01 and abs(float((whole.abs() >= 1).float().mean()) - 0.3173) < 0.01


@pytest.mark.parametrize('dense', [False, True])
def test_single_stage_launches_equal_fused_step_gpu(gpu_model, reference_traj, dense):
    """fb_batch_stage (one stage of a control step per launch: the unit tools/stage_profile.py attributes hardware counters to) walks the
    stage sequence of the fused kernel: bit-identical state and observations after three control steps, both builds."""
    import torch
    from flybody_amd import engine
    M = engine.Model.from_asset('walk_imitation', dense=True) if dense else gpu_model
    qp, qv = reference_traj
    out = []
    for staged in (False, True):
        B = engine.Batch(M, 96, precision=64); B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
        a = torch.empty(96, M.dim('nact'), device='cuda'); st = torch.cuda.current_stream().cuda_stream
        seq = engine.stage_sequence(M.dim('nsubstep'))
        for k in range(3):
            B.random_actions(a.data_ptr(), k, seed=3, stream=st)
            if staged:
                for _, word in seq:
                    B.stage(word, a.data_ptr(), st)
            else:
                B.step_ptr(a.data_ptr(), st)
        B.synchronize(st)
        out.append([B.get(f).copy() for f in ('QPOS', 'QVEL', 'ACT', 'OBS', 'SENSORDATA', 'QACC', 'STEP_COUNT')])
    for x, y in zip(*out):
        assert np.array_equal(x, y)


def _sched_rollout(M, n, steps, seed, reference_traj, stream=None):
    import torch
    from flybody_amd import engine
    qp, qv = reference_traj
    st = (stream or torch.cuda.current_stream()).cuda_stream
    B = engine.Batch(M, n, precision=64); B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset(stream=st)
    a = torch.empty(n, M.dim('nact'), device='cuda')
    return B, a, st


@pytest.mark.parametrize('n', [64, 6144])
def test_substep_scheduler_stress_bit_equal_to_per_wave(gpu_model, reference_traj, n, monkeypatch):
    """Substep scheduler under stress: FB_TICKET_SLOTS=1 forces the ticket path for ANY batch.  64 environments on a GPU
    with thousands of idle wave slots: every ticket's successor is drawn at once by another wave, so nearly every ticket WAITS for its
    predecessor (the hand-over protocol runs hot); 6144 = three times the resident slots of the default build.  50 control steps,
    bit-equal to the one-environment-per-wave path, no FB_WARN bit."""
    import torch
    res = []
    for tickets in (True, False):
        if tickets: monkeypatch.setenv('FB_TICKET_SLOTS', '1'); monkeypatch.delenv('FB_NO_TICKETS', raising=False)
        else: monkeypatch.delenv('FB_TICKET_SLOTS', raising=False); monkeypatch.setenv('FB_NO_TICKETS', '1')
        B, a, st = _sched_rollout(gpu_model, n, 50, 21, reference_traj)
        assert B.substep_scheduler == tickets
        for k in range(50):
            B.random_actions(a.data_ptr(), k, seed=21, stream=st); B.step_ptr(a.data_ptr(), st)
        B.synchronize(st)
        assert (B.get('WARN_EVER') == 0).all()
        res.append((B.get('QPOS').copy(), B.get('QVEL').copy(), B.get('OBS').copy()))
        del B
    for x, y in zip(*res):
        assert np.array_equal(x, y)


def test_two_ticket_batches_on_two_streams(gpu_model, reference_traj, monkeypatch):
    """Two fb_batch handles of 4096 environments, each under the substep scheduler (own ticket and progress counters), stepped
    CONCURRENTLY on two HIP streams: each equals the same batch stepped alone, bit for bit."""
    import torch
    monkeypatch.delenv('FB_NO_TICKETS', raising=False); monkeypatch.delenv('FB_TICKET_SLOTS', raising=False)
    alone = []
    for seed in (31, 32):
        B, a, st = _sched_rollout(gpu_model, 4096, 12, seed, reference_traj)
        assert B.substep_scheduler
        for k in range(12):
            B.random_actions(a.data_ptr(), k, seed=seed, stream=st); B.step_ptr(a.data_ptr(), st)
        B.synchronize(st); alone.append(B.get('QPOS').copy()); del B
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    pair = [_sched_rollout(gpu_model, 4096, 12, seed, reference_traj, s) for seed, s in ((31, s1), (32, s2))]
    torch.cuda.synchronize()
    for k in range(12):
        for (B, a, st), seed in zip(pair, (31, 32)):
            B.random_actions(a.data_ptr(), k, seed=seed, stream=st); B.step_ptr(a.data_ptr(), st)
    for (B, a, st), ref in zip(pair, alone):
        B.synchronize(st)
        assert (B.get('WARN_EVER') == 0).all() and np.array_equal(B.get('QPOS'), ref)
