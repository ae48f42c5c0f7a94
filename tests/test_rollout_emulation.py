"""fb_batch_rollout (csrc/fb_rollout.hpp: MuJoCo's rollout for the engine's step, one rollout per ticket on the scratch rows of the
derivative kernel) through the kernel-source emulation build.  No GPU needed.

  * ctrl rollouts against a twin batch driven by set('CTRL') + substep(n) per interval, and action rollouts against a twin stepped by
    fb_batch_step: BIT-EQUAL.  Both sides run the same stage functions in the same order on the same inputs; a difference is a bug in
    what the ticket copies or recomputes, not rounding;
  * row reuse and determinism, the skipped tail, the sources left alone;
  * against the CPU oracle's recipe (tests/rollout_reference.py) at the project's standing parity bound, 1e-6 relative
    (tests/test_gpu_parity.py's contract and measure);
  * argument validation and the array API.

Measured on the emulation build (T = 5 intervals of 10 substeps, mid-range random ctrl; largest relative error over the intervals):
    walk_imitation, four frames:  qpos 7.0e-13  qvel 1.3e-11  sensordata 6.9e-12   (the largest: the frames in contact, nefc up to 15)
    flight_imitation:             qpos 1.0e-15  qvel 2.0e-14  sensordata 4.1e-12
    walk_on_ball:                 qpos 1.3e-14  qvel 2.9e-13  sensordata 3.2e-17   (nefc 12 .. 25)
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, random_state

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fd_reference as fr  # noqa: E402
import rollout_reference as rr  # noqa: E402
from test_deriv_emulation import _load, _other_task_state, mid_ctrl, set_frames, settle  # noqa: E402

PARITY = 1e-6                     # the project's standing bound on qpos / qvel / sensordata against the oracle (tests/test_gpu_parity.py)
STATE_FIELDS = ('QPOS', 'QVEL', 'ACT', 'QACC', 'WARN_EVER', 'SIZE_STATS')       # (QACC is the next solve's warm start)


@pytest.fixture(scope='module')
def emu_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    return g.build_emu()


def walk_frames(om, a):
    """Four walking frames (qpos, qvel, act, ctrl) as in tests/test_gpu_deriv.py: two in the air (one with a strongly rotated root), two
    settled on the floor."""
    rng = np.random.default_rng(21)
    frames = []
    q, v = random_state(a, np.random.default_rng(0), spread=0.0, z=2.0)
    frames.append((q, v, rng.uniform(-0.1, 0.1, 59), mid_ctrl(a, rng)))
    q, v = random_state(a, np.random.default_rng(1), spread=0.1, z=2.0)
    quat = np.array([0.3, -0.6, 0.5, 0.55]); q[3:7] = quat/np.linalg.norm(quat)
    frames.append((q, v, rng.uniform(-0.1, 0.1, 59), mid_ctrl(a, rng)))
    for seed in (3, 8):
        q, v = random_state(a, np.random.default_rng(seed), spread=0.05, z=0.13, vel=0.0)
        ctrl = mid_ctrl(a, rng, 0.45, 0.55)
        frames.append(settle(om, a, q, v, ctrl) + (ctrl,))
    return frames


def ctrl_rows(a, n, T, seed):
    """Mid-range random controls [n, T, nu], a different row for every (r, t)."""
    rng = np.random.default_rng(seed)
    return np.array([[mid_ctrl(a, rng) for _ in range(T)] for _ in range(n)])


def twin_ctrl_loop(twin, ctrl, n_substeps, fields=('QPOS', 'QVEL', 'ACT', 'SENSORDATA'), sync=lambda: None):
    """The loop a rollout replaces, on a batch of its own: per interval set('CTRL'), substep(n), get.  [{field: array}] per interval."""
    out = []
    for t in range(ctrl.shape[1]):
        twin.set('CTRL', ctrl[:, t]); twin.substep(n_substeps); sync()
        out.append({f: twin.get(f) for f in fields})
    return out


def assert_equals_twin(res, rec, na, to_np=lambda t: t.numpy()):
    """Rollout result [n, T, ..] against the twin's records, to the bit."""
    for t, r in enumerate(rec):
        assert np.array_equal(to_np(res.qpos)[:, t], r['QPOS']), ('qpos', t)
        assert np.array_equal(to_np(res.qvel)[:, t], r['QVEL']), ('qvel', t)
        if na:
            assert np.array_equal(to_np(res.act)[:, t], r['ACT']), ('act', t)
        if res.sensordata is not None and 'SENSORDATA' in r:
            assert np.array_equal(to_np(res.sensordata)[:, t], r['SENSORDATA']), ('sensordata', t)


@pytest.fixture(scope='module')
def walk(emu_lib):
    from flybody_amd import engine
    model, om, a = _load('walk_imitation', emu_lib)
    frames = walk_frames(om, a)
    F = [fr.Frame(om, a, *f) for f in frames]
    for f in F:
        f.nominal()
    nefc0 = [f.nefc[0] for f in F]
    assert nefc0[0] == 0 and nefc0[2] > 0 and nefc0[3] > 0, nefc0             # (the rotated frame in the air sits on a joint limit: one row)
    batch = engine.Batch(model, 4, precision=64)
    set_frames(batch, frames)
    return dict(model=model, om=om, a=a, frames=frames, F=F, batch=batch)


# ------------------------------------------------------------------ 1, 4, 5: the twin loop, the skipped tail, the sources
def test_ctrl_rollout_has_the_bits_of_the_twin_loop_and_leaves_the_sources_alone(walk):
    import torch
    from flybody_amd import engine
    a = walk['a']
    batch, twin = engine.Batch(walk['model'], 4, precision=64), engine.Batch(walk['model'], 4, precision=64)      # (the batch moves below: not the fixture's)
    set_frames(batch, walk['frames']); set_frames(twin, walk['frames'])
    ctrl = ctrl_rows(a, 4, 3, seed=7)
    before = {f: batch.get(f) for f in STATE_FIELDS + ('CTRL', 'WARN', 'STEP_TICKS')}
    res = batch.rollout(ctrl=torch.from_numpy(ctrl), n_substeps=2, sensors=True)
    assert batch.rollouts_run() == 4 and res.status.tolist() == [0, 0, 0, 0]
    assert res.state.shape == (4, 3, 109 + 108 + 59) and res.sensordata.shape == (4, 3, 33)
    for f, x in before.items():
        assert np.array_equal(x, batch.get(f)), f
    rec = twin_ctrl_loop(twin, ctrl, 2, fields=('QPOS', 'QVEL', 'ACT', 'SENSORDATA') + STATE_FIELDS)
    assert_equals_twin(res, rec, 59)
    # the skipped tail: without the sensors the stages behind the last integration do not run, and the state has the same bits
    bare = batch.rollout(ctrl=torch.from_numpy(ctrl), n_substeps=2)
    assert bare.sensordata is None and np.array_equal(bare.state.numpy(), res.state.numpy())
    # the sources: the same intervals on the batch itself are those of the twin, which never ran a rollout
    mine = twin_ctrl_loop(batch, ctrl, 2, fields=STATE_FIELDS)
    for t in range(3):
        for f in STATE_FIELDS:
            assert np.array_equal(mine[t][f], rec[t][f]), (t, f)


# ------------------------------------------------------------------ 2, 4: fb_batch_step, the pattern generator in the scratch row
def make_task_batch(name, emu_lib, n_env, reference_traj):
    from flybody_amd import engine
    model = engine.Model.from_asset(name, lib_path=emu_lib)
    b = engine.Batch(model, n_env, precision=64)
    if name == 'flight_imitation':
        from flybody_amd.reference import constant_speed_trajectory
        from flybody_amd.wbpg import build_tables
        b.set_wbpg(build_tables(), seed=0)
        qp, qv = constant_speed_trajectory(200, 20.0, init_pos=(0, 0, 1), body_rot_angle_y=-47.5, control_timestep=2e-4)
        b.set_reference(qp, qv, future_steps=5, terminal_com_dist=2.0, time_limit=0.6)
    else:
        b.set_reference(*reference_traj, terminal_com_dist=float('inf'))
    b.reset()
    return model, b


@pytest.mark.parametrize('name', ['walk_imitation', 'flight_imitation'])
def test_action_rollout_has_the_bits_of_control_steps(emu_lib, reference_traj, name):
    import torch
    model, batch = make_task_batch(name, emu_lib, 8, reference_traj)
    _, twin = make_task_batch(name, emu_lib, 8, reference_traj)
    nact, na = model.dim('nact'), model.dim('na')
    assert (name == 'flight_imitation') == (nact == model.dim('nu') + 1)
    rng = np.random.default_rng(4)
    acts = (0.1*rng.normal(size=(10, 8, nact))).astype(np.float32)
    for k in range(3):
        batch.step_ptr(acts[k].ctypes.data); twin.step_ptr(acts[k].ctypes.data)
    rows = np.ascontiguousarray(acts[3:7].transpose(1, 0, 2))                 # [8, 4, nact]
    res = batch.rollout(action=torch.from_numpy(rows))
    assert batch.rollouts_run() == 8 and not res.status.numpy().any()
    for t in range(4):
        twin.step_ptr(acts[3 + t].ctypes.data)
        assert (twin.get('STEP_TYPE') != 2).all()                            # precondition: no episode of the twin ends on the way
        assert np.array_equal(res.qpos.numpy()[:, t], twin.get('QPOS')) and np.array_equal(res.qvel.numpy()[:, t], twin.get('QVEL')), t
        assert not na or np.array_equal(res.act.numpy()[:, t], twin.get('ACT')), t
    # the sources: the batch takes the same four steps and three more, like the twin that never ran a rollout
    for k in range(3, 7):
        batch.step_ptr(acts[k].ctypes.data)
    for k in range(7, 10):
        batch.step_ptr(acts[k].ctypes.data); twin.step_ptr(acts[k].ctypes.data)
        for f in STATE_FIELDS + ('OBS', 'WARN', 'STEP_TICKS'):
            assert np.array_equal(batch.get(f), twin.get(f)), (k, f)


# ------------------------------------------------------------------ 3: row reuse, determinism
def test_results_do_not_depend_on_the_pool_or_the_call(walk):
    import torch
    batch, a = walk['batch'], walk['a']
    ids = [0, 2, 2, 1, 0]
    ctrl = ctrl_rows(a, 5, 3, seed=9)
    ctrl[2] = ctrl[1]                                   # rollouts 1 and 2: environment 2 with the same inputs; 0 and 4: environment 0 with different ones
    u = torch.from_numpy(ctrl)
    full = batch.rollout(ctrl=u, env_ids=ids, n_substeps=2, sensors=True)
    assert batch.rollouts_run() == 5
    x, s = full.state.numpy(), full.sensordata.numpy()
    assert np.array_equal(x[1], x[2]) and np.array_equal(s[1], s[2])
    assert not np.array_equal(x[0], x[4]) and not np.array_equal(x[0, 0], x[4, 0])
    for pool in (1, 3, 0):
        other = batch.rollout(ctrl=u, env_ids=ids, n_substeps=2, sensors=True, pool_rows=pool)
        assert batch.rollouts_run() == 5
        assert np.array_equal(x, other.state.numpy()) and np.array_equal(s, other.sensordata.numpy()), pool
        assert other.status.tolist() == [0]*5


# ------------------------------------------------------------------ 6: the CPU oracle
def check_against_oracle(tag, res, k, om, a, frame, ctrl, n_substeps, to_np=lambda t: t.numpy()):
    nq, nv = len(a['qpos0']), len(a['dof_bodyid'])
    w = fr.Frame(om, a, *frame).w                        # the acceleration of a forward evaluation at the frame: what forward() left as the warm start
    state, sens, nefc = rr.oracle_rollout(om, a, frame[0], frame[1], frame[2], ctrl, n_substeps, w=w)
    got, gs = to_np(res.state)[k], to_np(res.sensordata)[k]
    eq = max(rr.rel_err(got[t, :nq], state[t, :nq]) for t in range(len(ctrl)))
    ev = max(rr.rel_err(got[t, nq:nq + nv], state[t, nq:nq + nv]) for t in range(len(ctrl)))
    es = max(rr.rel_err(gs[t], sens[t]) for t in range(len(ctrl)))
    print(f'{tag}: qpos {eq:.1e}  qvel {ev:.1e}  sensordata {es:.1e}  bound {PARITY:.0e}  nefc {min(nefc)} .. {max(nefc)}')
    assert eq <= PARITY and ev <= PARITY and es <= PARITY, (tag, eq, ev, es)


def test_walking_rollouts_match_the_oracle(walk):
    import torch
    ctrl = ctrl_rows(walk['a'], 4, 5, seed=13)
    res = walk['batch'].rollout(ctrl=torch.from_numpy(ctrl), n_substeps=10, sensors=True)
    assert res.status.tolist() == [0, 0, 0, 0]
    for k in range(4):
        check_against_oracle(f'walk frame {k}', res, k, walk['om'], walk['a'], walk['frames'][k], ctrl[k], 10)


@pytest.mark.parametrize('name', ['flight_imitation', 'walk_on_ball'])
def test_other_tasks_match_the_oracle(emu_lib, name):
    import torch
    from flybody_amd import engine
    model, om, a = _load(name, emu_lib)
    frame = _other_task_state(model, a)
    batch = engine.Batch(model, 1, precision=64)
    set_frames(batch, [frame])
    ctrl = ctrl_rows(a, 1, 5, seed=17)
    res = batch.rollout(ctrl=torch.from_numpy(ctrl), n_substeps=10, sensors=True)
    assert res.status.tolist() == [0]
    check_against_oracle(name, res, 0, om, a, frame, ctrl[0], 10)


# ------------------------------------------------------------------ 7: validation
def test_argument_validation(emu_lib, walk):
    import ctypes as C
    import torch
    from flybody_amd import engine
    model, a = walk['model'], walk['a']
    B = engine.Batch(model, 2, precision=64)
    L = B.L
    u = np.zeros((3, 2, 59)); act = np.zeros((3, 2, 59), np.float32); out = np.zeros(3*2*276)
    U = torch.zeros(2, 2, 59, dtype=torch.float64)

    def raw(b, cfg, ctrl=u.ctypes.data, action=None, state=out.ctypes.data):
        engine._check(L, L.fb_batch_rollout(b, None if cfg is None else C.byref(cfg), ctrl, action, state, None, None, None))

    def cfg(n_roll=1, horizon=2, n_substeps=1, ids=None, pool=0):
        return engine._RolloutConfig(n_roll, horizon, n_substeps, None if ids is None else ids.ctypes.data, pool)
    with pytest.raises(engine.EngineError, match='null batch'):
        raw(None, cfg())
    with pytest.raises(engine.EngineError, match='null config'):
        raw(B.h, None)
    with pytest.raises(engine.EngineError, match='state output is NULL'):
        raw(B.h, cfg(), state=None)
    with pytest.raises(engine.EngineError, match='both ctrl and action'):
        raw(B.h, cfg(), action=act.ctypes.data)
    with pytest.raises(engine.EngineError, match='neither ctrl nor action'):
        raw(B.h, cfg(), ctrl=None)
    with pytest.raises(ValueError, match='exactly one of ctrl and action'):
        B.rollout()
    with pytest.raises(engine.EngineError, match='n_roll must be >= 1'):
        raw(B.h, cfg(n_roll=0))
    with pytest.raises(engine.EngineError, match='horizon must be >= 1'):
        raw(B.h, cfg(horizon=0))
    with pytest.raises(engine.EngineError, match='n_substeps must be >= 0'):
        B.rollout(ctrl=U, n_substeps=-1)
    for ids in ([2, 0], [0, -1], [0, 5]):
        with pytest.raises(engine.EngineError, match='environment id -?\\d+ out of range'):
            B.rollout(ctrl=U, env_ids=ids)
    with pytest.raises(engine.EngineError, match='environment id out of range'):
        raw(B.h, cfg(n_roll=3))
    for pool in (-1, 9, 1 << 20):
        with pytest.raises(engine.EngineError, match='pool_rows out of range'):
            B.rollout(ctrl=U, pool_rows=pool)
    with pytest.raises(engine.EngineError, match='FP64 batch'):
        engine.Batch(model, 2, precision=32).rollout(ctrl=U)
    a2 = dict(a); a2['body_mass'] = np.asarray(a['body_mass'])*1.1
    with pytest.raises(engine.EngineError, match='group of 2 models'):
        engine.Batch(engine.ModelGroup([a, a2], lib_path=emu_lib), 2, precision=64).rollout(ctrl=U)
    Bl = engine.Batch(model, 2, precision=64)
    Bl.set_control_law(bias=np.zeros(108))
    with pytest.raises(engine.EngineError, match='knows no control law'):
        Bl.rollout(ctrl=U)
    Bl.clear_control_law()
    Bf = engine.Batch(model, 2, precision=64)
    Bf.set('QFRC_APPLIED', np.zeros((2, 108)))
    with pytest.raises(engine.EngineError, match='knows no applied forces'):
        Bf.rollout(ctrl=U)
    Bf.clear_forces()
    fl = engine.Batch(engine.Model.from_asset('flight_imitation', lib_path=emu_lib), 1, precision=64)
    with pytest.raises(engine.EngineError, match='needs fb_batch_set_wbpg first'):
        fl.rollout(action=torch.zeros(1, 1, fl.model.dim('nact')))
    # the Python shim's own checks: dtype, shape, contiguity, the number of environments listed
    for bad in (U.float(), U[:, :, :58], U.transpose(0, 1), np.zeros((2, 2, 59))):
        with pytest.raises(ValueError, match='ctrl must be a contiguous'):
            B.rollout(ctrl=bad)
    with pytest.raises(ValueError, match='env_ids names 1 environments for 2 rollouts'):
        B.rollout(ctrl=U, env_ids=[0])
    # repeats are allowed, more rollouts than environments with env_ids, and n_substeps = 0 is the model's own count
    B.forward()
    r = B.rollout(ctrl=torch.zeros(3, 1, 59, dtype=torch.float64), env_ids=[1, 1, 1])
    ten = B.rollout(ctrl=torch.zeros(1, 1, 59, dtype=torch.float64), env_ids=[1], n_substeps=model.dim('nsubstep'))
    assert B.rollouts_run() == 1 and r.state.shape == (3, 1, 276) and np.array_equal(r.state.numpy()[2], ten.state.numpy()[0])


# ------------------------------------------------------------------ 8: the array API
def test_array_api(emu_lib):
    from flybody_amd import rollout
    model, om, a = _load('walk_on_ball', emu_lib)
    q, v, act, _ = _other_task_state(model, a)
    ctrl = ctrl_rows(a, 6, 2, seed=3)
    many = rollout.rollout(model, q, v, act, ctrl, n_substeps=2, sensors=True, batch_size=4)
    nq, nv, na = (model.dim(k) for k in ('nq', 'nv', 'na'))
    assert many.state.shape == (6, 2, nq + nv + na) and many.qpos.shape == (6, 2, nq) and many.qvel.shape == (6, 2, nv)
    assert many.act.shape == (6, 2, na) and many.sensordata.shape == (6, 2, 33) and many.status.tolist() == [0]*6
    for k in range(6):
        one = rollout.rollout(model, q, v, act, ctrl[k], n_substeps=2, sensors=True)
        assert one.state.shape == (2, nq + nv + na) and one.sensordata.shape == (2, 33) and one.status == 0
        assert np.array_equal(one.state, many.state[k]) and np.array_equal(one.sensordata, many.sensordata[k]), k
    assert not np.array_equal(many.state[0], many.state[1])
    # n states against n sequences
    pairs = rollout.rollout(model, np.array([q, q]), np.array([v, 0.5*v]), np.array([act, act]), ctrl[:2], n_substeps=2, batch_size=1)
    assert pairs.sensordata is None and np.array_equal(pairs.state[0], many.state[0]) and not np.array_equal(pairs.state[1], many.state[1])
    with pytest.raises(ValueError):
        rollout.rollout(model, q, v[:-1], act, ctrl)
    with pytest.raises(ValueError):
        rollout.rollout(model, np.array([q, q, q]), np.array([v, v, v]), None, ctrl[:2])
