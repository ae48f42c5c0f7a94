"""The task layer -- observations, rewards, episode ends (flybody_amd/csrc/fb_task.hpp) -- against an independent FP64 reference
(tests/task_reference.py) at the kernel's own state, in FP64 and FP32, on the emulation build and on the MI355X (default library in both
precisions, the 12-per-CU library in FP64).  tests/task_cases.py has the cases, the runner and the derivation of every bound.

THE TESTS.  test_reference_is_pinned_to_the_reference_project ties the numpy reference to the reference project's own outputs.
test_task_layer_* run every case of task_cases.cases(): the staged ones (after reset, mid-episode, LAST -> FIRST, root at (50, -30), root
quaternion x 1.7, dataset modes, flight with randomize_start_step, all four tasks) and the termination rollouts (terminal_com_dist 0.005 /
0.002, root velocities and height written into reach, short time limits).  test_termination_decisions_* count the decisions that lie within
an FP32 rounding band of their threshold: none in FP64, at most 2 % in FP32 (measured: 0 of 233 on the emulation build and on the MI355X, in
both precisions).  test_cases_reach_every_predicate_task_mode_and_state asserts the coverage on the reference alone.  The sensor accumulator
IS reconstructible (SENSORDATA after every `velocity` stage), so the sensor-mean keys are checked on every staged step, not only on FIRST.

MEASURED, FP32 build, worst relative difference to the reference (asserted: 4 x the emulation figure, task_cases.REWARD_BOUND32 / FACTOR_BOUND32):
                                              emulation    MI355X
  REWARD_FACTORS com / qvel / root2site       4.7e-8 / 4.4e-8 / 4.5e-8    6.5e-8 / 6.4e-8 / 5.3e-8      (one single-precision rounding is 6e-8)
  REWARD_FACTORS joint_quat                   1.25e-5      1.87e-5     acos(2 dt^2 - 1) near 1: 97 distances of ~5e-3 rad, each the arc cosine of
                                                                       1 - 1e-5, where one rounding of the argument is 0.5 % of the distance
  REWARD_FACTORS wings                        1.4e-7       1.4e-7
  REWARD walk_imitation, dataset mode         1.26e-5      1.87e-5
  REWARD flight_imitation (both modes)        4.7e-6       9.6e-6
  REWARD walk_on_ball                         6.4e-7       9.5e-7
  REWARD walk_imitation inference, template   0            0           (the constant 1)
  observation keys, worst measured c of c 2^-24 s (emulation): sensor means 0.34, world_zaxis 1.3, appendages_pos 2.5, ref_displacement 0.6,
  ref_root_quat 2.5 -- against the a-priori 1, 8, 24, 27, 48 that are asserted.

MUTATIONS (emulation builds of mutated sources, outside the repository; a case run = one case at one precision, 36 in all):
  s_site 0.0735 -> 0.074235 (1 %)                         6 runs fail: walk_ds, walk_ds_quat, walk_ds_end in both precisions (REWARD_FACTORS[2])
  ref_root(rv, step + k + 1) in ref_displacement          28 runs fail: every case of walk_imitation and flight_imitation (the observation key)
  world_zaxis from R[3 + lane]                            all 36 fail
  the clock summed and compared in single precision       test_clock_decisions_* fail at the first frame check behind control step 2700

WHAT THE TESTS FOUND, both fixed in csrc/fb_task.hpp.  (1) The episode clock was kept in `real`.  The arithmetic
(test_the_double_clock_and_what_a_single_precision_clock_decided) predicts for the FP32 build: walk_imitation's reward scored against the
previous dataset frame on 2285 of 5020 steps, first at control step 2701, LAST by the time limit at 5001 instead of 5000; flight_imitation
3000 instead of 3001; walk_on_ball 1000 instead of 1001; template_task equal.  Observed on the parent's emulation build: walk_on_ball's FP32
episode ends at control step 1000, the FP64 one at 1001.  The clock is a double at either precision now (field TIME).  A real flight episode
never reaches its 0.6 s: on a reference longer than the limit the trajectory ends it at control step 2994 = 3000 - future_steps - 1
(flight_imitation.py:97-102) with discount 1; the limit itself is reached with TIME set in front of it (test_clock_decisions_*).
Run times on the MI355X, 2 environments, zero actions, a host read per step where the step type is compared: 2710 walk_imitation steps
6.3 s (FP64) / 5.8 s (FP32) -- above 5 s, so test_clock_real_episodes_gpu starts that episode at step 1350 of the double clock --, 1002
walk_on_ball steps 2.3 / 2.2 s, 3002 flight_imitation steps 2.0 / 1.9 s.
(2) DeepMimic's egocentric site vectors were rotated with quat2mat(conj(q) / |q|^2), which is a rotation times 1 / |q|^2: walk_ds_quat found
REWARD_FACTORS[2] at 0.2 % of the reference's with the root quaternion x 1.7 (reward 0.036 against 18.0), in both precisions.
"""
import os
import sys
import time

import numpy as np
import pytest

import task_cases as tc
import task_reference as tr
from conftest import ROOT

STAGED = ('walk', 'walk_far', 'walk_quat', 'walk_ds', 'walk_ds_quat', 'flight', 'flight_far', 'flight_quat', 'flight_ds', 'ball', 'template')
ROLLOUTS = ('walk_early', 'walk_ds_end', 'flight_early', 'flight_end', 'flight_ds_limit', 'ball_limit', 'template_limit')
GPU_BUILDS = [('default', 64), ('default', 32), ('dense', 64)]


@pytest.fixture(scope='module')
def emu_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    return g.build_emu()


_RUNS = {}


def _run(name, lib, precision, on_gpu=False, dense=False):
    """(task, records, layout, figures) of a case; a case runs once per library and precision and is shared by the tests that read it"""
    key = (name, lib, precision, dense)
    if key not in _RUNS:
        from flybody_amd import engine
        case = tc.cases()[name]
        task, recs = tc.run_case(case, lib, precision, on_gpu=on_gpu, dense=dense)
        from flybody_amd.engine import Model
        M = Model(tc.arrays(case.asset), lib_path=lib, dense=dense)
        layout = engine.observation_layout(M, task.future_steps, ball=(task.kind == 'ball'))[0]
        _RUNS[key] = (task, recs, layout)
    return _RUNS[key]


def _check_case(name, lib, precision, on_gpu=False, dense=False):
    task, recs, layout = _run(name, lib, precision, on_gpu, dense)
    figures = {}
    xs = [tc.check_record(task, r, layout, precision, figures) for r in recs]
    for k, v in sorted(figures.items()):
        print('%s FP%d %s: worst relative difference %.3g over %d values' % (name, precision, k, max(v), len(v)))
    return task, recs, xs


# ------------------------------------------------------------------ the reference itself
def test_reference_is_pinned_to_the_reference_project():
    """tests/golden/reference_functions.npz holds what the reference project's own quaternions.py and rewards.py return for random inputs
    (tools/make_reference_goldens.py): the numpy reference of this suite must return the same."""
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'reference_functions.npz'))
    q1, q2, v, p, ang = g['q_in1'], g['q_in2'], g['v_in'], g['p_in'], g['ang_in']
    close = lambda a, b: np.allclose(a, b, rtol=1e-12, atol=1e-13)
    assert close(tr.mult_quat(q1, q2), g['q_mult']) and close(tr.reciprocal_quat(q1), g['q_recip'])
    assert close(tr.rotate_vec_with_quat(v, q1), g['q_rotvec']) and close(tr.get_egocentric_vec(p, v, q1), g['q_egocentric'])
    assert close(tr.get_dquat_local(q1, q2), g['q_dquat_local']) and close(tr.quat_z2vec(v), g['q_z2vec'])
    assert np.allclose(tr.quat_dist_short_arc(q1, q2), g['q_dist_short'], rtol=1e-9, atol=1e-12)
    assert close(tr.axis_angle_to_quat(v, ang), g['q_axis_angle']) and close(tr.joint_orientation_quat(v, ang), g['q_joint_orient'])
    assert close(tr.rotate_vec_with_quat(v, 1.7*q1), g['q_rotvec'])                      # a rotation whatever the quaternion's norm
    nj, ns = (int(x) for x in g['rw_dims'])
    cut = np.cumsum([3, 6 + nj, 3*ns])
    for w, r, f in zip(g['rw_walker'], g['rw_reference'], g['rw_factors']):
        feats = [dict(com=x[:cut[0]], qvel=x[cut[0]:cut[1]], root2site=x[cut[1]:cut[2]].reshape(ns, 3), joint_quat=x[cut[2]:].reshape(-1, 4)) for x in (w, r)]
        assert np.allclose(tr.reward_factors_deep_mimic(*feats)[0], f, rtol=1e-9, atol=1e-300)
    assert g['const_terminal'].tolist() == [tr.TERMINAL_LINVEL, tr.TERMINAL_ANGVEL, tr.TERMINAL_QACC]
    assert tr.tolerance_linear(np.array([0.0, 1.5, -3.0, 4.0]), 3.0).tolist() == [1.0, 0.5, 0.0, 0.0]


# ------------------------------------------------------------------ the epilogue at the kernel's own state
@pytest.mark.parametrize('precision', [64, 32])
@pytest.mark.parametrize('name', STAGED + ROLLOUTS)
def test_task_layer_emulation(emu_lib, name, precision):
    _check_case(name, emu_lib, precision)


@pytest.mark.gpu
@pytest.mark.parametrize('build,precision', GPU_BUILDS)
@pytest.mark.parametrize('name', STAGED + ROLLOUTS)
def test_task_layer_gpu(name, build, precision):
    _check_case(name, None, precision, on_gpu=True, dense=(build == 'dense'))


def _decisions(lib, precision, on_gpu=False, dense=False):
    """(decisions compared, decisions within an FP32 band) over the termination rollouts; every other decision equals the reference's"""
    total = left = 0
    for name in ROLLOUTS:
        task, recs, xs = _check_case(name, lib, precision, on_gpu, dense)
        for r, x in zip(recs, xs):
            if x['outcome'] is None: continue
            total += 1; left += bool(tc.band32(x['outcome'], task))
    return total, left


@pytest.mark.parametrize('precision', [64, 32])
def test_termination_decisions_emulation(emu_lib, precision):
    total, left = _decisions(emu_lib, precision)
    print('FP%d: %d of %d decisions within a rounding band' % (precision, left, total))
    assert total > 200 and left <= (0.02*total if precision == 32 else 0)
    if precision == 64:            # (FP64: nothing may even come near)
        for name in ROLLOUTS:
            task, recs, layout = _run(name, emu_lib, 64)
            assert not any(tc.band32(tc.expected(task, r, layout)['outcome'], task) for r in recs if not r['first'])


@pytest.mark.gpu
@pytest.mark.parametrize('build,precision', GPU_BUILDS)
def test_termination_decisions_gpu(build, precision):
    total, left = _decisions(None, precision, on_gpu=True, dense=(build == 'dense'))
    print('%s FP%d: %d of %d decisions within a rounding band' % (build, precision, left, total))
    assert total > 200 and left <= (0.02*total if precision == 32 else 0)


def test_cases_reach_every_predicate_task_mode_and_state(emu_lib):
    """On the reference alone (evaluated at the states the FP64 emulation run went through): every termination predicate fires at least once
    and stays silent at least once, both discounts occur at LAST, every task and mode is there, and the exceptional states are what their names
    say.  physics_error stays silent throughout: this suite adds no NaN or fault state (tests/test_gpu_parity.py::test_numeric_guards_on_gpu)."""
    fired, silent, last_discounts, kinds = set(), set(), set(), set()
    time_limit_alone = False
    for name in STAGED + ROLLOUTS:
        task, recs, layout = _run(name, emu_lib, 64)
        kinds.add(task.kind)
        types = []
        for r in recs:
            x = tc.expected(task, r, layout); types.append(x['step_type'])
            if x['outcome'] is None: continue
            for p, (hit, _, _) in x['outcome']['predicates'].items():
                (fired if hit else silent).add((task.kind.split('_')[0], p))
            if x['step_type'] == tr.LAST:
                last_discounts.add(x['discount'])
                time_limit_alone |= not x['outcome']['term']
        n = tc.cases()[name].n_env
        seq = np.array(types).reshape(-1, n)
        if name not in ('walk_far', 'walk_quat', 'walk_ds', 'walk_ds_quat', 'flight', 'flight_far', 'flight_quat', 'flight_ds'):
            assert ((seq[:-1] == tr.LAST) & (seq[1:] == tr.FIRST)).any(), name           # LAST, then FIRST through the auto-reset
        assert (seq[0] == tr.FIRST).all() and (seq[1] != tr.FIRST).all()
    want = {('walk', 'linvel'), ('walk', 'angvel'), ('walk', 'traj_end'), ('walk', 'com_dist'), ('flight', 'height'), ('flight', 'com_dist'), ('flight', 'traj_end')}
    assert want <= fired, want - fired
    assert want | {('ball', 'linvel'), ('ball', 'angvel')} | {(k, 'physics_error') for k in ('walk', 'flight', 'ball', 'template')} <= silent
    assert not any(p == 'physics_error' for _, p in fired)
    assert last_discounts == {0.0, 1.0} and time_limit_alone
    assert kinds == {'walk', 'walk_ds', 'flight', 'flight_ds', 'ball', 'template'}
    # the exceptional states
    for name, kind in (('walk_far', 'far'), ('flight_far', 'far'), ('walk_quat', 'quat'), ('flight_quat', 'quat'), ('walk_ds_quat', 'quat')):
        task, recs, _ = _run(name, emu_lib, 64)
        if kind == 'far': assert all(abs(r['st']['qpos'][0] - 50) < 1 and abs(r['st']['qpos'][1] + 30) < 1 for r in recs)
        else:
            norms = [np.linalg.norm(r['st']['qpos'][3:7]) for r in recs if r['k'] in tc.cases()[name].events]
            assert len(norms) >= 3 and np.allclose(norms, 1.7, rtol=1e-6)
    task, recs, _ = _run('flight_ds', emu_lib, 64)
    assert len({task.episode(r['env'], r['episode'])['row0'] for r in recs}) == 3           # randomize_start_step: three different start rows
    task, recs, _ = _run('walk_ds_end', emu_lib, 64)
    assert len({(r['env'], r['episode']) for r in recs}) > 3                               # a new snippet after the first ends


# ------------------------------------------------------------------ the episode clock
def clock(h, n):
    """MuJoCo's and the oracle's clock, d->time += h in double: the time after 0 .. n substeps"""
    t = np.zeros(n + 1)
    for k in range(n): t[k + 1] = t[k] + h
    return t


def clock32(h, n):
    """... and the same sum kept in single precision, as the FP32 build kept it up to and including the parent of this test"""
    t = np.zeros(n + 1, np.float32); h = np.float32(h)
    for k in range(n): t[k + 1] = t[k] + h
    return t


# (timestep, control_timestep, the factory's time limit) -> the control step that is LAST by the time limit
FACTORY = dict(walk_imitation=(2e-4, 2e-3, 10.0, 5000), flight_imitation=(5e-5, 2e-4, 0.6, 3001), walk_on_ball=(2e-4, 2e-3, 2.0, 1001), template_task=(2e-4, 2e-3, 1.0, 501))


def test_the_double_clock_and_what_a_single_precision_clock_decided():
    """The arithmetic alone.  The double clock stands at control step k after k control steps, for every k of every task's longest episode, and
    ends the time-limited episodes at the steps of FACTORY.  The single-precision sum the FP32 build used to keep: walk_imitation one frame
    behind on 2285 of 5020 steps, first at control step 2701 (t = 5.401 s), LAST at 5001 instead of 5000; flight_imitation LAST at 3000
    instead of 3001; walk_on_ball 1000 instead of 1001; template_task equal."""
    before = {}
    for name, (h, dt, limit, last) in FACTORY.items():
        nsub = int(round(dt/h)); n = last + 20
        t = clock(h, n*nsub)[::nsub]
        assert (np.floor(t/dt + 0.5) == np.arange(n + 1)).all(), name
        assert int(np.argmax(t >= limit)) == last, name
        t32 = clock32(h, n*nsub)[::nsub]
        behind = np.floor(t32/np.float32(dt) + np.float32(0.5)).astype(int) != np.arange(n + 1)
        before[name] = (int(np.argmax(t32 >= np.float32(limit))), int(behind.sum()), int(np.argmax(behind)) if behind.any() else None)
    assert before == dict(walk_imitation=(5001, 2285, 2701), flight_imitation=(3000, 0, None), walk_on_ball=(1000, 0, None), template_task=(501, 0, None)), before


def test_oracle_clock_is_the_double_sum(oracle_model, reference_traj):
    from oracle import fbo
    od = fbo.OracleData(oracle_model); od.configure_env(*reference_traj, terminal_com_dist=float('inf')); od.env_reset()
    t = clock(2e-4, 30)
    for k in range(1, 4):
        od.env_step(np.zeros(59)); assert od.scalar('time') == t[10*k]


def _clock_batch(asset, lib, precision, dense, n_frames=None):
    """2 environments under zero actions whose episodes end by the clock alone (terminal_com_dist = inf)"""
    from flybody_amd import engine
    from flybody_amd.wbpg import build_tables
    a = tc.arrays(asset)
    B = engine.Batch(engine.Model(a, lib_path=lib, dense=dense), 2, precision=precision)
    task = None
    if asset == 'walk_imitation':
        ds, jid, sid = tc.clock_dataset(n_frames)
        B.set_walk_dataset(ds, jid, sid, future_steps=2, terminal_com_dist=float('inf'), time_limit=10.0, seed=0)
        r = tc._round32 if precision == 32 else (lambda x: np.asarray(x, float))
        import collections
        dsr = collections.namedtuple('DS', 'n_traj offsets qpos qvel root2site joint_quat')(1, ds.offsets, r(ds.qpos), r(ds.qvel), r(ds.root2site), r(ds.joint_quat))
        task = tr.Task('walk_ds', tc._arrays32(a) if precision == 32 else a, None, None, 2, np.inf, 10.0, ds=dsr, joint_ids=jid, site_ids=sid)
    elif asset == 'flight_imitation':
        B.set_wbpg(build_tables(), seed=5)
        q, v = tc._flight_track(3100 if n_frames is None else n_frames, z=200.0)      # (too high to fall to the terminal height within 0.6 s)
        B.set_reference(q, v, future_steps=5, terminal_com_dist=float('inf'), time_limit=0.6)
    elif asset == 'walk_on_ball':
        B.set_time_limit(2.0)
    return B, task, B.model.dim('nact'), a


def _walk_frames(B, task, dev, steps, k0):
    """Control steps k0 + 1 ... of a walk_imitation dataset episode: per step the frame (k - 1, k or k + 1) whose DeepMimic CoM factor the
    kernel's REWARD_FACTORS[0] is, judged by the reference at the kernel's own state (one frame apart: 0.8 % or more; the bound: FACTOR_BOUND32[0])"""
    a0 = np.zeros((2, 59), np.float32); frames = []
    ep = task.episode(0, 0)
    for k in range(k0 + 1, k0 + 1 + steps):
        dev.step(a0)
        S = tc.read_state(B); f0 = B.get('REWARD_FACTORS')[:, 0]
        row = []
        for e in range(2):
            st = tc.env_state(S, e, int(S['STEP_COUNT'][e, 0]), 0)
            near = {j: tr.reward_factors_deep_mimic(tr.walker_features(task, st), tr.reference_features(task, ep, j))[0][0] for j in (k - 1, k, k + 1)}
            hit = [j for j, f in near.items() if abs(f0[e] - f) <= max(tc.FACTOR_BOUND32[0], 1e-10)*f]
            assert len(hit) == 1, (k, e, f0[e], near)
            row.append(hit[0])
        frames.append(row)
    return np.array(frames)


def _jump(B, asset, k):
    """The clock of every environment set to the double sum after k control steps"""
    h, dt, _, _ = FACTORY[asset]; nsub = int(round(dt/h))
    B.set('TIME', clock(h, k*nsub)[-1])


def _clock_decisions(lib, precision, on_gpu, dense=False):
    """With the clock set in front of each boundary (TIME), FP32 and FP64 builds must decide as the double clock does; TIME itself must hold
    that sum to the bit."""
    # walk_imitation, dataset mode: the frames either side of control step 2701
    B, task, nact, a = _clock_batch('walk_imitation', lib, precision, dense, n_frames=2720)
    dev = tc.Device(B, on_gpu); B.reset(); _jump(B, 'walk_imitation', 2698)
    frames = _walk_frames(B, task, dev, 5, 2698)
    assert frames.tolist() == [[k, k] for k in range(2699, 2704)], frames.tolist()
    assert (B.get('TIME')[:, 0] == clock(2e-4, 27030)[-1]).all() and (B.get('STEP_TYPE') == tr.MID).all()
    # ... and its time limit: LAST at control step 5000 (the trajectory's own end, step 2717, lies behind the jump)
    _jump(B, 'walk_imitation', 4997)
    types = []
    for _ in range(4): dev.step(np.zeros((2, nact), np.float32)); types.append((B.get('STEP_TYPE')[:, 0].tolist(), B.get('DISCOUNT')[:, 0].tolist()))
    assert types == [([1, 1], [1, 1]), ([1, 1], [1, 1]), ([2, 2], [1, 1]), ([0, 0], [1, 1])], types
    # walk_on_ball (2 s) and flight_imitation (0.6 s): LAST at 1001 and 3001
    for asset, last in (('walk_on_ball', 1001), ('flight_imitation', 3001)):
        B, _, nact, _ = _clock_batch(asset, lib, precision, dense, n_frames=40)
        dev = tc.Device(B, on_gpu); B.reset(); _jump(B, asset, last - 3)
        types = []
        for _ in range(4): dev.step(np.zeros((2, nact), np.float32)); types.append((B.get('STEP_TYPE')[:, 0].tolist(), B.get('DISCOUNT')[:, 0].tolist()))
        assert types == [([1, 1], [1, 1]), ([1, 1], [1, 1]), ([2, 2], [1, 1]), ([0, 0], [1, 1])], (asset, types)


@pytest.mark.parametrize('precision', [64, 32])
def test_clock_decisions_emulation(emu_lib, precision):
    _clock_decisions(emu_lib, precision, on_gpu=False)


@pytest.mark.gpu
@pytest.mark.parametrize('build,precision', GPU_BUILDS)
def test_clock_decisions_gpu(build, precision):
    _clock_decisions(None, precision, on_gpu=True, dense=(build == 'dense'))


@pytest.mark.gpu
@pytest.mark.parametrize('precision', [64, 32])
@pytest.mark.parametrize('asset,steps', [('walk_imitation', 2710), ('walk_on_ball', 1002), ('flight_imitation', 3002)])
def test_clock_real_episodes_gpu(asset, steps, precision):
    """The real episodes, from their reset, on the MI355X: STEP_TYPE and DISCOUNT of every step as the double clock decides them, the dataset
    frame through control step 2710 of walk_imitation, the LAST step under the factory time limits of walk_on_ball and flight_imitation
    (a flight episode on a reference of 3100 frames ends at control step 2994 = 3000 - future_steps - 1 with discount 1, the trajectory's
    end as flight_imitation.py:97-102 sets it; its time limit of 0.6 s is reached by test_clock_decisions_* alone)."""
    B, task, nact, a = _clock_batch(asset, None, precision, False, n_frames=2720 if asset == 'walk_imitation' else None)
    dev = tc.Device(B, True); B.reset()
    a0 = np.zeros((2, nact), np.float32); types, disc = [], []
    t0 = time.time()
    if asset == 'walk_imitation':
        # (all 2710 steps from the reset measured 6.3 s in FP64 and 5.8 s in FP32 on the MI355X: the run starts at control step 1350 of the double clock)
        ptr = dev.action(a0); _jump(B, asset, 1350)
        for k in range(1346): B.step_ptr(ptr, dev.st)
        B.synchronize(dev.st)
        assert (B.get('STEP_TYPE') == tr.MID).all() and (B.get('STEP_COUNT') == 1346).all()
        frames = _walk_frames(B, task, dev, 14, 2696)
        print('walk_imitation FP%d: control steps 1351 ... 2710 in %.2f s' % (precision, time.time() - t0))
        assert frames.tolist() == [[k, k] for k in range(2697, 2711)], frames.tolist()
        assert (B.get('TIME')[:, 0] == clock(2e-4, 27100)[-1]).all()
        return
    ptr = dev.action(a0)
    for k in range(steps):
        B.step_ptr(ptr, dev.st); B.synchronize(dev.st)
        types.append(B.get('STEP_TYPE')[:, 0].copy()); disc.append(B.get('DISCOUNT')[:, 0].copy())
    print('%s FP%d: %d control steps in %.2f s' % (asset, precision, steps, time.time() - t0))
    types = np.array(types); disc = np.array(disc)
    last = 1001 if asset == 'walk_on_ball' else 2994
    want = np.ones(steps, int); want[last - 1] = tr.LAST; want[last] = tr.FIRST
    assert (types == want[:, None]).all(), np.argwhere(types != want[:, None])[:4].tolist()
    assert (disc == 1).all()
