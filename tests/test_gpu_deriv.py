"""fb_batch_transition_fd (csrc/fb_deriv.hpp) on the MI355X, against the finite-difference recipe run on the CPU oracle
(tests/fd_reference.py; the comparison, its two column classes and the rounding floor are those of tests/test_deriv_emulation.py): four
walking frames on both engine builds with the full pool and a pool of 64 rows, the other two tasks, two substeps, live environments
linearised between control steps, and determinism.

Measured on the MI355X (eps = 1e-6; largest column error over the columns the oracle resolves, beside it the largest of the oracle's own
eps-vs-2 eps figures for the same frames; both engine builds and both pool sizes give the same figures):
    four walking frames, centred:  A 2.3e-6 (4.6e-5, the first frame in contact)  B 2.0e-9 (1.4e-9)  C 7.3e-3 (6.3e-3)  D 0
        in the air alone:          A 1.1e-8 (5.3e-8)   B 6.1e-10 (6.9e-10)   C 3.4e-4 (3.0e-4)
    a frame in contact, forward:   A 1.1e-6 (4.3e-3)   B 4.0e-9 (2.8e-9)     C 1.4e-2 (6.2e-3)   D 0
    the same frame, two substeps:  A 8.1e-4 (4.8e-4)   B 1.4e-7 (2.1e-7)
    flight_imitation:              A 2.7e-5 (5.4e-4)   B 9.0e-9 (1.3e-8)         walk_on_ball: A 9.1e-8 (3.9e-8)   B 7.4e-10 (3.5e-10)
    8 live environments:           A 3.9e-6 (8.8e-6)   B 2.4e-10 (6.9e-10)
The gap is of the size of the oracle's own sensitivity to its step, not far below it: at eps = 1e-6 both are what two evaluations of
one transition differ by (rounding, and in contact the last iterations of the constraint solver and the noslip passes) divided by
2 eps; tests/test_deriv_emulation.py says how that was told from a systematic difference.  A frame in contact is the worst case, two
substeps through contact amplify it again.  The bounds are ten times the measured figures, per matrix and group of frames."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fd_reference as fr  # noqa: E402
from test_deriv_emulation import _other_task_state, compare, floors, mid_ctrl, settle  # noqa: E402
from conftest import random_state  # noqa: E402

pytestmark = pytest.mark.gpu

# 10 x the largest column error measured on the MI355X, per matrix (module comment)
TOL = dict(A=2.4e-5, B=2.1e-8, C=7.4e-2, D=0.0)             # four walking frames, centred
TOL_FWD = dict(A=1.2e-5, B=4.1e-8, C=1.5e-1, D=0.0)         # forward differences, a frame in contact
TOL_TWO = dict(A=8.2e-3, B=1.5e-6)                          # two substeps, the same frame
TOL_OTHER = dict(A=2.8e-4, B=9.0e-8)                        # flight_imitation, walk_on_ball
TOL_LIVE = dict(A=3.9e-5, B=2.4e-9)                         # live environments


def _load(name, dense):
    from flybody_amd import engine
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    a = dict(engine.load_npz(os.path.join(engine.ASSETS, name + '.npz')))
    return engine.Model(a, dense=dense), fbo.OracleModel(pack_model(a)), a


def set_frames(batch, frames):
    import torch
    batch.set('QPOS', np.array([f[0] for f in frames])); batch.set('QVEL', np.array([f[1] for f in frames]))
    batch.set('CTRL', np.array([f[3] for f in frames]))
    if batch.model.dim('na'):
        batch.set('ACT', np.array([f[2] for f in frames]))
    batch.forward(torch.cuda.current_stream().cuda_stream); torch.cuda.synchronize()


def np_(t):
    return t.cpu().numpy()


def check(tag, got, k, ref, ref2, fl, names, tol=TOL):
    out = {}
    for m in names:
        gap, sens = compare(np_(getattr(got, m)[k]), ref[m], ref2[m], fl[m])
        print(f'{tag} {m}: gap {gap:.2e}  oracle eps vs 2 eps {sens:.2e}  bound {tol[m]:.1e}')
        out[m] = gap
    for m in names:
        assert out[m] <= tol[m], (tag, m, out[m])


@pytest.fixture(scope='module')
def walk_state():
    """Four walking frames, computed once: two in the air (one with a strongly rotated root), two settled on the floor."""
    from flybody_amd import engine
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    a = dict(engine.load_npz(os.path.join(engine.ASSETS, 'walk_imitation.npz')))
    om = fbo.OracleModel(pack_model(a))
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
    return dict(a=a, om=om, frames=frames)


@pytest.fixture(scope='module')
def walk_ref(walk_state):
    """The four walking frames and the oracle recipe's matrices for them, computed once."""
    a, om, frames = walk_state['a'], walk_state['om'], walk_state['frames']
    F = [fr.Frame(om, a, *f) for f in frames]
    ref = [dict(zip('ABCD', f.matrices(1e-6))) for f in F]
    ref2 = [dict(zip('ABCD', f.matrices(2e-6))) for f in F]
    for f in F:
        assert len(set(f.nefc)) == 1, sorted(set(f.nefc))
    assert F[0].nefc[0] == 0 and F[2].nefc[0] > 0 and F[3].nefc[0] > 0
    fwd = dict(zip('ABCD', F[2].matrices(1e-6, False))), dict(zip('ABCD', F[2].matrices(2e-6, False)))
    two = dict(zip('ABCD', F[2].matrices(1e-6, True, 2))), dict(zip('ABCD', F[2].matrices(2e-6, True, 2)))
    assert len(set(F[2].nefc)) == 1
    return dict(a=a, om=om, frames=frames, F=F, ref=ref, ref2=ref2, fwd=fwd, two=two)


@pytest.fixture(scope='module', params=[False, True], ids=['default', 'dense'])
def walk_batch(request, walk_ref):
    from flybody_amd import engine
    model = engine.Model(walk_ref['a'], dense=request.param)
    batch = engine.Batch(model, 4, precision=64)
    set_frames(batch, walk_ref['frames'])
    return batch


@pytest.mark.parametrize('pool_rows', [0, 64])
def test_four_walking_frames_match_the_oracle_recipe(walk_ref, walk_batch, pool_rows):
    res = walk_batch.transition_fd(sensors=True, pool_rows=pool_rows)
    assert walk_batch.fd_tickets() == 4*(1 + 2*(275 + 59))
    assert np_(res.status).tolist() == [0, 0, 0, 0]
    for k in range(4):
        F = walk_ref['F'][k]
        check(f'walk frame {k} pool {pool_rows}', res, k, walk_ref['ref'][k], walk_ref['ref2'][k], floors(F, 1e-6, True), 'ABCD')
    fwd = walk_batch.transition_fd(env_ids=[2], sensors=True, centered=False, pool_rows=pool_rows)
    check(f'walk frame 2 forward pool {pool_rows}', fwd, 0, *walk_ref['fwd'], floors(walk_ref['F'][2], 1e-6, False), 'ABCD', TOL_FWD)


def test_two_substeps_match_the_oracle_recipe(walk_ref, walk_batch):
    res = walk_batch.transition_fd(env_ids=[2], n_substeps=2)
    check('walk frame 2, two substeps', res, 0, *walk_ref['two'], floors(walk_ref['F'][2], 1e-6, True, 2), 'AB', TOL_TWO)


def test_two_calls_give_the_same_bits_and_a_clean_status(walk_ref, walk_batch):
    x = walk_batch.transition_fd(sensors=True)
    y = walk_batch.transition_fd(sensors=True)
    z = walk_batch.transition_fd(sensors=True, pool_rows=7)
    for m in 'ABCD':
        assert np.array_equal(np_(getattr(x, m)), np_(getattr(y, m))) and np.array_equal(np_(getattr(x, m)), np_(getattr(z, m))), m
    assert not np_(x.status).any()


def test_a_side_stream_orders_the_outputs_behind_the_call(walk_state):
    """stream=: the matrices and status are made in the order of the call's stream.  Two walking frames (one in the air, one
    in contact), B's columns alone, centred, one substep, the default build.  Measured on the MI355X: the call 0.25 ms, the filler
    116 ms."""
    from flybody_amd import engine
    from test_gpu_rollout import assert_a_side_stream_call_has_the_bits
    batch = engine.Batch(engine.Model(walk_state['a']), 2, precision=64)
    set_frames(batch, [walk_state['frames'][k] for k in (0, 2)])
    assert_a_side_stream_call_has_the_bits(lambda s: batch.transition_fd(want_A=False, centered=True, n_substeps=1, stream=s), ('B', 'status'))
    assert batch.fd_tickets() == 2*(1 + 2*59)


@pytest.mark.parametrize('name', ['flight_imitation', 'walk_on_ball'])
def test_other_tasks_match_the_oracle_recipe(name):
    from flybody_amd import engine
    model, om, a = _load(name, False)
    frame = _other_task_state(model, a)
    batch = engine.Batch(model, 1, precision=64)
    set_frames(batch, [frame])
    F = fr.Frame(om, a, *frame)
    ref, ref2 = dict(zip('ABCD', F.matrices(1e-6))), dict(zip('ABCD', F.matrices(2e-6)))
    assert len(set(F.nefc)) == 1
    res = batch.transition_fd()
    assert np_(res.status).tolist() == [0]
    check(name, res, 0, ref, ref2, floors(F, 1e-6, True), 'AB', TOL_OTHER)


@pytest.mark.parametrize('dense', [False, True], ids=['default', 'dense'])
def test_live_environments_are_linearised_and_left_alone(dense):
    """64 environments after 5 random control steps; 8 of them linearised between two steps against the recipe started from their own
    QPOS / QVEL / ACT / CTRL with w = QACC; 3 more control steps are bit-identical to a twin that was never linearised."""
    import torch
    from flybody_amd import fly_envs
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    fields = ('QPOS', 'QVEL', 'ACT', 'QACC', 'OBS', 'WARN', 'SIZE_STATS')

    def make():
        env = fly_envs.BatchedFlyEnv(64, terminal_com_dist=float('inf'), dense=dense)
        env.reset_all()
        return env, torch.empty(64, env.model.dim('nact'), device='cuda')

    def steps(env, act, ks):
        h = torch.cuda.current_stream().cuda_stream
        for k in ks:
            env.batch.random_actions(act.data_ptr(), k, seed=5, dist=1, stream=h)
            env.step_tensor(act)
        torch.cuda.synchronize()
    (env, act), (twin, act2) = make(), make()
    steps(env, act, range(5)); steps(twin, act2, range(5))
    a = env.model.arrays
    om = fbo.OracleModel(pack_model(a))
    Q, V, A_, C_, W = (env.batch.get(f) for f in ('QPOS', 'QVEL', 'ACT', 'CTRL', 'QACC'))
    # the first 8 environments whose perturbed transitions keep the nominal's nefc on the oracle's side
    ids, refs = [], []
    for e in range(64):
        F = fr.Frame(om, a, Q[e], V[e], A_[e], C_[e], w=W[e])
        ref = dict(zip('ABCD', F.matrices(1e-6)))
        if len(set(F.nefc)) != 1:
            continue
        ids.append(e); refs.append((F, ref, dict(zip('ABCD', F.matrices(2e-6)))))
        if len(ids) == 8:
            break
    assert len(ids) == 8, ids
    res = env.linearize(ids)
    torch.cuda.synchronize()
    assert not np_(res.status).any()
    for k, (F, ref, ref2) in enumerate(refs):
        check(f'live environment {ids[k]}', res, k, ref, ref2, floors(F, 1e-6, True), 'AB', TOL_LIVE)
    steps(env, act, range(5, 8)); steps(twin, act2, range(5, 8))
    for f in fields:
        assert np.array_equal(env.batch.get(f), twin.batch.get(f)), f
