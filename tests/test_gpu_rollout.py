"""fb_batch_rollout (csrc/fb_rollout.hpp) on the MI355X: the cases of tests/test_rollout_emulation.py on the device -- ctrl rollouts
bit-equal to a twin's set('CTRL') + substep loop on both engine builds, action rollouts of live BatchedFlyEnv environments bit-equal
to the control steps of a twin, the sources left alone, row reuse and determinism, the CPU oracle's recipe at the project's standing
parity bound (1e-6 relative, tests/test_gpu_parity.py's contract and measure), and the array API.

Measured on the MI355X (T = 5 intervals of 10 substeps, mid-range random ctrl; largest relative error over the intervals; both engine
builds print the same figures):
    walk_imitation, four frames:  qpos 6.1e-13  qvel 8.4e-12  sensordata 4.5e-12   (the largest: the frames in contact, nefc up to 15)
    flight_imitation:             qpos 1.9e-15  qvel 1.7e-14  sensordata 4.4e-12
    walk_on_ball:                 qpos 5.7e-15  qvel 1.5e-13  sensordata 2.1e-17   (nefc 12 .. 25)
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_deriv_emulation import _other_task_state  # noqa: E402
from test_rollout_emulation import (STATE_FIELDS, assert_equals_twin, check_against_oracle, ctrl_rows, twin_ctrl_loop,  # noqa: E402
                                    walk_frames)

pytestmark = pytest.mark.gpu


def np_(t):
    return t.cpu().numpy()


def sync():
    import torch
    torch.cuda.synchronize()


def set_frames(batch, frames):
    import torch
    batch.set('QPOS', np.array([f[0] for f in frames])); batch.set('QVEL', np.array([f[1] for f in frames]))
    batch.set('CTRL', np.array([f[3] for f in frames]))
    if batch.model.dim('na'):
        batch.set('ACT', np.array([f[2] for f in frames]))
    batch.forward(torch.cuda.current_stream().cuda_stream); sync()


def _load(name, dense=False):
    from flybody_amd import engine
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    a = dict(engine.load_npz(os.path.join(engine.ASSETS, name + '.npz')))
    return engine.Model(a, dense=dense), fbo.OracleModel(pack_model(a)), a


@pytest.fixture(scope='module')
def walk_ref():
    """The four walking frames of tests/test_rollout_emulation.py, computed once."""
    _, om, a = _load('walk_imitation')
    return dict(a=a, om=om, frames=walk_frames(om, a))


@pytest.fixture(scope='module', params=[False, True], ids=['default', 'dense'])
def walk_model(request, walk_ref):
    from flybody_amd import engine
    return engine.Model(walk_ref['a'], dense=request.param)


def walk_batch(model, walk_ref):
    from flybody_amd import engine
    batch = engine.Batch(model, 4, precision=64)
    set_frames(batch, walk_ref['frames'])
    return batch


N_FILLER = 128                    # products of the side-stream tests' filler: 116 ms measured on the MI355X, against calls of at most 1.4 ms


def assert_a_side_stream_call_has_the_bits(call, fields, n_filler=N_FILLER):
    """`call(stream)` on the current stream gives the expectation.  Then a chain of n_filler 4096 x 4096 FP32 products is queued on the
    current stream and, while it runs, `call` goes to a fresh stream that does not wait for it (the inputs are complete): every output
    in `fields` has the expectation's bits.  An output that was made in the current stream's order instead is zero-filled there behind
    the filler -- after the kernel wrote it.  Precondition, asserted: the filler is still running when the call's stream has drained.
    Shared by tests/test_gpu_rollout_feedback.py and tests/test_gpu_deriv.py."""
    import torch
    x = torch.full((4096, 4096), 1/4096, device='cuda')
    y = [torch.ones_like(x), torch.empty_like(x)]
    sync()
    want = call(None)
    sync()
    want = {f: np_(getattr(want, f)) for f in fields}
    for i in range(n_filler):
        torch.mm(x, y[i % 2], out=y[(i + 1) % 2])
    s = torch.cuda.Stream()
    got = call(s.cuda_stream)
    s.synchronize()
    outlasted = not torch.cuda.current_stream().query()
    sync()
    assert outlasted, 'the filler ended before the call on the side stream did: the comparison below would show nothing'
    for f in fields:
        assert np.array_equal(np_(getattr(got, f)), want[f]), f


# ------------------------------------------------------------------ 1, 4, 5: the twin loop, the skipped tail, the sources
def test_ctrl_rollout_has_the_bits_of_the_twin_loop_and_leaves_the_sources_alone(walk_ref, walk_model):
    import torch
    batch, twin = walk_batch(walk_model, walk_ref), walk_batch(walk_model, walk_ref)
    ctrl = ctrl_rows(walk_ref['a'], 4, 3, seed=7)
    u = torch.from_numpy(ctrl).cuda()
    before = {f: batch.get(f) for f in STATE_FIELDS + ('CTRL', 'WARN')}
    res = batch.rollout(ctrl=u, n_substeps=2, sensors=True)
    assert batch.rollouts_run() == 4 and np_(res.status).tolist() == [0, 0, 0, 0]
    for f, x in before.items():
        assert np.array_equal(x, batch.get(f)), f
    rec = twin_ctrl_loop(twin, ctrl, 2, fields=('QPOS', 'QVEL', 'ACT', 'SENSORDATA') + STATE_FIELDS, sync=sync)
    assert_equals_twin(res, rec, 59, np_)
    bare = batch.rollout(ctrl=u, n_substeps=2)
    assert bare.sensordata is None and np.array_equal(np_(bare.state), np_(res.state))
    mine = twin_ctrl_loop(batch, ctrl, 2, fields=STATE_FIELDS, sync=sync)
    for t in range(3):
        for f in STATE_FIELDS:
            assert np.array_equal(mine[t][f], rec[t][f]), (t, f)


def test_a_side_stream_orders_the_outputs_behind_the_call(walk_ref):
    """stream=: state, sensordata and status are made in the order of the call's stream.  Four walking frames, ctrl
    [4, 3, nu], two substeps, the default build.  Measured on the MI355X: the call 1.2 ms, the filler 116 ms."""
    import torch
    from flybody_amd import engine
    batch = walk_batch(engine.Model(walk_ref['a']), walk_ref)
    u = torch.from_numpy(ctrl_rows(walk_ref['a'], 4, 3, seed=7)).cuda()
    assert_a_side_stream_call_has_the_bits(lambda s: batch.rollout(ctrl=u, n_substeps=2, sensors=True, stream=s),
                                           ('state', 'sensordata', 'status'))


# ------------------------------------------------------------------ 2, 4: live environments, actions through the task's hook
@pytest.mark.parametrize('name', ['walk_imitation', 'flight_imitation'])
def test_action_rollout_of_live_environments_has_the_bits_of_their_steps(name):
    """8 environments and a twin after 3 warm-up steps; K = 2 action sequences per environment ([8, 2, 4, nact]: the sample axis), the
    first of them then stepped on the twin; the environments take the same steps and three more, bit-identical to the twin's."""
    import torch
    from flybody_amd import fly_envs

    def make():
        env = fly_envs.flight_imitation(n_env=8) if name == 'flight_imitation' else fly_envs.BatchedFlyEnv(8, terminal_com_dist=float('inf'))
        env.reset_all()
        return env
    env, twin = make(), make()
    nact, na = env.model.dim('nact'), env.model.dim('na')
    g = torch.Generator(device='cuda'); g.manual_seed(4)
    acts = 0.1*torch.randn(10, 8, nact, generator=g, device='cuda', dtype=torch.float32)
    for k in range(3):
        env.step_tensor(acts[k].contiguous()); twin.step_tensor(acts[k].contiguous())
    rows = torch.stack([acts[3:7].transpose(0, 1), -acts[3:7].transpose(0, 1)], dim=1).contiguous()        # [8, 2, 4, nact]
    res = env.rollout(action=rows, sensors=True)
    assert env.batch.rollouts_run() == 16 and not np_(res.status).any()
    assert res.state.shape[:3] == (8, 2, 4) and res.sensordata.shape == (8, 2, 4, 33) and res.status.shape == (8, 2)
    assert not np.array_equal(np_(res.state[:, 0]), np_(res.state[:, 1]))
    for t in range(4):
        twin.step_tensor(acts[3 + t].contiguous()); sync()
        assert (twin.batch.get('STEP_TYPE') != 2).all()                      # precondition: no episode of the twin ends on the way
        assert np.array_equal(np_(res.qpos[:, 0, t]), twin.batch.get('QPOS')) and np.array_equal(np_(res.qvel[:, 0, t]), twin.batch.get('QVEL')), t
        assert not na or np.array_equal(np_(res.act[:, 0, t]), twin.batch.get('ACT')), t
    for k in range(3, 7):
        env.step_tensor(acts[k].contiguous())
    for k in range(7, 10):
        env.step_tensor(acts[k].contiguous()); twin.step_tensor(acts[k].contiguous()); sync()
        for f in STATE_FIELDS + ('OBS', 'WARN'):
            assert np.array_equal(env.batch.get(f), twin.batch.get(f)), (k, f)


# ------------------------------------------------------------------ 3: row reuse, determinism
def test_results_do_not_depend_on_the_pool_or_the_call(walk_ref, walk_model):
    import torch
    batch = walk_batch(walk_model, walk_ref)
    ids = [0, 2, 2, 1, 0]
    ctrl = ctrl_rows(walk_ref['a'], 5, 3, seed=9)
    ctrl[2] = ctrl[1]
    u = torch.from_numpy(ctrl).cuda()
    full = batch.rollout(ctrl=u, env_ids=ids, n_substeps=2, sensors=True)
    assert batch.rollouts_run() == 5
    x, s = np_(full.state), np_(full.sensordata)
    assert np.array_equal(x[1], x[2]) and np.array_equal(s[1], s[2])
    assert not np.array_equal(x[0], x[4]) and not np.array_equal(x[0, 0], x[4, 0])
    for pool in (1, 3, 0):
        other = batch.rollout(ctrl=u, env_ids=ids, n_substeps=2, sensors=True, pool_rows=pool)
        assert batch.rollouts_run() == 5
        assert np.array_equal(x, np_(other.state)) and np.array_equal(s, np_(other.sensordata)), pool
        assert np_(other.status).tolist() == [0]*5


# ------------------------------------------------------------------ 6: the CPU oracle
def test_walking_rollouts_match_the_oracle(walk_ref, walk_model):
    import torch
    batch = walk_batch(walk_model, walk_ref)
    ctrl = ctrl_rows(walk_ref['a'], 4, 5, seed=13)
    res = batch.rollout(ctrl=torch.from_numpy(ctrl).cuda(), n_substeps=10, sensors=True)
    assert np_(res.status).tolist() == [0, 0, 0, 0]
    for k in range(4):
        check_against_oracle(f'walk frame {k}', res, k, walk_ref['om'], walk_ref['a'], walk_ref['frames'][k], ctrl[k], 10, np_)


@pytest.mark.parametrize('name', ['flight_imitation', 'walk_on_ball'])
def test_other_tasks_match_the_oracle(name):
    import torch
    from flybody_amd import engine
    model, om, a = _load(name)
    frame = _other_task_state(model, a)
    batch = engine.Batch(model, 1, precision=64)
    set_frames(batch, [frame])
    ctrl = ctrl_rows(a, 1, 5, seed=17)
    res = batch.rollout(ctrl=torch.from_numpy(ctrl).cuda(), n_substeps=10, sensors=True)
    assert np_(res.status).tolist() == [0]
    check_against_oracle(name, res, 0, om, a, frame, ctrl[0], 10, np_)


# ------------------------------------------------------------------ 8: the array API
def test_array_api():
    from flybody_amd import rollout
    model, om, a = _load('walk_on_ball')
    q, v, act, _ = _other_task_state(model, a)
    nq, nv, na = (model.dim(k) for k in ('nq', 'nv', 'na'))
    ctrl = ctrl_rows(a, 6, 2, seed=3)
    many = rollout.rollout(model, q, v, act, ctrl, n_substeps=2, sensors=True, batch_size=4)
    assert many.state.shape == (6, 2, nq + nv + na) and many.qpos.shape == (6, 2, nq) and many.qvel.shape == (6, 2, nv)
    assert many.act.shape == (6, 2, na) and many.sensordata.shape == (6, 2, 33) and many.status.tolist() == [0]*6
    for k in range(6):
        one = rollout.rollout(model, q, v, act, ctrl[k], n_substeps=2, sensors=True)
        assert one.state.shape == (2, nq + nv + na) and one.sensordata.shape == (2, 33) and one.status == 0
        assert np.array_equal(one.state, many.state[k]) and np.array_equal(one.sensordata, many.sensordata[k]), k
    assert not np.array_equal(many.state[0], many.state[1])
