"""fb_batch_rollout_feedback (csrc/fb_rollout.hpp: k_closedloop_rollout) on the MI355X, on both engine builds: the assertions
of tests/feedback_cases.py that tests/test_rollout_feedback_emulation.py runs on the emulation build, and on the device alone the
first-order consistency with fb_batch_transition_fd and BatchedFlyEnv.rollout(feedback=...).

Measured on the MI355X (both builds print the same figures): inputs against the formula in numpy, largest vector: dense gains 1.8e-15,
indexing 1.7e-15, quaternion columns 1.5e-16 (the feedback term alone 5.6e-16); first order, K = 0 against A delta / closed loop against
(A + B K) delta: hinge angle 2.5e-6 / 2.5e-6, hinge velocity 2.7e-9 / 2.7e-9, root rotation 2.7e-7 / 2.7e-7, activation 5.0e-11 / 3.0e-10."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feedback_cases as fc  # noqa: E402
from test_gpu_rollout import assert_a_side_stream_call_has_the_bits, np_, set_frames, sync, walk_batch, walk_model, walk_ref  # noqa: E402,F401  (fixtures: the four walking frames, both builds)

pytestmark = pytest.mark.gpu


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.fixture(scope='module')
def ctx(walk_ref, walk_model):  # noqa: F811
    from flybody_amd import engine

    def make_batch():
        b = engine.Batch(walk_model, 4, precision=64)
        set_frames(b, walk_ref['frames'])
        return b
    c = fc.Ctx(walk_ref['a'], walk_ref['frames'], make_batch, dev=dev, np_=np_, sync=sync)
    c.model, c.batch = walk_model, make_batch()
    c.tag = 'MI355X, ' + ('dense' if walk_model.L is not engine.load_library() else 'default') + ' build'
    return c


def test_degenerate_cases_are_the_open_loop_bits(ctx):
    fc.degenerate_cases_are_the_open_loop_bits(ctx, ctx.batch)


def test_closed_loop_is_open_loop_on_its_own_inputs_and_the_inputs_are_the_formula(ctx):
    fc.closed_loop_is_open_loop_on_its_own_inputs_and_the_inputs_are_the_formula(ctx, ctx.batch, ctx.tag)


def test_exact_inputs_give_exact_bits(ctx):
    fc.exact_inputs_give_exact_bits(ctx, ctx.batch)


def test_time_and_nominal_indexing(ctx):
    fc.time_and_nominal_indexing(ctx, ctx.batch, ctx.tag)


def test_quaternion_columns_are_live(ctx):
    fc.quaternion_columns_are_live(ctx, ctx.batch, ctx.tag)


def test_rows_and_calls(ctx):
    fc.rows_and_calls(ctx, ctx.batch)


def test_sources_are_untouched(ctx):
    fc.sources_are_untouched(ctx)


def test_refusals(ctx):
    from flybody_amd import engine
    fc.refusals(ctx, ctx.model, lib_path=None if ctx.model.L is engine.load_library() else engine.HIP_LIB_DENSE)


def test_a_side_stream_orders_the_outputs_behind_the_call(walk_ref):  # noqa: F811
    """stream=: state, ctrl, sensordata and status -- and the transposed gains the kernel streams -- are made in the order of the call's
    stream.  The four walking frames, T = 3 intervals of two substeps, dense gains of scale 1e-2, the default build.
    Measured on the MI355X: the call 1.3 ms, the filler 116 ms."""
    from flybody_amd import engine
    batch = walk_batch(engine.Model(walk_ref['a']), walk_ref)
    c = fc.Ctx(walk_ref['a'], walk_ref['frames'], None, dev=dev, np_=np_, sync=sync)
    K, k = fc.dense_gains(c, 4, seed=122, scale=1e-2)
    args = [dev(x) for x in fc.nominals(c, [0, 1, 2, 3], seed=121) + (K, k)]
    assert_a_side_stream_call_has_the_bits(lambda s: batch.rollout_feedback(*args, n_substeps=2, sensors=True, stream=s),
                                           ('state', 'ctrl', 'sensordata', 'status'))


# ------------------------------------------------------------------ 9: first order, against fb_batch_transition_fd
def test_first_order_consistency_with_transition_fd(ctx):
    fc.first_order_consistency_with_transition_fd(ctx, ctx.model, set_frames, ctx.tag)


# ------------------------------------------------------------------ 11: live environments, the sample axis
def test_fly_env_rollout_with_a_sample_axis_equals_the_flat_call():
    import torch
    from flybody_amd import engine, fly_envs
    env = fly_envs.BatchedFlyEnv(8, terminal_com_dist=float('inf'))
    env.reset_all()
    nact = env.model.dim('nact')
    g = torch.Generator(device='cuda'); g.manual_seed(4)
    for _ in range(3):
        env.step_tensor(0.1*torch.randn(8, nact, generator=g, device='cuda', dtype=torch.float32))
    sync()
    a = env.model.arrays
    frames = [(q, v, act, None) for q, v, act in zip(env.batch.get('QPOS'), env.batch.get('QVEL'), env.batch.get('ACT'))]
    c = fc.Ctx(a, frames, None, dev=dev, np_=np_, sync=sync)
    ids = [1, 3, 6]
    x_nom, u_nom = fc.nominals(c, ids, seed=111)
    K, k = fc.dense_gains(c, 3, seed=112, scale=0.3)
    alpha = np.array([[1.0, 0.5], [0.25, 1.0], [0.0, 2.0]])
    fb = engine.Feedback(dev(x_nom), dev(u_nom), dev(K), dev(k), dev(alpha))
    res = env.rollout(feedback=fb, env_ids=ids, n_substeps=2, sensors=True)
    assert env.batch.rollouts_run() == 6
    assert res.state.shape == (3, 2, fc.T, c.nx) and res.ctrl.shape == (3, 2, fc.T, c.nu) and res.sensordata.shape == (3, 2, fc.T, 33) and res.status.shape == (3, 2)
    flat = env.batch.rollout_feedback(fb.x_nom, fb.u_nom, fb.K, fb.k, dev(alpha.reshape(-1)), nom_ids=[0, 0, 1, 1, 2, 2], env_ids=[1, 1, 3, 3, 6, 6],
                                      n_substeps=2, sensors=True)
    for name in ('state', 'ctrl', 'sensordata', 'status'):
        assert np.array_equal(np_(getattr(res, name)).reshape(np_(getattr(flat, name)).shape), np_(getattr(flat, name))), name
    assert not np.array_equal(np_(res.ctrl[:, 0]), np_(res.ctrl[:, 1]))
    # without a sample axis: one rollout per listed environment
    one = env.rollout(feedback=engine.Feedback(fb.x_nom, fb.u_nom, fb.K, fb.k, dev(alpha[:, 0].copy())), env_ids=ids, n_substeps=2)
    assert np.array_equal(np_(one.state), np_(res.state[:, 0])) and np.array_equal(np_(one.ctrl), np_(res.ctrl[:, 0]))
    with pytest.raises(ValueError):
        env.rollout(feedback=fb, ctrl=fb.u_nom, env_ids=ids)
