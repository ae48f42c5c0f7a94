"""fb_batch_rollout_feedback (csrc/fb_rollout.hpp: k_closedloop_rollout, closed-loop rollouts under a time-varying affine feedback on ctrl;
DESIGN.md 21) through the kernel-source emulation build.  No GPU needed.  The assertions are those of tests/feedback_cases.py, which
tests/test_gpu_rollout_feedback.py runs on the MI355X:

  * K = k = 0, K and k NULL, alpha = 0: the bits of fb_batch_rollout(ctrl = u_nom);
  * the recorded inputs through the open-loop kernel reproduce state and sensordata BIT FOR BIT (gains scaled so that some inputs
    saturate ctrlrange and most do not, frames in contact included);
  * the recorded inputs against the formula in numpy FP64 (lqr.state_difference, act_ctrlrange) at the project's standing bound, 1e-6
    relative per vector (tests/test_gpu_parity.py's contract and measure); with exact products, bit for bit;
  * time and nominal indexing, the quaternion columns, rows and calls, the sources left alone, the refusals, the array API.

Measured on the emulation build (inputs against the formula, largest vector): dense gains 2.3e-15, indexing 1.6e-15, quaternion
columns 9.7e-17 (the feedback term alone: 5.6e-16), walk_on_ball's ball joint 1.9e-16."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feedback_cases as fc  # noqa: E402
from test_deriv_emulation import _load, _other_task_state, set_frames  # noqa: E402
from test_rollout_emulation import emu_lib, walk_frames  # noqa: E402,F401  (the emulation library's fixture)


@pytest.fixture(scope='module')
def ctx(emu_lib):  # noqa: F811
    import torch
    from flybody_amd import engine
    model, om, a = _load('walk_imitation', emu_lib)
    frames = walk_frames(om, a)

    def make_batch():
        b = engine.Batch(model, 4, precision=64)
        set_frames(b, frames)
        return b
    c = fc.Ctx(a, frames, make_batch, dev=lambda x: torch.from_numpy(np.ascontiguousarray(x)), np_=lambda t: t.numpy())
    c.model, c.batch = model, make_batch()
    return c


def test_degenerate_cases_are_the_open_loop_bits(ctx):
    fc.degenerate_cases_are_the_open_loop_bits(ctx, ctx.batch)


def test_closed_loop_is_open_loop_on_its_own_inputs_and_the_inputs_are_the_formula(ctx):
    fc.closed_loop_is_open_loop_on_its_own_inputs_and_the_inputs_are_the_formula(ctx, ctx.batch, 'emulation')


def test_exact_inputs_give_exact_bits(ctx):
    fc.exact_inputs_give_exact_bits(ctx, ctx.batch)


def test_time_and_nominal_indexing(ctx):
    fc.time_and_nominal_indexing(ctx, ctx.batch, 'emulation')


def test_quaternion_columns_are_live(ctx):
    fc.quaternion_columns_are_live(ctx, ctx.batch, 'emulation')


def test_rows_and_calls(ctx):
    fc.rows_and_calls(ctx, ctx.batch)


def test_sources_are_untouched(ctx):
    fc.sources_are_untouched(ctx)


def test_refusals(ctx, emu_lib):  # noqa: F811
    fc.refusals(ctx, ctx.model, lib_path=emu_lib)


def test_ball_joint_columns(emu_lib):  # noqa: F811
    """walk_on_ball: a ball joint and no free joint -- its three columns go through the quaternion difference too."""
    import torch
    from flybody_amd import derivatives, engine, lqr
    model, om, a = _load('walk_on_ball', emu_lib)
    frame = _other_task_state(model, a)
    batch = engine.Batch(model, 1, precision=64)
    set_frames(batch, [frame])
    c = fc.Ctx(a, [frame], None, dev=lambda x: torch.from_numpy(np.ascontiguousarray(x)), np_=lambda t: t.numpy())
    j = list(a['jnt_type']).index(1); d = int(a['jnt_dofadr'][j])
    rng = np.random.default_rng(3)
    x_nom = np.repeat(c.x0[:, None], fc.T, axis=1)
    for t in range(fc.T):
        dq = np.zeros(c.nv); dq[d:d + 3] = rng.uniform(-0.4, 0.4, 3)
        x_nom[0, t, :c.nq] = derivatives.integrate_pos(c.shim, c.x0[0, :c.nq], dq)
    _, u_nom = fc.nominals(c, [0], seed=5)
    K = np.zeros((1, fc.T, c.nu, c.ndx))
    w = c.hi - c.lo
    for i in range(3):
        K[:, :, i, d + i] = 0.5*2.0**np.floor(np.log2(w[i]))
    res = fc.run(c, batch, x_nom, u_nom, K, n_substeps=1)
    u = res.ctrl.numpy()
    ref = fc.formula(c, res.state.numpy(), [0], [0], x_nom, u_nom, K, None, None)
    assert (np.abs(u[0, 0, :3] - u_nom[0, 0, :3]) > 0.01*w[:3]).all()
    assert np.abs(lqr.state_difference(c.shim, c.x0[0], x_nom[0, 0])[d:d + 3]).min() > 0
    err = max(fc.rel_err(u[0, t], ref[0, t]) for t in range(fc.T))
    print(f'walk_on_ball: inputs against the formula {err:.1e}')
    assert err <= fc.PARITY


def test_array_api(emu_lib):  # noqa: F811
    """rollout.rollout(feedback=...): numpy in and out, equal to the same call in pieces; lqr.nominal_from_rollout closes the loop on an
    open-loop rollout: with k = 0 and the start on the nominal, dx stays at rounding level and the closed loop repeats it."""
    from flybody_amd import engine, lqr, rollout
    from test_rollout_emulation import ctrl_rows
    model, om, a = _load('walk_on_ball', emu_lib)
    q, v, act, _ = _other_task_state(model, a)
    nq, nv, na, nu = (model.dim(k) for k in ('nq', 'nv', 'na', 'nu'))
    ctrl = ctrl_rows(a, 2, 3, seed=3)
    open_ = rollout.rollout(model, q, v, act, ctrl, n_substeps=2, sensors=True)
    assert open_.ctrl is None
    x_nom, u_nom = lqr.nominal_from_rollout(np.r_[q, v, act], open_.state, ctrl)
    K = 0.1*np.random.default_rng(1).normal(size=(2, 3, nu, 2*nv + na))
    closed = rollout.rollout(model, q, v, act, feedback=engine.Feedback(x_nom, u_nom, K), n_substeps=2, sensors=True, batch_size=1)
    assert closed.state.shape == (2, 3, nq + nv + na) and closed.ctrl.shape == (2, 3, nu) and closed.status.tolist() == [0, 0]
    # dx is exactly zero on every column but the ball joint's three: the rotation that takes a quaternion to itself is the rounding of
    # one quaternion product (a few ulp of 1), which the gains carry into the inputs
    assert np.abs(closed.ctrl - ctrl).max() <= 3*np.abs(K).max()*8*np.finfo(float).eps
    assert np.allclose(closed.state, open_.state, rtol=0, atol=1e-12) and np.allclose(closed.sensordata, open_.sensordata, rtol=1e-9, atol=1e-12)
    # a perturbed start: the loop acts; one nominal without its axis, and n states against n nominals
    q2 = q.copy(); q2[-1] += 0.05
    one = rollout.rollout(model, q2, v, act, feedback=engine.Feedback(x_nom[0], u_nom[0], K[0]), n_substeps=2)
    assert one.state.shape == (3, nq + nv + na) and one.ctrl.shape == (3, nu) and one.status == 0 and not np.array_equal(one.ctrl, ctrl[0])
    two = rollout.rollout(model, np.array([q2, q]), np.array([v, v]), np.array([act, act]), feedback=engine.Feedback(x_nom, u_nom, K), n_substeps=2)
    assert np.array_equal(two.state[0], one.state) and np.array_equal(two.state[1], closed.state[1])
    half = rollout.rollout(model, q2, v, act, feedback=engine.Feedback(x_nom, u_nom, K, None, np.array([1.0, 0.5, 0.0]), [0, 0, 1]), n_substeps=2)
    assert half.state.shape[0] == 3 and np.array_equal(half.state[0], one.state) and np.array_equal(half.state[1], one.state)    # (k is None: alpha multiplies nothing)
    with pytest.raises(ValueError):
        rollout.rollout(model, q, v, act, ctrl, feedback=engine.Feedback(x_nom, u_nom))
    with pytest.raises(ValueError):
        rollout.rollout(model, q, v, act, feedback=engine.Feedback(x_nom, u_nom[:, :2]))
