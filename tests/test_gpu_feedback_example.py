"""The README's closed-loop example as a test: nominal rollout -> derivatives.transition_fd along it -> lqr.tvlqr ->
closed-loop rollouts from perturbed starts.  The walking fly held in the air under a constant mid-range input; eight starts with the
leg and body joints off the nominal; the gains must do in the simulation what the linear model says they do."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

T, N_START = 5, 8


def weights(nv, na, nu, width):
    """Q: the hinge angles (the root floats free in the air and no actuator reaches it: weight 0), a little on their velocities;
    R: cheap inputs, in units of each actuator's range."""
    q = np.r_[np.zeros(6), np.ones(nv - 6), np.zeros(6), 1e-6*np.ones(nv - 6), np.zeros(na)]
    return np.diag(q), np.diag(1e-3/width**2)


def cost(dx, du, Q, R):
    """sum_t dx_t' Q dx_t + du_t' R du_t + dx_T' Q dx_T for dx [.., T + 1, ndx], du [.., T, nu]."""
    return np.einsum('...ti,ij,...tj->...', dx, Q, dx) + np.einsum('...ti,ij,...tj->...', du, R, du)


def run_example(model, shim):
    """Returns (linear open-loop cost, linear closed-loop cost, simulated open-loop cost, simulated closed-loop cost, status), each [8]."""
    from conftest import random_state
    from flybody_amd import derivatives, engine, lqr, rollout
    from test_deriv_emulation import mid_ctrl
    a = shim.arrays
    nq, nv, na, nu = (model.dim(k) for k in ('nq', 'nv', 'na', 'nu'))
    rng = np.random.default_rng(0)
    q0, v0 = random_state(a, np.random.default_rng(0), spread=0.0, z=2.0)
    act0 = np.zeros(na)
    u_bar = np.tile(mid_ctrl(a, rng, 0.45, 0.55), (T, 1))
    # 1. the nominal: one open-loop rollout, and its states at the START of every interval
    nom = rollout.rollout(model, q0, v0, act0, u_bar)
    x_nom, u_nom = lqr.nominal_from_rollout(np.r_[q0, v0, act0], nom.state, u_bar)
    # 2. A_t, B_t of one control interval along it
    fd = derivatives.transition_fd(model, x_nom[:, :nq], x_nom[:, nq:nq + nv], x_nom[:, nq + nv:], u_nom, n_substeps=model.dim('nsubstep'))
    assert not np.asarray(fd.status).any()
    # 3. gains
    width = np.asarray(a['actuator_ctrlrange'], float) @ [-1.0, 1.0]
    Q, R = weights(nv, na, nu, width)
    K, P = lqr.tvlqr(fd.A, fd.B, Q, R)
    # the starts: hinge angles 0.02 rad and hinge velocities 0.5 rad/s off the nominal
    d0 = np.zeros((N_START, 2*nv + na))
    d0[:, 6:nv] = 0.02*rng.normal(size=(N_START, nv - 6)); d0[:, nv + 6:2*nv] = 0.5*rng.normal(size=(N_START, nv - 6))
    # what the linear model predicts, open and closed loop
    lin = []
    for gains in (np.zeros_like(K), K):
        dx = [d0]; du = []
        for t in range(T):
            du.append(dx[-1] @ gains[t].T)
            dx.append(dx[-1] @ fd.A[t].T + du[-1] @ fd.B[t].T)
        lin.append(cost(np.stack(dx, 1), np.stack(du, 1), Q, R))
    # 4. the simulation: open loop under u_nom, closed loop under the gains
    qs = derivatives.integrate_pos(shim, np.tile(q0, (N_START, 1)), d0[:, :nv])
    vs, acts = v0 + d0[:, nv:2*nv], act0 + d0[:, 2*nv:]
    open_ = rollout.rollout(model, qs, vs, acts, np.tile(u_bar, (N_START, 1, 1)))
    closed = rollout.rollout(model, qs, vs, acts, feedback=engine.Feedback(x_nom, u_nom, K))
    x_end = np.concatenate([x_nom, nom.state[-1:]])     # the nominal at the start of every interval and behind the last
    sim = []
    for r, u in ((open_, np.tile(u_bar, (N_START, 1, 1))), (closed, closed.ctrl)):
        x = np.concatenate([np.c_[qs, vs, acts][:, None], r.state], axis=1)
        sim.append(cost(lqr.state_difference(shim, x, np.broadcast_to(x_end, x.shape)), u - u_nom, Q, R))
    return lin[0], lin[1], sim[0], sim[1], np.r_[open_.status, closed.status]


def test_tvlqr_gains_lower_the_simulated_cost():
    import types
    from flybody_amd import engine
    model = engine.Model.from_asset('walk_imitation')
    lin_open, lin_closed, sim_open, sim_closed, status = run_example(model, types.SimpleNamespace(arrays=model.arrays))
    for i in range(N_START):
        print(f'start {i}: linear model open {lin_open[i]:.4e} closed {lin_closed[i]:.4e} ({lin_closed[i]/lin_open[i]:.2f})   '
              f'simulated open {sim_open[i]:.4e} closed {sim_closed[i]:.4e} ({sim_closed[i]/sim_open[i]:.2f})')
    assert (lin_closed <= 0.9*lin_open).all(), lin_closed/lin_open              # precondition, checkable without the kernel: Q, R leave the loop >= 10 % to gain
    assert (status == 0).all()
    assert (sim_closed < sim_open).all(), sim_closed/sim_open
