"""flybody_amd/lqr.py: the host-side pieces between transition derivatives and a closed-loop rollout.  CPU, numpy only, no engine."""
import os
import types

import numpy as np
import pytest

from flybody_amd import derivatives, lqr
from flybody_amd.engine import ASSETS, load_npz


def random_system(rng, ndx=6, nu=2, T=20):
    """A time-varying system around an unstable A: controllable through dense B (stabilisable)."""
    A0 = 1.05*np.linalg.qr(rng.normal(size=(ndx, ndx)))[0]
    A = A0 + 0.05*rng.normal(size=(T, ndx, ndx))
    B = rng.normal(size=(T, ndx, nu))
    M = rng.normal(size=(ndx, ndx)); Q = M @ M.T + np.eye(ndx)
    N = rng.normal(size=(nu, nu)); R = N @ N.T + np.eye(nu)
    return A, B, Q, R


def closed_loop_cost(A, B, Q, R, Qf, K, x0):
    x, J = x0, 0.0
    for t in range(len(A)):
        u = K[t] @ x
        J += x @ Q @ x + u @ R @ u
        x = A[t] @ x + B[t] @ u
    return J + x @ Qf @ x


def test_tvlqr_cost_to_go_is_the_simulated_cost_and_the_gains_are_optimal():
    rng = np.random.default_rng(0)
    A, B, Q, R = random_system(rng)
    Qf = 3*Q
    K, P = lqr.tvlqr(A, B, Q, R, Qf)
    assert K.shape == (20, 2, 6) and P.shape == (21, 6, 6) and np.array_equal(P[20], Qf)
    for _ in range(5):
        x0 = rng.normal(size=6)
        J = closed_loop_cost(A, B, Q, R, Qf, K, x0)
        assert abs(J - x0 @ P[0] @ x0) <= 1e-9*J, (J, x0 @ P[0] @ x0)
        assert J < closed_loop_cost(A, B, Q, R, Qf, np.zeros_like(K), x0)       # (A is unstable: the open loop costs more)
        for t in (0, 7, 19):
            for _ in range(3):
                Kp = K.copy(); Kp[t] += 1e-3*rng.normal(size=(2, 6))
                assert closed_loop_cost(A, B, Q, R, Qf, Kp, x0) > J, t
    # leading axes are independent trajectories; Qf defaults to Q
    A2, B2 = np.stack([A, A[::-1]]), np.stack([B, B[::-1]])
    K2, P2 = lqr.tvlqr(A2, B2, Q, R)
    Kb, Pb = lqr.tvlqr(A[::-1], B[::-1], Q, R)
    assert K2.shape == (2, 20, 2, 6) and np.array_equal(K2[1], Kb) and np.array_equal(P2[1], Pb) and np.array_equal(P2[0, 20], Q)
    with pytest.raises(ValueError):
        lqr.tvlqr(A, B[:, :5], Q, R)
    with pytest.raises(ValueError):
        lqr.tvlqr(A, B, Q[:5, :5], R)


def test_lqr_fixed_point_satisfies_the_riccati_equation():
    rng = np.random.default_rng(1)
    A, B, Q, R = random_system(rng)
    A, B = A[0], B[0]
    tol = 1e-11
    K, P = lqr.lqr(A, B, Q, R, iters=5000, tol=tol)
    BtP = B.T @ P
    res = Q + A.T @ P @ A - A.T @ P @ B @ np.linalg.solve(R + BtP @ B, BtP @ A) - P
    assert np.abs(res).max() <= tol*np.abs(P).max()*(1 + 1e-3), np.abs(res).max()/np.abs(P).max()      # (the residual lqr itself tested, formed once more)
    assert np.abs(np.linalg.eigvals(A + B @ K)).max() < 1 < np.abs(np.linalg.eigvals(A)).max()
    assert np.allclose(K, -np.linalg.solve(R + BtP @ B, BtP @ A), rtol=0, atol=1e-9)
    with pytest.raises(RuntimeError):
        lqr.lqr(A, B, Q, R, iters=3, tol=1e-14)
    with pytest.raises(ValueError):
        lqr.lqr(A, B.T, Q, R)


@pytest.fixture(scope='module')
def walk_shim():
    return types.SimpleNamespace(arrays=dict(load_npz(os.path.join(ASSETS, 'walk_imitation.npz'))))


def test_state_difference_inverts_integrate_pos(walk_shim):
    a = walk_shim.arrays
    nq, nv = len(a['qpos0']), len(a['dof_bodyid'])
    na = int((np.asarray(a['actuator_actadr']) >= 0).sum())
    rng = np.random.default_rng(2)
    q = np.array(a['qpos0'], float); quat = rng.normal(size=4); q[3:7] = quat/np.linalg.norm(quat)
    x_nom = np.r_[q, rng.normal(size=nv), rng.normal(size=na)]
    for angle in (1e-6, 0.3, 3.0):                       # below half a turn
        d = np.r_[0.1*rng.normal(size=nv), rng.normal(size=nv), rng.normal(size=na)]
        axis = rng.normal(size=3); d[3:6] = angle*axis/np.linalg.norm(axis)
        x = np.r_[derivatives.integrate_pos(walk_shim, q, d[:nv]), x_nom[nq:] + d[nv:]]
        got = lqr.state_difference(walk_shim, x, x_nom)
        assert got.shape == (2*nv + na,) and np.abs(got - d).max() <= 1e-13*max(1.0, angle), (angle, np.abs(got - d).max())
    assert np.array_equal(lqr.state_difference(walk_shim, x_nom, x_nom)[6:], np.zeros(2*nv + na - 6))
    both = lqr.state_difference(walk_shim, np.stack([x, x_nom]), np.stack([x_nom, x_nom]))         # leading axes
    assert both.shape == (2, 2*nv + na) and np.array_equal(both[0], got)
    with pytest.raises(ValueError):
        lqr.state_difference(walk_shim, x, x_nom[:-1])


def test_nominal_from_rollout_is_the_shifted_layout():
    rng = np.random.default_rng(3)
    state, ctrl, x0 = rng.normal(size=(4, 5, 7)), rng.normal(size=(4, 5, 3)), rng.normal(size=(4, 7))
    x_nom, u_nom = lqr.nominal_from_rollout(x0, state, ctrl)
    assert x_nom.shape == (4, 5, 7) and np.array_equal(x_nom[:, 0], x0) and np.array_equal(x_nom[:, 1:], state[:, :-1])
    assert np.array_equal(u_nom, ctrl) and x_nom.flags.c_contiguous and u_nom.flags.c_contiguous
    one, _ = lqr.nominal_from_rollout(x0[0], state[0], ctrl[0])
    assert np.array_equal(one, x_nom[0])
    shared, _ = lqr.nominal_from_rollout(x0[0], state, ctrl)                   # one start state for all rollouts
    assert np.array_equal(shared[:, 0], np.tile(x0[0], (4, 1))) and np.array_equal(shared[:, 1:], state[:, :-1])
    with pytest.raises(ValueError):
        lqr.nominal_from_rollout(x0[:3], state, ctrl)
