"""From transition derivatives to feedback gains: the host-side pieces between ``derivatives.transition_fd`` and a closed-loop rollout.

The chain is  nominal rollout -> ``A_t, B_t`` along it -> ``tvlqr`` -> ``K_t`` -> ``engine.Batch.rollout_feedback`` (or
``rollout.rollout(feedback=...)``), which applies ``u_t = clamp(u_nom_t + alpha k_t + K_t (x_t (-) x_nom_t))`` on the device.  Everything
here is plain numpy in FP64: the Riccati recursion of a 275-dimensional tangent space over tens of intervals is not the hot path.

Conventions: ``x = (qpos, qvel, act)`` with the tangent ``dx = (dq[nv], dv[nv], dact[na])`` of ``derivatives`` (``ndx = 2 nv + na``);
the linear model is ``dx_{t+1} = A_t dx_t + B_t du_t``; the cost is ``sum_t (dx_t' Q dx_t + du_t' R du_t) + dx_T' Qf dx_T``; the gain is
returned in the convention ``u = u_nom + K dx`` (so ``K = -(R + B'PB)^-1 B'PA``).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from . import inverse_dynamics


def state_difference(model, x: np.ndarray, x_nom: np.ndarray) -> np.ndarray:
    """x (-) x_nom in the tangent space: (dq[nv], dv[nv], dact[na]) with dq = differentiate_pos(x_nom.qpos, x.qpos, 1) -- subtraction for
    hinge and slide joints and free-joint translation, the body-frame rotation vector that takes the nominal quaternion to the state's
    for free- and ball-joint rotation -- and plain differences of qvel and act.  What the feedback kernel multiplies the gains with.
    x, x_nom: (..., nq + nv + na), leading axes broadcast; model: an engine.Model, an asset name, or anything with the model's `.arrays`."""
    a = inverse_dynamics._model(model).arrays
    nq = len(a['qpos0'])
    x = np.asarray(x, np.float64); xn = np.asarray(x_nom, np.float64)
    if x.shape[-1:] != xn.shape[-1:] or x.shape[-1] < nq:
        raise ValueError(f'x and x_nom must both be (..., nq + nv + na), got {x.shape} and {xn.shape}')
    x, xn = np.broadcast_arrays(x, xn)
    dq = inverse_dynamics.differentiate_pos(model, xn[..., :nq], x[..., :nq], 1.0)
    return np.concatenate([dq, x[..., nq:] - xn[..., nq:]], axis=-1)


def nominal_from_rollout(x0: np.ndarray, state: np.ndarray, ctrl: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(x_nom, u_nom) of a rollout, in the layout the feedback kernel wants: x_nom[t] is the state at the START of interval t, that is
    (x0, state[0], .., state[T-2]) for the rollout's records state (..., T, nx) -- which hold the state BEHIND every interval -- from the
    start state x0 (..., nx), or one start state (nx,) for all of them; u_nom = ctrl (..., T, nu).  Arrays come back contiguous FP64."""
    s = np.asarray(state, np.float64); x0 = np.asarray(x0, np.float64); u = np.asarray(ctrl, np.float64)
    if s.ndim < 2 or x0.shape not in (s.shape[:-2] + s.shape[-1:], s.shape[-1:]) or u.shape[:-1] != s.shape[:-1]:
        raise ValueError(f'state (..., T, nx) needs x0 (..., nx) and ctrl (..., T, nu), got {s.shape}, {x0.shape} and {u.shape}')
    x0 = np.broadcast_to(x0, s.shape[:-2] + s.shape[-1:])
    return np.ascontiguousarray(np.concatenate([x0[..., None, :], s[..., :-1, :]], axis=-2)), np.ascontiguousarray(u)


def _riccati_step(A, B, Q, R, P):
    """(K, P_prev) of one backward step: K = -(R + B'PB)^-1 B'PA, P_prev = Q + A'PA + A'PB K, symmetrised."""
    BtP = np.swapaxes(B, -1, -2) @ P
    K = -np.linalg.solve(R + BtP @ B, BtP @ A)
    AtP = np.swapaxes(A, -1, -2) @ P
    Pn = Q + AtP @ A + AtP @ B @ K
    return K, 0.5*(Pn + np.swapaxes(Pn, -1, -2))


def tvlqr(A: np.ndarray, B: np.ndarray, Q: np.ndarray, R: np.ndarray, Qf: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Time-varying LQR by the backward Riccati recursion.  A (..., T, ndx, ndx), B (..., T, ndx, nu) -- the leading axes are independent
    trajectories --, Q (ndx, ndx), R (nu, nu) positive definite, Qf (ndx, ndx) the terminal weight (None: Q).  Returns
    (K (..., T, nu, ndx), P (..., T + 1, ndx, ndx)): u_t = u_nom_t + K_t dx_t minimises the cost of the linear model, and dx' P_t dx is
    the cost-to-go from interval t (P_T = Qf)."""
    A = np.asarray(A, np.float64); B = np.asarray(B, np.float64); Q = np.asarray(Q, np.float64); R = np.asarray(R, np.float64)
    if A.ndim < 3 or B.ndim != A.ndim or A.shape[-1] != A.shape[-2] or B.shape[:-1] != A.shape[:-1]:
        raise ValueError(f'A must be (..., T, ndx, ndx) and B (..., T, ndx, nu), got {A.shape} and {B.shape}')
    T, ndx, nu = A.shape[-3], A.shape[-1], B.shape[-1]
    Qf = Q if Qf is None else np.asarray(Qf, np.float64)
    if Q.shape != (ndx, ndx) or R.shape != (nu, nu) or Qf.shape != (ndx, ndx):
        raise ValueError(f'Q and Qf must be ({ndx}, {ndx}) and R ({nu}, {nu})')
    lead = A.shape[:-3]
    K = np.empty(lead + (T, nu, ndx)); P = np.empty(lead + (T + 1, ndx, ndx))
    P[..., T, :, :] = Qf
    for t in range(T - 1, -1, -1):
        K[..., t, :, :], P[..., t, :, :] = _riccati_step(A[..., t, :, :], B[..., t, :, :], Q, R, P[..., t + 1, :, :])
    return K, P


def lqr(A: np.ndarray, B: np.ndarray, Q: np.ndarray, R: np.ndarray, iters: int = 10_000, tol: float = 1e-10) -> Tuple[np.ndarray, np.ndarray]:
    """Infinite-horizon LQR of one linear model A (ndx, ndx), B (ndx, nu): the recursion of tvlqr iterated from P = Q until
    max |riccati(P) - P| <= tol max |P| (RuntimeError after `iters` steps without it: the pair is not stabilisable, or tol is below
    what FP64 resolves).  Returns (K (nu, ndx), P (ndx, ndx)) with u = u_nom + K dx; P then satisfies the discrete algebraic Riccati
    equation to that tolerance."""
    A = np.asarray(A, np.float64); B = np.asarray(B, np.float64); Q = np.asarray(Q, np.float64); R = np.asarray(R, np.float64)
    if A.ndim != 2 or A.shape[0] != A.shape[1] or B.ndim != 2 or B.shape[0] != A.shape[0] or Q.shape != A.shape or R.shape != (B.shape[1],)*2:
        raise ValueError('A and Q must be (ndx, ndx), B (ndx, nu) and R (nu, nu)')
    P = Q
    for _ in range(int(iters)):
        K, Pn = _riccati_step(A, B, Q, R, P)
        if np.abs(Pn - P).max() <= tol*np.abs(P).max():  # the Riccati residual of P itself, and K is P's gain
            return K, P
        P = Pn
    raise RuntimeError(f'lqr: no fixed point within {int(iters)} iterations at tol {tol}')
