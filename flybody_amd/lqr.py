"""From transition derivatives to feedback gains: the host-side pieces between ``derivatives.transition_fd`` and a closed-loop rollout.

The chain is  nominal rollout -> ``A_t, B_t`` along it -> ``tvlqr`` -> ``K_t`` -> ``engine.Batch.rollout_feedback`` (or
``rollout.rollout(feedback=...)``), which applies ``u_t = clamp(u_nom_t + alpha k_t + K_t (x_t (-) x_nom_t))`` on the device.  Everything
here is plain numpy in FP64, which is enough for one nominal; for a batch of nominals the Riccati recursion of a 275-dimensional tangent
space is the longest leg of the chain, and ``engine.Batch.lqr_backward`` runs it on the device, on derivatives that never leave it
(``tvlqr`` and ``lqr`` take ``batch=`` to go that way; ``backward_pass`` is its counterpart here, with the gradient terms and the
regularisation of iLQR).

Conventions: ``x = (qpos, qvel, act)`` with the tangent ``dx = (dq[nv], dv[nv], dact[na])`` of ``derivatives`` (``ndx = 2 nv + na``);
the linear model is ``dx_{t+1} = A_t dx_t + B_t du_t``; the cost is ``sum_t (dx_t' Q dx_t + du_t' R du_t) + dx_T' Qf dx_T``; the gain is
returned in the convention ``u = u_nom + K dx`` (so ``K = -(R + B'PB)^-1 B'PA``).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from . import engine, inverse_dynamics


def state_difference(model, x: np.ndarray, x_nom: np.ndarray) -> np.ndarray:
    """x (-) x_nom in the tangent space: (dq[nv], dv[nv], dact[na]) with dq = differentiate_pos(x_nom.qpos, x.qpos, 1) -- subtraction for
    hinge and slide joints and free-joint translation, the body-frame rotation vector that takes the nominal quaternion to the state's
    for free- and ball-joint rotation -- and plain differences of qvel and act.  What the feedback kernel multiplies the gains with.
    x, x_nom: (..., nq + nv + na), leading axes broadcast; model: an engine.Model, an asset name, or anything with the model's `.arrays`."""
    a = engine.as_model(model).arrays
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


def _on_device(batch, *arrays):
    """The arrays as contiguous FP64 torch tensors where `batch` computes (None stays None)."""
    import torch
    dev = batch._torch_device()
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev) for a in arrays]


def _refuse_failed(status, what):
    bad = np.flatnonzero(status)
    if len(bad):
        raise np.linalg.LinAlgError(f'{what}: R + B\'PB is not positive definite for nominal {int(bad[0])} at interval {int(status[bad[0]]) - 1}')


def backward_pass(A, B, Q, R, Qf=None, q=None, r=None, mu=None):
    """The backward pass of LQR / iLQR in numpy FP64, the host counterpart of engine.Batch.lqr_backward (include/flybody_engine.h states
    the formulas).  A (..., T, ndx, ndx), B (..., T, ndx, nu) with independent leading axes, Q / Qf (ndx, ndx) (Qf None: Q), R (nu, nu);
    optional q (..., T + 1, ndx), r (..., T, nu) -- the cost's gradient terms, 2 q_t'dx + 2 r_t'du -- and mu (...), added to the diagonal of
    Quu for the gains only.  Returns (K (..., T, nu, ndx), k (..., T, nu), P (..., T + 1, ndx, ndx), p (..., T + 1, ndx), dV (..., 2),
    status (...)): u = u_nom + alpha k + K dx, the value dx'P_t dx + 2 p_t'dx, the predicted change of the cost alpha dV[0] + alpha^2 dV[1],
    and status 0 or 1 + the first interval whose Quu + mu I has no Cholesky factor (that trajectory's outputs are zero from there down)."""
    A = np.asarray(A, np.float64); B = np.asarray(B, np.float64); Q = np.asarray(Q, np.float64); R = np.asarray(R, np.float64)
    if A.ndim < 3 or B.ndim != A.ndim or A.shape[-1] != A.shape[-2] or B.shape[:-1] != A.shape[:-1]:
        raise ValueError(f'A must be (..., T, ndx, ndx) and B (..., T, ndx, nu), got {A.shape} and {B.shape}')
    T, ndx, nu = A.shape[-3], A.shape[-1], B.shape[-1]
    lead = A.shape[:-3]
    Qf = Q if Qf is None else np.asarray(Qf, np.float64)
    q = np.zeros(lead + (T + 1, ndx)) if q is None else np.asarray(q, np.float64)
    r = np.zeros(lead + (T, nu)) if r is None else np.asarray(r, np.float64)
    mu = np.zeros(lead) if mu is None else np.asarray(mu, np.float64)
    if Q.shape != (ndx, ndx) or R.shape != (nu, nu) or Qf.shape != (ndx, ndx) or q.shape != lead + (T + 1, ndx) or r.shape != lead + (T, nu) \
            or mu.shape != lead:
        raise ValueError(f'Q and Qf must be ({ndx}, {ndx}), R ({nu}, {nu}), q {lead + (T + 1, ndx)}, r {lead + (T, nu)} and mu {lead}')
    n = int(np.prod(lead, dtype=np.int64))
    A = A.reshape((n, T, ndx, ndx)); B = B.reshape((n, T, ndx, nu)); q = q.reshape((n, T + 1, ndx)); r = r.reshape((n, T, nu)); mu = mu.reshape(n)
    K = np.zeros((n, T, nu, ndx)); k = np.zeros((n, T, nu)); P = np.zeros((n, T + 1, ndx, ndx)); p = np.zeros((n, T + 1, ndx))
    dV = np.zeros((n, 2)); status = np.zeros(n, np.int32)
    for m in range(n):
        P[m, T] = Qf; p[m, T] = q[m, T]
        for t in range(T - 1, -1, -1):
            At, Bt, Pn, pn = A[m, t], B[m, t], P[m, t + 1], p[m, t + 1]
            W = Pn @ At; Y = Pn @ Bt
            Qxx = Q + At.T @ W; Qux = Bt.T @ W; Quu = R + Bt.T @ Y
            Qx = q[m, t] + At.T @ pn; Qu = r[m, t] + Bt.T @ pn
            try:
                with np.errstate(all='ignore'):
                    L = np.linalg.cholesky(Quu + mu[m]*np.eye(nu))
                if not np.isfinite(L).all():
                    raise np.linalg.LinAlgError
            except np.linalg.LinAlgError:
                status[m] = 1 + t; dV[m] = 0.0
                K[m, :t + 1] = 0.0; k[m, :t + 1] = 0.0; P[m, :t + 1] = 0.0; p[m, :t + 1] = 0.0
                break
            solve = lambda b: np.linalg.solve(L.T, np.linalg.solve(L, b))
            Kt = -solve(Qux); kt = -solve(Qu)
            Pt = Qxx + Kt.T @ Quu @ Kt + Kt.T @ Qux + Qux.T @ Kt
            K[m, t] = Kt; k[m, t] = kt; P[m, t] = 0.5*(Pt + Pt.T)
            p[m, t] = Qx + Kt.T @ (Quu @ kt + Qu) + Qux.T @ kt
            dV[m] += (2.0*(kt @ Qu), kt @ Quu @ kt)
    return (K.reshape(lead + (T, nu, ndx)), k.reshape(lead + (T, nu)), P.reshape(lead + (T + 1, ndx, ndx)), p.reshape(lead + (T + 1, ndx)),
            dV.reshape(lead + (2,)), status.reshape(lead))


def tvlqr(A: np.ndarray, B: np.ndarray, Q: np.ndarray, R: np.ndarray, Qf: Optional[np.ndarray] = None, batch=None) -> Tuple[np.ndarray, np.ndarray]:
    """Time-varying LQR by the backward Riccati recursion.  A (..., T, ndx, ndx), B (..., T, ndx, nu) -- the leading axes are independent
    trajectories --, Q (ndx, ndx), R (nu, nu) positive definite, Qf (ndx, ndx) the terminal weight (None: Q).  Returns
    (K (..., T, nu, ndx), P (..., T + 1, ndx, ndx)): u_t = u_nom_t + K_t dx_t minimises the cost of the linear model, and dx' P_t dx is
    the cost-to-go from interval t (P_T = Qf).  batch: an engine.Batch; the recursion then runs on its device (Batch.lqr_backward) and the
    same arrays come back as numpy (LinAlgError where R + B'PB is not positive definite)."""
    A = np.asarray(A, np.float64); B = np.asarray(B, np.float64); Q = np.asarray(Q, np.float64); R = np.asarray(R, np.float64)
    if A.ndim < 3 or B.ndim != A.ndim or A.shape[-1] != A.shape[-2] or B.shape[:-1] != A.shape[:-1]:
        raise ValueError(f'A must be (..., T, ndx, ndx) and B (..., T, ndx, nu), got {A.shape} and {B.shape}')
    T, ndx, nu = A.shape[-3], A.shape[-1], B.shape[-1]
    Qf = Q if Qf is None else np.asarray(Qf, np.float64)
    if Q.shape != (ndx, ndx) or R.shape != (nu, nu) or Qf.shape != (ndx, ndx):
        raise ValueError(f'Q and Qf must be ({ndx}, {ndx}) and R ({nu}, {nu})')
    lead = A.shape[:-3]
    if batch is not None:
        res = batch.lqr_backward(*_on_device(batch, A.reshape((-1, T, ndx, ndx)), B.reshape((-1, T, ndx, nu)), Q, R, Qf), want_P=True)
        _refuse_failed(res.status.cpu().numpy(), 'tvlqr')
        return res.K.cpu().numpy().reshape(lead + (T, nu, ndx)), res.P.cpu().numpy().reshape(lead + (T + 1, ndx, ndx))
    K = np.empty(lead + (T, nu, ndx)); P = np.empty(lead + (T + 1, ndx, ndx))
    P[..., T, :, :] = Qf
    for t in range(T - 1, -1, -1):
        K[..., t, :, :], P[..., t, :, :] = _riccati_step(A[..., t, :, :], B[..., t, :, :], Q, R, P[..., t + 1, :, :])
    return K, P


def lqr(A: np.ndarray, B: np.ndarray, Q: np.ndarray, R: np.ndarray, iters: int = 10_000, tol: float = 1e-10, batch=None) -> Tuple[np.ndarray, np.ndarray]:
    """Infinite-horizon LQR of one linear model A (ndx, ndx), B (ndx, nu): the recursion of tvlqr iterated from P = Q until
    max |riccati(P) - P| <= tol max |P| (RuntimeError after `iters` steps without it: the pair is not stabilisable, or tol is below
    what FP64 resolves).  Returns (K (nu, ndx), P (ndx, ndx)) with u = u_nom + K dx; P then satisfies the discrete algebraic Riccati
    equation to that tolerance.  batch: an engine.Batch; the recursion then runs on its device in stationary mode (Batch.lqr_backward), in
    rounds of doubling length from the terminal weight Q until the last step of a round meets the same test -- the iterates are those of
    the loop here, so the result is, to rounding, the one it would stop at or a later one."""
    A = np.asarray(A, np.float64); B = np.asarray(B, np.float64); Q = np.asarray(Q, np.float64); R = np.asarray(R, np.float64)
    if A.ndim != 2 or A.shape[0] != A.shape[1] or B.ndim != 2 or B.shape[0] != A.shape[0] or Q.shape != A.shape or R.shape != (B.shape[1],)*2:
        raise ValueError('A and Q must be (ndx, ndx), B (ndx, nu) and R (nu, nu)')
    if batch is not None:
        Ad, Bd, Qd, Rd = _on_device(batch, A[None], B[None], Q, R)
        H = 64
        while True:
            H = min(H, int(iters))
            res = batch.lqr_backward(Ad, Bd, Qd, Rd, stationary=True, horizon=H, want_P=True)
            _refuse_failed(res.status.cpu().numpy(), 'lqr')
            P0, P1 = res.P[0, 0].cpu().numpy(), res.P[0, 1].cpu().numpy()
            if np.abs(P0 - P1).max() <= tol*np.abs(P1).max():
                return res.K[0, 0].cpu().numpy(), P1                             # (K is P_1's gain, as below)
            if H >= int(iters):
                raise RuntimeError(f'lqr: no fixed point within {int(iters)} iterations at tol {tol}')
            H *= 2
    P = Q
    for _ in range(int(iters)):
        K, Pn = _riccati_step(A, B, Q, R, P)
        if np.abs(Pn - P).max() <= tol*np.abs(P).max():  # the Riccati residual of P itself, and K is P's gain
            return K, P
        P = Pn
    raise RuntimeError(f'lqr: no fixed point within {int(iters)} iterations at tol {tol}')
