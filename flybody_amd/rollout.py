"""Batched rollouts on the GPU, in the manner of MuJoCo's ``rollout`` module.

*What happens if this control sequence is applied from here?* is the call sampling planners (predictive sampling, MPPI, CEM) and the
line search of iLQR are built on.  One rollout is one ticket of one kernel launch (fb_batch_rollout, csrc/fb_rollout.hpp): it starts
from a state, holds ``ctrl[t]`` over the ``n_substeps`` physics substeps of interval ``t`` and records ``(qpos, qvel, act)`` -- and the
sensors -- after every interval; thousands run at once on a fixed pool of scratch rows.  ``rollout`` below takes arrays and returns
numpy; for live environments use ``fly_envs.BatchedFlyEnv.rollout`` (actions through the task's hook, torch tensors on the device),
for a batch of your own ``engine.Batch.rollout``.  With ``feedback=`` the rollouts are CLOSED-LOOP (fb_batch_rollout_feedback): the
input of interval ``t`` is a time-varying affine feedback on the state the rollout has reached, evaluated on the device (gains:
``flybody_amd.lqr``).  FP64 only; there is no CPU path: without a GPU the batch cannot be created and this raises.
"""
from __future__ import annotations

import collections
from typing import Optional, Union

import numpy as np

from . import engine

# rollout(): numpy arrays; state (.., T, nq + nv + na) = (qpos, qvel, act), which are views into it; sensordata None unless asked for;
# ctrl (.., T, nu): the inputs a closed-loop rollout applied (None for an open-loop one)
RolloutResult = collections.namedtuple('RolloutResult', ['state', 'qpos', 'qvel', 'act', 'sensordata', 'status', 'ctrl'], defaults=(None,))


def _feedback_arrays(feedback, nx, nu, ndx):
    """engine.Feedback of numpy arrays with the leading nominal axis ([n_nom, T, .]; one nominal may come without it)."""
    f = engine.Feedback(*feedback)
    x = np.asarray(f.x_nom, np.float64)
    lead = x.ndim == 2
    up = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, np.float64)[None] if lead else np.asarray(a, np.float64))
    x, u, K, k = up(f.x_nom), up(f.u_nom), up(f.K), up(f.k)
    if x.ndim != 3 or x.shape[2] != nx or x.shape[1] < 1 or u is None or u.shape != x.shape[:2] + (nu,) \
            or (K is not None and K.shape != x.shape[:2] + (nu, ndx)) or (k is not None and k.shape != u.shape):
        raise ValueError(f'feedback: x_nom (T, {nx}) or (n_nom, T, {nx}) with T >= 1, u_nom and k (.., T, {nu}), K (.., T, {nu}, {ndx})')
    alpha = None if f.alpha is None else np.ascontiguousarray(np.asarray(f.alpha, np.float64).reshape(-1))
    return x, u, K, k, alpha, engine.as_env_ids(f.nom_ids)


def rollout(model_or_task_name: Union['engine.Model', str], qpos: np.ndarray, qvel: np.ndarray, act: Optional[np.ndarray] = None,
            ctrl: Optional[np.ndarray] = None, n_substeps: int = 0, sensors: bool = False, device: int = 0,
            batch_size: int = 1024, feedback=None) -> RolloutResult:
    """Roll the control sequences `ctrl` out from the given states:
    RolloutResult(state (T, nq + nv + na), qpos (T, nq), qvel (T, nv), act (T, na), sensordata (T, 33) or None, status) for one state --
    qpos (nq,), qvel (nv,), act (na,), zeros when None -- and one sequence ctrl (T, nu); with a leading axis n for (n, T, nu)
    sequences.  One initial state broadcasts against n sequences (n samples from one state), or there are n of each.

    Interval t holds ctrl[t] (clamped to ctrlrange by the actuation stage) over n_substeps physics substeps (0: the model's own count,
    one control step) and records the state behind it; sensordata is what the interval's last substep leaves.
    model_or_task_name: an engine.Model (FP64 engine library) or an asset name ('walk_imitation', 'flight_imitation', 'walk_on_ball').
    The distinct initial states are set on a helper batch of at most `batch_size` environments on GPU `device`; a forward evaluation
    there defines the warm start of each rollout's first constraint solve (its acceleration).  status: the OR of the engine's WARN bits
    (engine.WARN_BITS) over the rollout -- non-zero means a cap or an iteration limit was hit on the way.

    feedback=engine.Feedback(x_nom, u_nom, K, k, alpha, nom_ids) instead of ctrl: CLOSED-LOOP rollouts (Batch.rollout_feedback),
    u_t = clamp(u_nom[t] + alpha k[t] + K[t] (x_t (-) x_nom[t])).  numpy arrays: x_nom (n_nom, T, nq + nv + na) -- the nominal state at
    the START of interval t --, u_nom and k (n_nom, T, nu), K (n_nom, T, nu, ndx), one nominal also without the leading axis; alpha (n,)
    and nom_ids (n,) per rollout (None: 1, and nominal r for rollout r -- or the one nominal for all).  The number of rollouts n is that
    of the states if there are several, else of nom_ids, alpha, or the nominals.  The result carries ctrl (n, T, nu), the inputs applied,
    and comes without the leading axis only for one state and one nominal given without theirs."""
    import torch
    model = engine.as_model(model_or_task_name)
    nq, nv, na, nu = (model.dim(k) for k in ('nq', 'nv', 'na', 'nu'))
    q = np.asarray(qpos, np.float64); v = np.asarray(qvel, np.float64)
    one_state = q.ndim == 1
    if one_state:
        q, v = q[None], v[None]
    ns = len(q)
    a_ = np.zeros((ns, na)) if act is None else np.asarray(act, np.float64).reshape(ns, -1)
    nx = nq + nv + na
    if feedback is not None:
        if ctrl is not None:
            raise ValueError('a closed-loop rollout computes its inputs: give feedback or ctrl, not both')
        xn, un, Kn, kn, alpha, noms = _feedback_arrays(feedback, nx, nu, 2*nv + na)
        single = one_state and np.asarray(engine.Feedback(*feedback).x_nom).ndim == 2 and alpha is None and noms is None
        n_nom, T = xn.shape[0], xn.shape[1]
        n = ns if not one_state else len(noms) if noms is not None else len(alpha) if alpha is not None else n_nom
        if noms is None:
            noms = np.zeros(n, np.int32) if n_nom == 1 else np.arange(n, dtype=np.int32)
        if len(noms) != n or (alpha is not None and len(alpha) != n) or noms.min() < 0 or noms.max() >= n_nom:
            raise ValueError(f'feedback: {n} rollouts need nom_ids ({len(noms)}) and alpha of that length, nominal ids in 0 .. {n_nom - 1}')
        if q.ndim != 2 or q.shape[1] != nq or v.shape != (ns, nv) or a_.shape != (ns, na):
            raise ValueError(f'qpos ({nq},), qvel ({nv},) and act ({na},), or (n, ...) with the same n')
    else:
        if ctrl is None:
            raise ValueError('rollout needs the control sequences ctrl (T, nu) or (n, T, nu)')
        u = np.asarray(ctrl, np.float64)
        single = u.ndim == 2
        if single:
            u = u[None]
        if u.ndim != 3 or u.shape[2] != nu or u.shape[1] < 1 or q.ndim != 2 or q.shape[1] != nq or v.shape != (ns, nv) or a_.shape != (ns, na):
            raise ValueError(f'ctrl must be (T, {nu}) or (n, T, {nu}) with T >= 1; qpos ({nq},), qvel ({nv},) and act ({na},), or (n, ...) with the same n')
        n, T = u.shape[0], u.shape[1]
        if not one_state and ns != n:
            raise ValueError(f'{ns} initial states for {n} control sequences: give one state, or one per sequence')
    state = np.empty((n, T, nx)); status = np.empty(n, np.int32)
    sens = np.empty((n, T, engine.NSENSOR)) if sensors else None
    applied = np.empty((n, T, nu)) if feedback is not None else None
    # (environments of the helper batch: the distinct states of a chunk)
    for batch, lo, hi in engine.helper_batches(model, n, batch_size, device, rows=1 if one_state else None):
        to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(batch._torch_device())
        if lo == 0 and feedback is not None:
            nominal = [to(a) for a in (xn, un, Kn, kn)]
        if lo == 0 or not one_state:
            s = slice(0, 1) if one_state else slice(lo, hi)
            batch.set('QPOS', q[s]); batch.set('QVEL', v[s])
            if na:
                batch.set('ACT', a_[s])
            batch.forward()
        ids = np.zeros(hi - lo, np.int32) if one_state else np.arange(hi - lo, dtype=np.int32)
        if feedback is not None:
            r = batch.rollout_feedback(*nominal, to(None if alpha is None else alpha[lo:hi]), nom_ids=noms[lo:hi], env_ids=ids,
                                       n_substeps=n_substeps, sensors=sensors)
        else:
            r = batch.rollout(ctrl=to(u[lo:hi]), env_ids=ids, n_substeps=n_substeps, sensors=sensors)
        batch.synchronize()
        state[lo:hi] = r.state.cpu().numpy(); status[lo:hi] = r.status.cpu().numpy()
        if sensors:
            sens[lo:hi] = r.sensordata.cpu().numpy()
        if applied is not None:
            applied[lo:hi] = r.ctrl.cpu().numpy()
    if single:
        state, status, sens = state[0], int(status[0]), None if sens is None else sens[0]
        applied = None if applied is None else applied[0]
    return RolloutResult(*engine.state_views(state, nq, nv), sens, status, applied)
