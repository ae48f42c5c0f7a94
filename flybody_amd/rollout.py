"""Batched open-loop rollouts on the GPU, in the manner of MuJoCo's ``rollout`` module.

*What happens if this control sequence is applied from here?* is the call sampling planners (predictive sampling, MPPI, CEM) and the
line search of iLQR are built on.  One rollout is one ticket of one kernel launch (fb_batch_rollout, csrc/fb_rollout.hpp): it starts
from a state, holds ``ctrl[t]`` over the ``n_substeps`` physics substeps of interval ``t`` and records ``(qpos, qvel, act)`` -- and the
sensors -- after every interval; thousands run at once on a fixed pool of scratch rows.  ``rollout`` below takes arrays and returns
numpy; for live environments use ``fly_envs.BatchedFlyEnv.rollout`` (actions through the task's hook, torch tensors on the device),
for a batch of your own ``engine.Batch.rollout``.  FP64 only; there is no CPU path: without a GPU the batch cannot be created and this
raises.
"""
from __future__ import annotations

import collections
from typing import Optional, Union

import numpy as np

from . import engine

# rollout(): numpy arrays; state (.., T, nq + nv + na) = (qpos, qvel, act), which are views into it; sensordata None unless asked for
RolloutResult = collections.namedtuple('RolloutResult', ['state', 'qpos', 'qvel', 'act', 'sensordata', 'status'])


def _model(model):
    return engine.Model.from_asset(model) if isinstance(model, str) else model


def rollout(model_or_task_name: Union['engine.Model', str], qpos: np.ndarray, qvel: np.ndarray, act: Optional[np.ndarray] = None,
            ctrl: Optional[np.ndarray] = None, n_substeps: int = 0, sensors: bool = False, device: int = 0,
            batch_size: int = 1024) -> RolloutResult:
    """Roll the control sequences `ctrl` out from the given states:
    RolloutResult(state (T, nq + nv + na), qpos (T, nq), qvel (T, nv), act (T, na), sensordata (T, 33) or None, status) for one state --
    qpos (nq,), qvel (nv,), act (na,), zeros when None -- and one sequence ctrl (T, nu); with a leading axis n for (n, T, nu)
    sequences.  One initial state broadcasts against n sequences (n samples from one state), or there are n of each.

    Interval t holds ctrl[t] (clamped to ctrlrange by the actuation stage) over n_substeps physics substeps (0: the model's own count,
    one control step) and records the state behind it; sensordata is what the interval's last substep leaves.
    model_or_task_name: an engine.Model (FP64 engine library) or an asset name ('walk_imitation', 'flight_imitation', 'walk_on_ball').
    The distinct initial states are set on a helper batch of at most `batch_size` environments on GPU `device`; a forward evaluation
    there defines the warm start of each rollout's first constraint solve (its acceleration).  status: the OR of the engine's WARN bits
    (engine.WARN_BITS) over the rollout -- non-zero means a cap or an iteration limit was hit on the way."""
    import torch
    model = _model(model_or_task_name)
    nq, nv, na, nu = (model.dim(k) for k in ('nq', 'nv', 'na', 'nu'))
    if ctrl is None:
        raise ValueError('rollout needs the control sequences ctrl (T, nu) or (n, T, nu)')
    u = np.asarray(ctrl, np.float64)
    q = np.asarray(qpos, np.float64); v = np.asarray(qvel, np.float64)
    single = u.ndim == 2
    if single:
        u = u[None]
    one_state = q.ndim == 1
    if one_state:
        q, v = q[None], v[None]
    ns = len(q)
    a_ = np.zeros((ns, na)) if act is None else np.asarray(act, np.float64).reshape(ns, -1)
    if u.ndim != 3 or u.shape[2] != nu or u.shape[1] < 1 or q.ndim != 2 or q.shape[1] != nq or v.shape != (ns, nv) or a_.shape != (ns, na):
        raise ValueError(f'ctrl must be (T, {nu}) or (n, T, {nu}) with T >= 1; qpos ({nq},), qvel ({nv},) and act ({na},), or (n, ...) with the same n')
    n, T = u.shape[0], u.shape[1]
    if not one_state and ns != n:
        raise ValueError(f'{ns} initial states for {n} control sequences: give one state, or one per sequence')
    if int(batch_size) < 1:
        raise ValueError('batch_size must be >= 1')
    nx = nq + nv + na
    dev = 'cpu' if b'emulation' in model.L.fb_version() else f'cuda:{device}'      # (the tests' kernel-emulation build: "device" memory is host memory)
    state = np.empty((n, T, nx)); status = np.empty(n, np.int32)
    sens = np.empty((n, T, engine.NSENSOR)) if sensors else None
    batch, bn = None, 0
    for lo in range(0, n, int(batch_size)):
        hi = min(n, lo + int(batch_size))
        rows = 1 if one_state else hi - lo               # environments of the helper batch: the distinct states of this chunk
        if batch is None or bn != rows:
            batch, bn = engine.Batch(model, rows, device=device, precision=64), rows
        if lo == 0 or not one_state:
            s = slice(0, 1) if one_state else slice(lo, hi)
            batch.set('QPOS', q[s]); batch.set('QVEL', v[s])
            if na:
                batch.set('ACT', a_[s])
            batch.forward()
        ids = np.zeros(hi - lo, np.int32) if one_state else np.arange(hi - lo, dtype=np.int32)
        r = batch.rollout(ctrl=torch.from_numpy(np.ascontiguousarray(u[lo:hi])).to(dev), env_ids=ids, n_substeps=n_substeps,
                          sensors=sensors)
        batch.synchronize()
        state[lo:hi] = r.state.cpu().numpy(); status[lo:hi] = r.status.cpu().numpy()
        if sensors:
            sens[lo:hi] = r.sensordata.cpu().numpy()
    if single:
        state, status, sens = state[0], int(status[0]), None if sens is None else sens[0]
    return RolloutResult(state, state[..., :nq], state[..., nq:nq + nv], state[..., nq + nv:], sens, status)
