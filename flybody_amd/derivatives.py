"""Batched transition derivatives on the GPU: MuJoCo's ``mjd_transitionFD`` for the fly model's physics step.

How the next state depends on this one -- ``A = dx'/dx``, ``B = dx'/du`` and, for the sensors, ``C = ds'/dx``, ``D = ds'/du`` -- is what
LQR and pole placement need to choose control-law gains (``engine.Batch.set_control_law``), what the stability of hovering is read from
(the product of step Jacobians over a wing beat), and what iLQR / MPC linearise around the states that inverse kinematics and inverse
dynamics produce.  ``x = (qpos, qvel, act)`` lives in the tangent space ``dx = (dq[nv], dv[nv], dact[na])`` with ``dq`` in the joints'
velocity space (``integrate_pos`` / ``inverse_dynamics.differentiate_pos``), ``u = ctrl``.  Every (frame, column, side) perturbation is
one ticket of one kernel launch (fb_batch_transition_fd, csrc/fb_deriv.hpp); thousands run at once.  FP64 only; there is no CPU path:
without a GPU the batch cannot be created and this raises.
"""
from __future__ import annotations

from typing import List, Optional, Union

import numpy as np

from . import engine
from .engine import TransitionFD
from .inverse_dynamics import _JNT_BALL, _JNT_FREE, _quat_mul


def _quat_integrate(q, w):
    """q exp(w / 2), normalised: mju_quatIntegrate(q, w, 1) for the local rotation vector w."""
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    ang = np.linalg.norm(w, axis=-1, keepdims=True)
    axis = np.where(ang > 0, w/np.where(ang > 0, ang, 1.0), np.array([1.0, 0.0, 0.0]))
    r = _quat_mul(q, np.concatenate([np.cos(0.5*ang), axis*np.sin(0.5*ang)], axis=-1))
    return r / np.linalg.norm(r, axis=-1, keepdims=True)


def integrate_pos(model: Union['engine.Model', str], qpos: np.ndarray, dq: np.ndarray) -> np.ndarray:
    """mj_integratePos(m, qpos, dq, 1): the position a tangent displacement dq (nv,) leads to -- the counterpart of
    ``inverse_dynamics.differentiate_pos`` (``differentiate_pos(m, q, integrate_pos(m, q, dq), 1) == dq`` for rotations below half a
    turn).  Free joint: translation added, rotation q exp(dq_rot / 2) with dq_rot in the body frame; ball joint: the rotation;
    hinge and slide joints: sums.  qpos (nq,) or (n, nq) with dq (nv,) or (n, nv); returns a new array."""
    a = engine.as_model(model).arrays
    q = np.array(qpos, np.float64); d = np.asarray(dq, np.float64)
    if q.shape[-1] != len(a['qpos0']) or d.shape[-1] != len(a['dof_bodyid']) or q.shape[:-1] != d.shape[:-1]:
        raise ValueError(f'qpos must be (..., {len(a["qpos0"])}) and dq (..., {len(a["dof_bodyid"])}) with equal leading shape, got {q.shape} and {d.shape}')
    for j, t in enumerate(a['jnt_type']):
        qa, da = int(a['jnt_qposadr'][j]), int(a['jnt_dofadr'][j])
        if t == _JNT_FREE:
            q[..., qa:qa + 3] += d[..., da:da + 3]
            q[..., qa + 3:qa + 7] = _quat_integrate(q[..., qa + 3:qa + 7], d[..., da + 3:da + 6])
        elif t == _JNT_BALL:
            q[..., qa:qa + 4] = _quat_integrate(q[..., qa:qa + 4], d[..., da:da + 3])
        else:
            q[..., qa] += d[..., da]
    return q


def tangent_names(model: Union['engine.Model', str]) -> List[str]:
    """Labels of the ndx = 2 nv + na tangent entries (rows and columns of A, rows of B, columns of C) followed by the nu controls (columns
    of B and D): 'dq:<joint>' (free joint: ':tx', ':ty', ':tz', ':rx', ':ry', ':rz'; ball joint: ':rx' ..), 'dv:<joint>...',
    'act:<actuator>' for the actuators that have an activation, 'ctrl:<actuator>'."""
    a = engine.as_model(model).arrays
    dof = [''] * len(a['dof_bodyid'])
    for j, t in enumerate(a['jnt_type']):
        name, d = str(a['names_jnt'][j]), int(a['jnt_dofadr'][j])
        if t == _JNT_FREE:
            for k, s in enumerate(('tx', 'ty', 'tz', 'rx', 'ry', 'rz')):
                dof[d + k] = f'{name}:{s}'
        elif t == _JNT_BALL:
            for k, s in enumerate(('rx', 'ry', 'rz')):
                dof[d + k] = f'{name}:{s}'
        else:
            dof[d] = name
    acts = [str(n) for n in a['names_actuator']]
    adr = np.asarray(a['actuator_actadr'])
    with_act = sorted((int(adr[i]), acts[i]) for i in range(len(acts)) if adr[i] >= 0)
    return ['dq:' + n for n in dof] + ['dv:' + n for n in dof] + ['act:' + n for _, n in with_act] + ['ctrl:' + n for n in acts]


def transition_fd(model_or_task_name: Union['engine.Model', str], qpos: np.ndarray, qvel: np.ndarray, act: Optional[np.ndarray] = None,
                  ctrl: Optional[np.ndarray] = None, eps: float = 1e-6, centered: bool = True, n_substeps: int = 1, sensors: bool = False,
                  device: int = 0, batch_size: int = 1024) -> TransitionFD:
    """Finite-difference Jacobians of n_substeps physics substeps (ctrl held) around the given states, as numpy:
    TransitionFD(A (ndx, ndx), B (ndx, nu), C (33, ndx) or None, D (33, nu) or None, status) for one frame -- qpos (nq,), qvel (nv,),
    act (na,) and ctrl (nu,), zeros when None -- or with a leading n_frames axis for (n_frames, ...) arrays.

    model_or_task_name: an engine.Model (FP64 engine library) or an asset name ('walk_imitation', 'flight_imitation', 'walk_on_ball').
    The states are set on a helper batch of at most `batch_size` environments on GPU `device`; a forward evaluation at the nominal state
    defines the warm start w of every perturbed constraint solve (its acceleration).  status: the OR of the engine's WARN bits
    (engine.WARN_BITS) over the frame's transitions -- non-zero means a cap or an iteration limit was hit and the frame's matrices are
    not derivatives."""
    model = engine.as_model(model_or_task_name)
    nq, nv, na, nu = (model.dim(k) for k in ('nq', 'nv', 'na', 'nu'))
    q = np.asarray(qpos, np.float64); v = np.asarray(qvel, np.float64)
    single = q.ndim == 1
    if single:
        q, v = q[None], v[None]
    nf = len(q)
    a_ = np.zeros((nf, na)) if act is None else np.asarray(act, np.float64).reshape(nf, -1)
    u = np.zeros((nf, nu)) if ctrl is None else np.asarray(ctrl, np.float64).reshape(nf, -1)
    if q.ndim != 2 or q.shape[1] != nq or v.shape != (nf, nv) or a_.shape != (nf, na) or u.shape != (nf, nu):
        raise ValueError(f'qpos must be ({nq},) or (n, {nq}); qvel ({nv},), act ({na},) and ctrl ({nu},) or (n, ...) with the same n')
    ndx = 2*nv + na
    A = np.empty((nf, ndx, ndx)); B = np.empty((nf, ndx, nu)); status = np.empty(nf, np.int32)
    Cs = np.empty((nf, engine.NSENSOR, ndx)) if sensors else None
    Ds = np.empty((nf, engine.NSENSOR, nu)) if sensors else None
    for batch, lo, hi in engine.helper_batches(model, nf, batch_size, device):
        batch.set('QPOS', q[lo:hi]); batch.set('QVEL', v[lo:hi]); batch.set('CTRL', u[lo:hi])
        if na:
            batch.set('ACT', a_[lo:hi])
        batch.forward()
        r = batch.transition_fd(eps=eps, centered=centered, n_substeps=n_substeps, sensors=sensors)
        batch.synchronize()
        A[lo:hi] = r.A.cpu().numpy(); B[lo:hi] = r.B.cpu().numpy(); status[lo:hi] = r.status.cpu().numpy()
        if sensors:
            Cs[lo:hi] = r.C.cpu().numpy(); Ds[lo:hi] = r.D.cpu().numpy()
    if single:
        return TransitionFD(A[0], B[0], None if Cs is None else Cs[0], None if Ds is None else Ds[0], int(status[0]))
    return TransitionFD(A, B, Cs, Ds, status)
