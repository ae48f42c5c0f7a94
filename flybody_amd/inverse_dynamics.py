"""Batched inverse dynamics on the GPU: MuJoCo's ``mj_inverse`` for the fly model, one frame per wavefront.

The question after inverse kinematics (``inverse_kinematics.qpos_from_site_xpos`` turns keypoints into ``qpos`` trajectories) is which
forces produce that motion: joint torques, ground-reaction forces at the claws and the residual wrench on the unactuated root.  Every
frame is one environment of an FP64 batch (fb_batch_inverse, csrc/fb_inverse.hpp); thousands run at once.  Noslip is not inverted
(neither does mj_inverse): on a model with ``opt_noslip_iterations > 0`` -- the shipped assets set 3 -- the inverse of a forward pass's
acceleration differs from its ``qfrc_actuator`` by what the noslip passes changed.  FP64 only; there is no CPU path: without a GPU the
batch cannot be created and this raises.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional, Union

import numpy as np

from . import engine

InverseResult = namedtuple('InverseResult', ['qfrc_inverse', 'qfrc_constraint', 'contact_force', 'contact_pos', 'contact_normal',
                                             'contact_geoms', 'ncon', 'root_residual'])
TrajectoryInverseResult = namedtuple('TrajectoryInverseResult', ['frames', 'qvel', 'qacc', 'joint_torques', 'result'])

_JNT_FREE, _JNT_BALL = 0, 1               # (mjJNT_*; derivatives.py imports them and _quat_mul)


def _quat_mul(a, b):
    w1, x1, y1, z1 = np.moveaxis(a, -1, 0)
    w2, x2, y2, z2 = np.moveaxis(b, -1, 0)
    return np.stack([w1*w2 - x1*x2 - y1*y2 - z1*z2, w1*x2 + x1*w2 + y1*z2 - z1*y2,
                     w1*y2 - x1*z2 + y1*w2 + z1*x2, w1*z2 + x1*y2 - y1*x2 + z1*w2], axis=-1)


def _quat_diff(qa, qb, dt):
    """Angular velocity w (local frame of qa) with qa exp(w dt / 2) = qb: mju_subQuat / mju_quat2Vel, angle wrapped to [-pi, pi]."""
    qa = qa / np.linalg.norm(qa, axis=-1, keepdims=True); qb = qb / np.linalg.norm(qb, axis=-1, keepdims=True)
    d = _quat_mul(qa*np.array([1.0, -1.0, -1.0, -1.0]), qb)
    axis = d[..., 1:]
    s = np.linalg.norm(axis, axis=-1, keepdims=True)
    angle = 2*np.arctan2(s, d[..., :1])
    angle = np.where(angle > np.pi, angle - 2*np.pi, angle)
    return np.where(s > 0, axis/np.where(s > 0, s, 1.0), 0.0)*angle/dt


def differentiate_pos(model: Union['engine.Model', str], qa: np.ndarray, qb: np.ndarray, dt: float) -> np.ndarray:
    """mj_differentiatePos: the velocity that takes qa to qb in time dt, the exact inverse of the engine's position integration
    (semi-implicit Euler: qpos <- integratePos(qpos, qvel_new, h)).  Free joint: world-frame linear velocity and the body-frame angular
    velocity log(qa^-1 qb) / dt; ball joint: the angular part; hinge and slide joints: differences.  qa, qb: (nq,) or (n, nq)."""
    a = engine.as_model(model).arrays
    qa = np.asarray(qa, np.float64); qb = np.asarray(qb, np.float64)
    if qa.shape != qb.shape or qa.shape[-1] != len(a['qpos0']):
        raise ValueError(f'qa and qb must both be (..., {len(a["qpos0"])}), got {qa.shape} and {qb.shape}')
    v = np.zeros(qa.shape[:-1] + (len(a['dof_bodyid']),))
    for j, t in enumerate(a['jnt_type']):
        q, d = int(a['jnt_qposadr'][j]), int(a['jnt_dofadr'][j])
        if t == _JNT_FREE:
            v[..., d:d + 3] = (qb[..., q:q + 3] - qa[..., q:q + 3])/dt
            v[..., d + 3:d + 6] = _quat_diff(qa[..., q + 3:q + 7], qb[..., q + 3:q + 7], dt)
        elif t == _JNT_BALL:
            v[..., d:d + 3] = _quat_diff(qa[..., q:q + 4], qb[..., q:q + 4], dt)
        else:
            v[..., d] = (qb[..., q] - qa[..., q])/dt
    return v


def inverse_dynamics(model: Union['engine.Model', str], qpos: np.ndarray, qvel: np.ndarray, qacc: np.ndarray, discrete: bool = False,
                     device: int = 0, batch_size: int = 8192) -> InverseResult:
    """Generalised forces that give the state (qpos, qvel) the acceleration qacc (mj_inverse):
        qfrc_inverse = M qacc + qfrc_bias - qfrc_passive - qfrc_constraint,  qfrc_constraint = J' f(J qacc - aref).
    discrete: qacc is (qvel+ - qvel) / h of one Euler step of the model's timestep h (mjENBL_INVDISCRETE).

    model: an engine.Model (FP64 engine library) or an asset name ('walk_imitation', 'flight_imitation', 'walk_on_ball').
    qpos (nq,), qvel / qacc (nv,): one frame, per-frame results without the frame axis; or (n_frames, ...) arrays.  Frames go through
    batches of at most `batch_size` environments on GPU `device`.
    Returns InverseResult: qfrc_inverse, qfrc_constraint (n, nv); contact_force (n, 64, 3) in each contact's frame (normal, tangent 1,
    tangent 2); contact_pos (n, 64, 3), contact_normal (n, 64, 3), contact_geoms (n, 64, 2) geom ids (-1 beyond ncon); ncon (n,);
    root_residual (n, 6) = qfrc_inverse[:, :6] for a model whose first joint is free (the wrench nothing actuates), else None."""
    model = engine.as_model(model)
    a = model.arrays
    nq, nv = len(a['qpos0']), len(a['dof_bodyid'])
    q = np.asarray(qpos, np.float64); v = np.asarray(qvel, np.float64); acc = np.asarray(qacc, np.float64)
    single = q.ndim == 1
    if single:
        q, v, acc = q[None], v[None], acc[None]
    if q.ndim != 2 or q.shape[1] != nq or v.shape != (len(q), nv) or acc.shape != (len(q), nv):
        raise ValueError(f'qpos must be ({nq},) or (n, {nq}); qvel and qacc ({nv},) or (n, {nv}) with the same n')
    nf = len(q)
    qi = np.empty((nf, nv)); qc = np.empty((nf, nv)); cf = np.empty((nf, engine.MAXCON, 3)); con = np.empty((nf, engine.MAXCON, 8))
    ncon = np.empty(nf, np.int32)
    for batch, lo, hi in engine.helper_batches(model, nf, batch_size, device):
        batch.set('QPOS', q[lo:hi]); batch.set('QVEL', v[lo:hi]); batch.set('QACC', acc[lo:hi])
        batch.inverse(discrete=discrete)
        qi[lo:hi] = batch.get('QFRC_INVERSE'); qc[lo:hi] = batch.get('QFRC_CONSTRAINT')
        cf[lo:hi] = batch.get('CONTACT_FORCE').reshape(-1, engine.MAXCON, 3)
        con[lo:hi] = batch.get('CONTACT').reshape(-1, engine.MAXCON, 8); ncon[lo:hi] = batch.get('NCON')[:, 0]
    live = np.arange(engine.MAXCON)[None, :] < ncon[:, None]
    pair = np.where(live, con[..., 7], 0).astype(np.int64)
    geoms = np.where(live[..., None], np.stack([a['pair_geom1'][pair], a['pair_geom2'][pair]], axis=-1), -1)
    pos = np.where(live[..., None], con[..., 1:4], 0.0); normal = np.where(live[..., None], con[..., 4:7], 0.0)
    root = qi[:, :6].copy() if len(a['jnt_type']) and int(a['jnt_type'][0]) == _JNT_FREE else None
    res = InverseResult(qi, qc, cf, pos, normal, geoms.astype(np.int32), ncon, root)
    if single:
        return InverseResult(*(None if x is None else x[0] for x in res))
    return res


def trajectory_inverse_dynamics(model: Union['engine.Model', str], qpos_traj: np.ndarray, dt: float, device: int = 0,
                                batch_size: int = 8192) -> TrajectoryInverseResult:
    """Inverse dynamics along a qpos trajectory (n_frames, nq) sampled every dt -- e.g. qpos_from_site_xpos output -- in the convention
    that inverts the engine's Euler substep:
        qvel_t = differentiate_pos(q_{t-1}, q_t) / dt,   qacc_t = (qvel_{t+1} - qvel_t) / dt,   discrete = True.
    Frames 1 .. T-2 have both (frames 0 and T-1 lack a neighbour): T-2 results.  With dt = the model's timestep and q the engine's own
    substeps this recovers each substep's applied force exactly up to rounding; at another dt the differences are a first-order
    approximation (the discrete conversion always uses the model's timestep).
    Returns TrajectoryInverseResult: frames (the frame indices), qvel, qacc, joint_torques {joint name: qfrc_inverse of the joint's
    dofs, (n,) for one-dof joints, (n, k) otherwise} and the InverseResult of those frames."""
    model = engine.as_model(model)
    a = model.arrays
    q = np.asarray(qpos_traj, np.float64)
    if q.ndim != 2 or q.shape[1] != len(a['qpos0']) or len(q) < 3:
        raise ValueError(f'qpos_traj must be (n_frames >= 3, {len(a["qpos0"])}), got {q.shape}')
    if not dt > 0:
        raise ValueError('dt must be > 0')
    vel = differentiate_pos(model, q[:-1], q[1:], dt)          # vel[k] = qvel of frame k + 1
    acc = (vel[1:] - vel[:-1])/dt                              # acc[k] = qacc of frame k + 1
    frames = np.arange(1, len(q) - 1)
    res = inverse_dynamics(model, q[1:-1], vel[:-1], acc, discrete=True, device=device, batch_size=batch_size)
    torques = {}
    for j, name in enumerate(a['names_jnt']):
        t, d = int(a['jnt_type'][j]), int(a['jnt_dofadr'][j])
        k = 6 if t == _JNT_FREE else (3 if t == _JNT_BALL else 1)
        torques[str(name)] = res.qfrc_inverse[:, d] if k == 1 else res.qfrc_inverse[:, d:d + k]
    return TrajectoryInverseResult(frames, vel[:-1], acc, torques, res)
