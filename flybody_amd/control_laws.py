"""Substep control laws: per-dof feedback that the step kernel evaluates in every physics substep (csrc/fb_law.hpp),

    u[i] = bias[i] + act_gain[i]*qfrc_actuator[i] - pos_gain[i]*(qpos[hinge of dof i] - pos_ref[i]) - vel_gain[i]*qvel[i]

added to the generalised forces next to qfrc_applied.  It is what a MuJoCo `mjcb_control` callback does when it writes qfrc_applied
from the state, for laws that are diagonal in the dofs: reflex springs and dampers, motor noise, assistive torques.  qfrc_actuator is
the actuator force of the SAME substep (MuJoCo's callback sees the previous substep's), so `motor_scale(model, g)` means exactly "every
motor is (1 + g) times as strong".

`ControlLaw` is a plain container of the five rows; `BatchedFlyEnv.set_control_law(law)` / `engine.Batch.set_control_law(**law.rows())`
hand it to the engine.  `model` below is an engine.Model (or anything with `.arrays`, the compiled tables).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

ROWS = ('bias', 'act_gain', 'pos_gain', 'pos_ref', 'vel_gain')
_JNT_HINGE = 3


class ControlLaw:
    """Five rows [nv] (one law for every environment) or [n_env, nv] (one per environment); a row left out is zeros."""

    def __init__(self, nv: int, bias=None, act_gain=None, pos_gain=None, pos_ref=None, vel_gain=None, n_env: Optional[int] = None):
        self.nv = int(nv)
        shape = (self.nv,) if n_env is None else (int(n_env), self.nv)
        for name, v in zip(ROWS, (bias, act_gain, pos_gain, pos_ref, vel_gain)):
            row = np.zeros(shape)
            if v is not None:
                row[...] = np.asarray(v, np.float64)
            setattr(self, name, row)

    @classmethod
    def from_dofs(cls, model, dof_ids, bias=0.0, act_gain=0.0, pos_gain=0.0, pos_ref=0.0, vel_gain=0.0) -> 'ControlLaw':
        """A law that acts on `dof_ids` only; every value is a scalar or one entry per listed dof."""
        nv = len(model.arrays['dof_jntid'])
        ids = np.asarray(dof_ids, np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= nv):
            raise IndexError(f'dof id outside [0, {nv})')
        law = cls(nv)
        for name, v in zip(ROWS, (bias, act_gain, pos_gain, pos_ref, vel_gain)):
            getattr(law, name)[ids] = np.asarray(v, np.float64)
        return law

    def rows(self) -> Dict[str, np.ndarray]:
        return {k: getattr(self, k) for k in ROWS}

    def __add__(self, other: 'ControlLaw') -> 'ControlLaw':
        """Two laws acting together.  The sum of two position terms with different references is one term again:
        gains add, the reference is their gain-weighted mean."""
        if self.nv != other.nv:
            raise ValueError('laws of different models')
        out = ControlLaw(self.nv)
        for k in ('bias', 'act_gain', 'vel_gain', 'pos_gain'):
            setattr(out, k, getattr(self, k) + getattr(other, k))
        kr = self.pos_gain*self.pos_ref + other.pos_gain*other.pos_ref
        out.pos_ref = np.divide(kr, out.pos_gain, out=np.zeros_like(kr), where=out.pos_gain != 0)
        return out


def hinge_dofs(model, joint_names: Sequence[str]) -> np.ndarray:
    """Dof ids of the named hinge joints (the compiled model's `names_jnt`)."""
    a = model.arrays
    table = {str(n): j for j, n in enumerate(a['names_jnt'])}
    missing = [n for n in joint_names if n not in table]
    if missing:
        raise KeyError(f'unknown joints {missing}')
    jid = np.array([table[n] for n in joint_names], np.int64)
    bad = [n for n, j in zip(joint_names, jid) if int(a['jnt_type'][j]) != _JNT_HINGE]
    if bad:
        raise ValueError(f'{bad} are not hinge joints: position and velocity feedback is per hinge dof')
    return np.asarray(a['jnt_dofadr'])[jid].astype(np.int64)


def motor_scale(model, g) -> ControlLaw:
    """Every actuator force scaled by 1 + g in the substep it acts in (g: a scalar or [nv]): motor noise, weakness, fatigue."""
    nv = len(model.arrays['dof_jntid'])
    return ControlLaw(nv, act_gain=np.broadcast_to(np.asarray(g, np.float64), (nv,)))


def joint_spring(model, joint_names: Sequence[str], k, ref=None) -> ControlLaw:
    """A spring of stiffness k on the named hinges, pulling towards `ref` (default: the model's qpos_spring of the joint)."""
    dofs = hinge_dofs(model, joint_names)
    a = model.arrays
    if ref is None:
        table = {str(n): j for j, n in enumerate(a['names_jnt'])}
        ref = np.asarray(a['qpos_spring'])[np.asarray(a['jnt_qposadr'])[[table[n] for n in joint_names]]]
    return ControlLaw.from_dofs(model, dofs, pos_gain=k, pos_ref=ref)


def joint_damper(model, joint_names: Sequence[str], d) -> ControlLaw:
    """A damper of coefficient d on the named hinges."""
    return ControlLaw.from_dofs(model, hinge_dofs(model, joint_names), vel_gain=d)
