"""External forces on a batch of flies: pushes, gusts, loads and assistive torques through the engine's applied-force inputs
(FB_QFRC_APPLIED / FB_XFRC_APPLIED, MuJoCo's qfrc_applied / xfrc_applied; include/flybody_engine.h).

The arrays are inputs like the actions: what is set here acts on every physics substep of every following control step until it is
changed; an auto-reset does not clear it.  `env` is a fly_envs.BatchedFlyEnv.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np


def body_ids(model, names: Sequence[str]) -> np.ndarray:
    """Body ids of the named bodies of an engine.Model (the compiled model's `names_body`)."""
    table = {str(n): i for i, n in enumerate(model.arrays['names_body'])}
    missing = [n for n in names if n not in table]
    if missing:
        raise KeyError(f'unknown bodies {missing}')
    return np.array([table[n] for n in names], np.int64)


def set_body_wrench(env, bodies, force, torque=None, env_ids=None) -> None:
    """xfrc_applied[env_ids, bodies] = [force, torque]: a world-frame force (and torque, default 0) at the centre of mass of every
    listed body (ids, or names resolved with body_ids), for the listed environments (default: all).  force / torque broadcast
    against [len(env_ids), len(bodies), 3]; torch tensors on the env's device are used without a host copy."""
    import torch
    x = env.applied_forces()['xfrc_applied']
    if len(bodies) and isinstance(bodies[0], str):
        bodies = body_ids(env.model, bodies)
    b = torch.as_tensor(np.asarray(bodies, np.int64), device=x.device)
    if len(b) and (int(b.min()) < 0 or int(b.max()) >= x.shape[1]):
        raise IndexError('body id out of range')
    e = torch.arange(env.n_env, device=x.device) if env_ids is None else torch.as_tensor(np.asarray(env_ids, np.int64), device=x.device)
    shape = (len(e), len(b), 3)
    f = torch.as_tensor(force, dtype=x.dtype, device=x.device).expand(shape)
    t = torch.zeros(shape, dtype=x.dtype, device=x.device) if torque is None else torch.as_tensor(torque, dtype=x.dtype, device=x.device).expand(shape)
    if not (bool(torch.isfinite(f).all()) and bool(torch.isfinite(t).all())):
        raise ValueError('force and torque must be finite')
    x[e[:, None], b[None, :]] = torch.cat([f, t], dim=-1)


def clear(env) -> None:
    """Remove every applied force: frees the arrays and returns the batch to the plain step kernel."""
    env.clear_forces()
