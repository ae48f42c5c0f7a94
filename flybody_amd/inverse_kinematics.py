"""Multi-site inverse kinematics on the GPU: the reference's ``flybody/inverse_kinematics.py`` ``qpos_from_site_xpos``, batched.

Fits joint angles so that model sites (tarsi, claws, thorax, head) match target positions -- what turns motion-capture keypoints into
the ``qpos`` reference trajectories walk_imitation / flight_imitation imitate.  The reference fits one frame at a time with up to 20 000
Python-driven iterations; here every frame is one GPU wavefront (fb_batch_ik, csrc/fb_ik.hpp) and thousands run at once.  Same
algorithm, hyper-parameters and result fields (see fb_ik.hpp for the reference semantics kept on purpose).  FP64 only; there is no CPU
path: without a GPU the batch cannot be created and this raises.
"""
from __future__ import annotations

from collections import namedtuple
from typing import List, Optional, Sequence, Union

import numpy as np

from . import engine

IKResult = namedtuple('IKResult', ['qpos', 'err_norm', 'err_norm_first_term', 'steps', 'success'])


def _ids(names: Sequence[str], table, kind: str) -> np.ndarray:
    if isinstance(names, str):
        names = [names]
    table = [str(n) for n in table]
    out = []
    for n in names:
        if n not in table:
            raise ValueError(f'unknown {kind} name {n!r}')
        out.append(table.index(n))
    if len(set(out)) != len(out):
        raise ValueError(f'duplicate {kind} names in {list(names)!r}')
    return np.asarray(out, np.int32)


def _include_mask(include_inds, n: int) -> np.ndarray:
    """The reference's include_inds (indices into the flattened [n_sites, 3] target, or a slice) as a 0 / 1 mask of length n."""
    idx = np.arange(n)[include_inds]
    if len(np.unique(idx)) != len(idx):
        raise ValueError('include_inds selects a component more than once')
    mask = np.zeros(n, np.int32)
    mask[idx] = 1
    return mask


def qpos_from_site_xpos(model: Union['engine.Model', str], site_names: Sequence[str], target_xpos: np.ndarray, joint_names: Sequence[str],
                        reg_strength: float = 0.0, lr: float = 0.01, beta: float = 0.99, progress_threshold: float = 0.01,
                        max_steps: int = 20_000, include_inds: Union[slice, List[int]] = slice(None), qpos_init: Optional[np.ndarray] = None,
                        device: int = 0, batch_size: int = 8192) -> IKResult:
    """Joint angles qpos such that the sites `site_names` match `target_xpos`, by momentum gradient descent on
    |s(q) - s*|^2 + reg_strength |q_hinge|^2 over the dofs of `joint_names` (the reference's qpos_from_site_xpos).

    model: an engine.Model (FP64 engine library) or an asset name ('walk_imitation', 'flight_imitation', 'walk_on_ball').
    target_xpos: (n_sites, 3) -- one frame, scalar results like the reference -- or (n_frames, n_sites, 3): every frame fitted
    independently, per-frame result arrays.  qpos_init: starting pose, (nq,) or (n_frames, nq); default the model's qpos0.
    Frames go through batches of at most `batch_size` environments on GPU `device`.
    Returns IKResult(qpos, err_norm, err_norm_first_term, steps, success)."""
    model = engine.as_model(model)
    a = model.arrays
    sites = _ids(site_names, a['names_site'], 'site')
    joints = _ids(joint_names, a['names_jnt'], 'joint')
    t = np.asarray(target_xpos, np.float64)
    single = t.ndim == 2
    if single:
        t = t[None]
    if t.ndim != 3 or t.shape[1:] != (len(sites), 3):
        raise ValueError(f'target_xpos must be ({len(sites)}, 3) or (n_frames, {len(sites)}, 3), got {np.shape(target_xpos)}')
    nf, nq = t.shape[0], len(a['qpos0'])
    q0 = a['qpos0'] if qpos_init is None else np.asarray(qpos_init, np.float64)
    if q0.shape not in ((nq,), (nf, nq)):
        raise ValueError(f'qpos_init must be ({nq},) or ({nf}, {nq})')
    q0 = np.broadcast_to(q0, (nf, nq))
    mask = _include_mask(include_inds, 3*len(sites))
    qpos = np.empty((nf, nq)); err = np.empty((nf, 2)); steps = np.empty((nf, 2), np.int32)
    for batch, lo, hi in engine.helper_batches(model, nf, batch_size, device):
        batch.set('QPOS', q0[lo:hi])
        batch.ik(sites, joints, t[lo:hi], include=mask, reg_strength=reg_strength, lr=lr, beta=beta,
                 progress_threshold=progress_threshold, max_steps=max_steps)
        qpos[lo:hi] = batch.get('QPOS'); err[lo:hi] = batch.get('IK_ERR'); steps[lo:hi] = batch.get('IK_STEPS')
    res = IKResult(qpos=qpos, err_norm=err[:, 0], err_norm_first_term=err[:, 1], steps=steps[:, 0], success=steps[:, 1].astype(bool))
    if single:
        return IKResult(qpos=res.qpos[0], err_norm=float(res.err_norm[0]), err_norm_first_term=float(res.err_norm_first_term[0]),
                        steps=int(res.steps[0]), success=bool(res.success[0]))
    return res
