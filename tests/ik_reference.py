"""FP64 line-by-line restatement of the reference's qpos_from_site_xpos (flybody/inverse_kinematics.py) on the CPU oracle -- the checker
of fb_batch_ik.  mj_fwdPosition is the oracle's kinematics + com_pos (all the IK reads of it), mj_jacSite is OracleData.jac at the site
position on the site's body, mj_integratePos is restated in numpy below (MuJoCo's mju_quatIntegrate for the free / ball joints).
Test infrastructure only; imports oracle.fbo and nothing of the package's kernels."""
from __future__ import annotations

import numpy as np

MINVAL = 1e-15
JNT_FREE, JNT_BALL, JNT_HINGE = 0, 1, 3


def _mulquat(a, b):
    return np.array([a[0]*b[0] - a[1]*b[1] - a[2]*b[2] - a[3]*b[3],
                     a[0]*b[1] + a[1]*b[0] + a[2]*b[3] - a[3]*b[2],
                     a[0]*b[2] - a[1]*b[3] + a[2]*b[0] + a[3]*b[1],
                     a[0]*b[3] + a[1]*b[2] - a[2]*b[1] + a[3]*b[0]])


def quat_integrate(quat, vel):
    """mju_quatIntegrate(quat, vel, 1): normalize3 / axisAngle2Quat / normalize4 with MuJoCo's mjMINVAL branches."""
    ax = np.array(vel, float)
    angle = np.sqrt(ax @ ax)
    ax = np.array([1.0, 0, 0]) if angle < MINVAL else ax * (1.0 / angle)
    qrot = np.array([1.0, 0, 0, 0]) if angle == 0 else np.concatenate([[np.cos(0.5*angle)], ax*np.sin(0.5*angle)])
    q = np.array(quat, float)
    n = np.sqrt(q @ q)
    if n < MINVAL:
        q = np.array([1.0, 0, 0, 0])
    elif abs(n - 1) > MINVAL:
        q = q * (1.0 / n)
    return _mulquat(q, qrot)


def integrate_pos(arrays, qpos, v):
    """mj_integratePos(m, qpos, v, 1) in place."""
    for j in range(len(arrays['jnt_type'])):
        t, qa, da = int(arrays['jnt_type'][j]), int(arrays['jnt_qposadr'][j]), int(arrays['jnt_dofadr'][j])
        if t == JNT_FREE:
            qpos[qa:qa + 3] += v[da:da + 3]
            qpos[qa + 3:qa + 7] = quat_integrate(qpos[qa + 3:qa + 7], v[da + 3:da + 6])
        elif t == JNT_BALL:
            qpos[qa:qa + 4] = quat_integrate(qpos[qa:qa + 4], v[da:da + 3])
        else:
            qpos[qa] += v[da]


def joint_dofs(arrays, joint_ids):
    out = []
    for j in joint_ids:
        t = int(arrays['jnt_type'][j]); n = 6 if t == JNT_FREE else (3 if t == JNT_BALL else 1)
        out += [int(arrays['jnt_dofadr'][j]) + k for k in range(n)]
    return out


def qpos_from_site_xpos(od, arrays, site_ids, target_xpos, joint_ids, reg_strength=0.0, lr=0.01, beta=0.99, progress_threshold=0.01,
                        max_steps=20_000, include=None):
    """od: oracle.fbo.OracleData whose qpos is the start (modified in place, the reference's inplace=True); ids instead of names;
    include: [3 n_site] 0 / 1 mask (the reference's include_inds).  Returns (qpos, err_norm, err_norm_first_term, steps, success)."""
    site_ids = [int(s) for s in site_ids]; joint_ids = [int(j) for j in joint_ids]
    target_xpos = np.asarray(target_xpos, float)
    include_inds = slice(None) if include is None else np.flatnonzero(np.asarray(include))
    nv = len(arrays['dof_bodyid'])
    site_body = [int(arrays['site_bodyid'][s]) for s in site_ids]
    qpos = od.field('qpos')

    def fwd_position():
        od.call('kinematics'); od.call('com_pos')

    def sxpos():
        return od.field('site_xpos').reshape(-1, 3)[site_ids].copy()

    nv_update = np.zeros(nv)
    dof_indices = joint_dofs(arrays, joint_ids)
    fwd_position()
    hinge_joints = [j for j in joint_ids if int(arrays['jnt_type'][j]) == JNT_HINGE]
    hinge_qadr = [int(arrays['jnt_qposadr'][j]) for j in hinge_joints]
    hinge_dof_indices = [int(arrays['jnt_dofadr'][j]) for j in hinge_joints]

    def objective(site_xpos, reg):
        hinge_qpos = qpos[hinge_qadr]
        diff = (np.array(site_xpos) - np.array(target_xpos)).flatten()[include_inds]
        err_pos = np.linalg.norm(diff)**2
        err_pos += reg * np.linalg.norm(hinge_qpos)**2
        return err_pos

    def gradient(site_xpos):
        jac_full = np.empty((3*target_xpos.shape[0], nv))
        for i, (s, b) in enumerate(zip(site_xpos, site_body)):
            jac_full[3*i:3*i + 3, :] = od.jac(s, b)[0]
        jac_partial = jac_full[:, dof_indices]
        hinge_qpos = np.zeros(nv)
        hinge_qpos[hinge_dof_indices] = qpos[hinge_qadr]
        hinge_qpos = hinge_qpos[dof_indices]
        grad = 2 * np.matmul((site_xpos - target_xpos).flatten()[include_inds], jac_partial[include_inds, :])
        grad += 2 * reg_strength * hinge_qpos
        return grad

    success = False
    update = 0.
    for step in range(max_steps):
        site_xpos = sxpos()
        grad = gradient(site_xpos)
        update = beta * update + grad
        nv_update[dof_indices] = -lr * update
        integrate_pos(arrays, qpos, nv_update)
        fwd_position()
        if step % 100 == 0:
            site_xpos = sxpos()
            err = objective(site_xpos, reg_strength)
            with np.errstate(divide='ignore', invalid='ignore'):
                progress_criterion = lr * np.linalg.norm(update) / err
            if progress_criterion < progress_threshold:
                success = True
                break
    err_first_term = objective(site_xpos, 0)
    return qpos.copy(), err, err_first_term, step, success
