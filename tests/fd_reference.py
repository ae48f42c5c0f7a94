"""The finite-difference recipe of fb_batch_transition_fd (MuJoCo's mjd_transitionFD for the engine's step), once, on the CPU oracle:
numpy with its own quaternion integrate / difference (ball joint included).  Test helper, not a test."""
import numpy as np

JNT_FREE, JNT_BALL = 0, 1
NSENS = 33


def _qmul(a, b):
    return np.array([a[0]*b[0] - a[1]*b[1] - a[2]*b[2] - a[3]*b[3], a[0]*b[1] + a[1]*b[0] + a[2]*b[3] - a[3]*b[2],
                     a[0]*b[2] - a[1]*b[3] + a[2]*b[0] + a[3]*b[1], a[0]*b[3] + a[1]*b[2] - a[2]*b[1] + a[3]*b[0]])


def quat_integrate(q, w):
    q = q / np.linalg.norm(q)
    ang = np.linalg.norm(w)
    if ang == 0:
        return q
    r = _qmul(q, np.r_[np.cos(0.5*ang), np.sin(0.5*ang)*w/ang])
    return r / np.linalg.norm(r)


def quat_sub(qb, qa):
    """Local rotation vector from qa to qb (mju_subQuat)."""
    d = _qmul(qa*np.array([1.0, -1, -1, -1]), qb)
    s = np.linalg.norm(d[1:])
    ang = 2*np.arctan2(s, d[0])
    if ang > np.pi:
        ang -= 2*np.pi
    return d[1:]*(ang/s) if s > 0 else np.zeros(3)


def integrate_pos(a, qpos, dq):
    q = np.array(qpos, float)
    for j, t in enumerate(a['jnt_type']):
        qa, da = int(a['jnt_qposadr'][j]), int(a['jnt_dofadr'][j])
        if t == JNT_FREE:
            q[qa:qa + 3] += dq[da:da + 3]; q[qa + 3:qa + 7] = quat_integrate(q[qa + 3:qa + 7], dq[da + 3:da + 6])
        elif t == JNT_BALL:
            q[qa:qa + 4] = quat_integrate(q[qa:qa + 4], dq[da:da + 3])
        else:
            q[qa] += dq[da]
    return q


def differentiate_pos(a, qa_, qb_):
    """dq with integrate_pos(qa, dq) == qb."""
    v = np.zeros(len(a['dof_bodyid']))
    for j, t in enumerate(a['jnt_type']):
        q, d = int(a['jnt_qposadr'][j]), int(a['jnt_dofadr'][j])
        if t == JNT_FREE:
            v[d:d + 3] = qb_[q:q + 3] - qa_[q:q + 3]; v[d + 3:d + 6] = quat_sub(qb_[q + 3:q + 7], qa_[q + 3:q + 7])
        elif t == JNT_BALL:
            v[d:d + 3] = quat_sub(qb_[q:q + 4], qa_[q:q + 4])
        else:
            v[d] = qb_[q] - qa_[q]
    return v


class Frame:
    """A nominal state (qpos, qvel, act, ctrl) and the warm start w of its perturbed solves (None: the acceleration of a forward
    evaluation at the nominal state)."""

    def __init__(self, om, a, qpos, qvel, act=None, ctrl=None, w=None):
        from oracle import fbo
        self.om, self.a, self.od = om, a, fbo.OracleData(om)
        self.nq, self.nv, self.nu = len(a['qpos0']), len(a['dof_bodyid']), len(a['actuator_trntype'])
        self.na = int((np.asarray(a['actuator_actadr']) >= 0).sum())
        self.ndx = 2*self.nv + self.na
        self.qpos = np.array(qpos, float); self.qvel = np.array(qvel, float)
        self.act = np.zeros(self.na) if act is None else np.array(act, float)
        self.ctrl = np.zeros(self.nu) if ctrl is None else np.array(ctrl, float)
        if w is None:
            self._set(self.qpos, self.qvel, self.act, self.ctrl, np.zeros(self.nv))
            self.od.call('forward')
            w = self.od.field('qacc').copy()
        self.w = np.array(w, float)
        self.nefc = []                     # nefc of every solve of every transition run so far

    def _set(self, q, v, act, ctrl, w):
        od = self.od
        od.field('qpos')[:] = q; od.field('qvel')[:] = v; od.field('ctrl')[:] = ctrl; od.field('qacc_warmstart')[:] = w
        if self.na:
            od.field('act')[:] = act

    def transition(self, q, v, act, ctrl, n=1):
        """T_n: (qpos', qvel', act', sensordata) of n substeps from the given state, warm-started from w."""
        od = self.od
        self._set(q, v, act, ctrl, self.w)
        od.call('step1')
        for _ in range(n):
            self.nefc.append(int(od.scalar('nefc')))
            od.call('step')
        act_n = od.field('act')[:self.na].copy() if self.na else np.zeros(0)
        return od.field('qpos').copy(), od.field('qvel').copy(), act_n, od.field('sensordata')[:NSENS].copy()

    def perturbed(self, col, d, n=1):
        q, v, act, ctrl = self.qpos.copy(), self.qvel.copy(), self.act.copy(), self.ctrl.copy()
        nv, ndx = self.nv, self.ndx
        if col < nv:
            dq = np.zeros(nv); dq[col] = d
            q = integrate_pos(self.a, q, dq)
        elif col < 2*nv:
            v[col - nv] += d
        elif col < ndx:
            act[col - 2*nv] += d
        else:
            ctrl[col - ndx] += d
        return self.transition(q, v, act, ctrl, n)

    def nominal(self, n=1):
        return self.transition(self.qpos, self.qvel, self.act, self.ctrl, n)

    def diff(self, xa, xb, h):
        return np.r_[differentiate_pos(self.a, xa[0], xb[0]), xb[1] - xa[1], xb[2] - xa[2], xb[3] - xa[3]]/h

    def ctrl_sides(self, i, eps):
        """(forward nudge fits, backward nudge fits) by MuJoCo's rule."""
        if not self.a['actuator_ctrllimited'][i]:
            return True, True
        lo, hi = self.a['actuator_ctrlrange'][i]
        c = self.ctrl[i]
        inside = lo <= c <= hi
        return bool(inside and c + eps <= hi), bool(inside and c - eps >= lo)

    def column(self, col, eps, centered=True, n=1, nominal=None):
        """One column of [A; C] (col < ndx) or [B; D]: (ndx + 33,)."""
        fwd, back = (True, True) if col < self.ndx else self.ctrl_sides(col - self.ndx, eps)
        nom = (lambda: nominal if nominal is not None else self.nominal(n))
        if centered and fwd and back:
            return self.diff(self.perturbed(col, -eps, n), self.perturbed(col, eps, n), 2*eps)
        if fwd:
            return self.diff(nom(), self.perturbed(col, eps, n), eps)
        if back:
            return self.diff(self.perturbed(col, -eps, n), nom(), eps)
        return np.zeros(self.ndx + NSENS)

    def matrices(self, eps=1e-6, centered=True, n=1, cols=None):
        """(A, B, C, D) by the recipe; cols: only these columns (the others stay NaN)."""
        ndx, nu = self.ndx, self.nu
        full = np.full((ndx + NSENS, ndx + nu), np.nan)
        nom = self.nominal(n)
        for c in (range(ndx + nu) if cols is None else cols):
            full[:, c] = self.column(c, eps, centered, n, nom)
        return full[:ndx, :ndx], full[:ndx, ndx:], full[ndx:, :ndx], full[ndx:, ndx:]


def column_errors(got, ref):
    """max |got - ref| per column over the column's largest |ref| entry (columns that are zero in ref: absolute)."""
    got, ref = np.asarray(got), np.asarray(ref)
    scale = np.abs(ref).max(axis=0)
    return np.abs(got - ref).max(axis=0) / np.where(scale > 0, scale, 1.0)
