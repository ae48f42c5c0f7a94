"""An FP64 reference of the task layer (flybody_amd/csrc/fb_task.hpp) in plain numpy, for tests/test_task_layer.py.

It is written from the sources the kernel's comments cite -- flybody/tasks/rewards.py, walk_imitation.py:152-203, walk_on_ball.py:62-90,
flight_imitation.py:170-223, base.py:206-268, template_task.py, quaternions.py, task_utils.py:223-240, dm_control's rewards.tolerance and the
fruit fly's observables (fruitfly.py:595-684) -- and calls nothing of oracle/ or csrc/.  It is a function of what a batch exposes through
Batch.get (QPOS, QVEL, ACT, XPOS, XQUAT, SITE_XPOS, SUBTREE_COM, QACC, SENSORDATA, STEP_COUNT, TIME), of the model's arrays and of the
configured reference / dataset.  The quaternion functions and the DeepMimic factors are pinned to the reference project's own outputs
(tests/golden/reference_functions.npz) by tests/test_task_layer.py::test_reference_is_pinned_to_the_reference_project, so this is no third
restatement with nobody behind it.

Two step indices, as in the reference project: the observables index the trajectory with the task's step COUNTER (base.py:252, :264; also
walk / flight com_dist, which is the norm of ref_displacement[0]), the rewards and the trajectory end with round(time / control_timestep)
(walk_imitation.py:159, :184; flight_imitation.py:208).  In an episode that runs from its reset the two agree; the tests that set TIME
move the second alone.

What the kernel alone defines (no counterpart in the reference project, which draws from a numpy RandomState): which trajectory, and in
flight which start row, an environment's episode gets -- hash_uniform below restates that integer hash.
"""
import collections

import numpy as np

U32 = 2.0**-24
TERMINAL_LINVEL, TERMINAL_ANGVEL, TERMINAL_QACC, TERMINAL_HEIGHT = 50.0, 200.0, 1e14, 0.2      # flybody/tasks/constants.py
DEEPMIMIC_STD = collections.OrderedDict(com=0.078487, qvel=53.7801, root2site=0.0735, joint_quat=1.2247)      # rewards.py:101-108
FIRST, MID, LAST = 0, 1, 2
SENSOR_KEYS = ('accelerometer', 'force', 'gyro', 'touch', 'velocimeter')                      # means over the substeps (fruitfly.py:626-665)


# ------------------------------------------------------------------ quaternions.py
def mult_quat(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    a1, b1, c1, d1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    a2, b2, c2, d2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([a1*a2 - b1*b2 - c1*c2 - d1*d2, a1*b2 + b1*a2 + c1*d2 - d1*c2, a1*c2 - b1*d2 + c1*a2 + d1*b2,
                     a1*d2 + b1*c2 - c1*b2 + d1*a2], axis=-1)


def conj_quat(q):
    return np.asarray(q, float)*np.array([1.0, -1, -1, -1])


def reciprocal_quat(q):
    q = np.asarray(q, float)
    return conj_quat(q)/np.sum(q*q, axis=-1, keepdims=True)


def rotate_vec_with_quat(v, q):
    """q v q^-1: a rotation whatever the norm of q"""
    v = np.asarray(v, float); q = np.broadcast_to(np.asarray(q, float), v.shape[:-1] + (4,))
    va = np.concatenate([np.zeros(v.shape[:-1] + (1,)), v], axis=-1)
    return mult_quat(q, mult_quat(va, reciprocal_quat(q)))[..., 1:]


def get_egocentric_vec(root_xpos, site_xpos, root_quat):
    return rotate_vec_with_quat(np.asarray(site_xpos, float) - np.asarray(root_xpos, float), conj_quat(root_quat))


def get_dquat_local(q1, q2):
    return mult_quat(reciprocal_quat(q1), q2)


def quat_dist_short_arc(q1, q2):
    q1 = np.asarray(q1, float); q2 = np.asarray(q2, float)
    q1 = q1/np.linalg.norm(q1, axis=-1, keepdims=True); q2 = q2/np.linalg.norm(q2, axis=-1, keepdims=True)
    return np.arccos(np.minimum(1.0, 2*np.sum(q1*q2, axis=-1)**2 - 1))


def quat_z2vec(vec):
    vec = np.atleast_2d(np.asarray(vec, float))
    out = np.zeros((len(vec), 4))
    for k, v in enumerate(vec):
        if v[0] == 0 and v[1] == 0:
            out[k] = [0, 1, 0, 0] if v[2] < 0 else [1, 0, 0, 0]
            continue
        v = v/np.linalg.norm(v)
        axis = np.array([-v[1], v[0], 0.0]); axis /= np.linalg.norm(axis)
        ang = np.arccos(v[2])
        out[k, 0] = np.cos(ang/2); out[k, 1:] = np.sin(ang/2)*axis
    return out


def axis_angle_to_quat(axis, angle):
    axis = np.atleast_2d(np.asarray(axis, float)); angle = np.atleast_1d(np.asarray(angle, float))
    axis = axis/np.linalg.norm(axis, axis=-1, keepdims=True)
    return np.concatenate([np.cos(angle/2)[:, None], np.sin(angle/2)[:, None]*axis], axis=-1)


def joint_orientation_quat(xaxis, qpos):
    return mult_quat(axis_angle_to_quat(xaxis, qpos), quat_z2vec(xaxis))


def quat_to_mat(q):
    """MuJoCo's mju_quat2Mat: the frame of a body from its (unit) quaternion, rows = world components"""
    w, x, y, z = np.asarray(q, float)
    return np.array([[w*w + x*x - y*y - z*z, 2*(x*y - w*z), 2*(x*z + w*y)],
                     [2*(x*y + w*z), w*w - x*x + y*y - z*z, 2*(y*z - w*x)],
                     [2*(x*z - w*y), 2*(y*z + w*x), w*w - x*x - y*y + z*z]])


# ------------------------------------------------------------------ rewards
def tolerance_linear(x, margin):
    """dm_control rewards.tolerance(x, bounds=(0, 0), sigmoid='linear', margin=margin, value_at_margin=0)"""
    d = np.abs(np.asarray(x, float))/margin
    return np.where(d < 1, 1 - d, 0.0)


def compute_diffs(walker, reference):
    """rewards.py:9-34 with n = 2"""
    out = collections.OrderedDict()
    for k in walker:
        if 'quat' in k: out[k] = float(np.sum(quat_dist_short_arc(walker[k], reference[k])**2))
        else: out[k] = float(np.sum(np.abs(np.asarray(walker[k], float) - np.asarray(reference[k], float))**2))
    return out


def reward_factors_deep_mimic(walker, reference, weights=(20, 1, 1, 1)):
    """rewards.py:84-116 -> (factors [4], diffs)"""
    diffs = compute_diffs(walker, reference)
    return np.array([np.exp(-0.5/DEEPMIMIC_STD[k]**2*diffs[k]) for k in walker])*np.asarray(weights, float), diffs


# ------------------------------------------------------------------ which trajectory an episode gets (fb_task.hpp: hash_uniform, pick_trajectory)
def hash_uniform(seed, env, episode):
    m = 0xffffffff
    x = ((seed*0x9E3779B9) & m) ^ ((env*0x85EBCA6B) & m) ^ ((episode*0xC2B2AE35) & m)
    x ^= x >> 16; x = (x*0x7feb352d) & m; x ^= x >> 15; x = (x*0x846ca68b) & m; x ^= x >> 16
    return float(np.float32(x >> 8)*np.float32(1.0/16777216.0))


class Task:
    """A configured task.  kind: 'walk', 'walk_ds', 'flight', 'flight_ds', 'ball', 'template'.  arrays: the model's arrays (model_blob.load_npz).
    ref_qpos [T, 7] / ref_qvel [T, 6]: the inference-mode reference (flight: the ROOT track; template: the start pose).  ds: for walk_ds a
    trajectory_loaders.WalkingDataset with joint_ids / site_ids, for flight_ds (offsets, root_qpos, qvel)."""

    def __init__(self, kind, arrays, ref_qpos=None, ref_qvel=None, future_steps=0, terminal_com_dist=np.inf, time_limit=10.0, ds=None,
                 joint_ids=None, site_ids=None, select=None, seed=0, env_id_base=0, randomize_start_step=False):
        self.kind, self.a = kind, arrays
        self.ref_qpos = None if ref_qpos is None else np.asarray(ref_qpos, float); self.ref_qvel = None if ref_qvel is None else np.asarray(ref_qvel, float)
        self.future_steps, self.terminal_com_dist, self.time_limit = int(future_steps), float(terminal_com_dist), float(time_limit)
        self.ds, self.joint_ids, self.site_ids, self.seed, self.env_id_base, self.random_start = ds, joint_ids, site_ids, int(seed), int(env_id_base), bool(randomize_start_step)
        self.dt = float(arrays['opt_control_timestep']); self.h = float(arrays['opt_timestep'])
        self.dt_real = self.dt            # the control step as the physics holds it (an FP32 build: rounded); the clock's is the double
        self.nsubstep = int(np.floor(self.dt/self.h + 0.5))
        n_traj = 0 if ds is None else (ds.n_traj if kind == 'walk_ds' else len(ds[0]) - 1)
        self.select = np.arange(n_traj) if select is None else np.asarray(select)
        self.has_ref = kind in ('walk', 'walk_ds', 'flight', 'flight_ds')
        self.nf = self.future_steps + 1 if self.has_ref else 0
        self.thorax = int(arrays['site_bodyid'][int(arrays['sensor_site_thorax'])])

    def clock_step(self, time):
        return int(np.round(time/self.dt))

    def episode(self, env, episode):
        """The reference track of episode number `episode` (0 for the first after the batch was made) of environment `env`:
        dict(q [T, 7] root track, v [T, 6], episode_steps, row0: the dataset row of its first frame, shift: what the loader took off x / y)."""
        max_steps = int(np.round(self.time_limit/self.dt)) + 1
        if self.kind in ('walk', 'template'):
            T = len(self.ref_qpos)
            return dict(q=self.ref_qpos, v=self.ref_qvel, episode_steps=min(max_steps, T - self.future_steps - 1), row0=0, shift=np.zeros(2))
        if self.kind == 'flight':                                             # flight_imitation.py:97-102
            T = len(self.ref_qpos)
            return dict(q=self.ref_qpos, v=self.ref_qvel, episode_steps=min(T, max_steps - 1) - (self.future_steps + 1), row0=0, shift=np.zeros(2))
        if self.kind == 'ball':
            return dict(q=None, v=None, episode_steps=0, row0=0, shift=np.zeros(2))
        u = hash_uniform(self.seed, self.env_id_base + env, episode)
        k = min(int(u*len(self.select)), len(self.select) - 1)
        traj = int(self.select[k])
        if self.kind == 'walk_ds':                                            # walk_imitation.py:92-105, trajectory_loaders.py:249
            off, end = int(self.ds.offsets[traj]), int(self.ds.offsets[traj + 1])
            q = np.array(self.ds.qpos[off:end, :7], float); v = np.array(self.ds.qvel[off:end, :6], float)
            shift = q[0, :2].copy(); q[:, :2] -= shift
            return dict(q=q, v=v, episode_steps=min(max_steps, (end - off) - self.future_steps - 1), row0=off, shift=shift)
        offsets, root, vel = self.ds                                          # flight_ds: trajectory_loaders.py:110-141
        off, end = int(offsets[traj]), int(offsets[traj + 1]); start = 0
        if self.random_start:
            u2 = hash_uniform(self.seed ^ 0x5bd1e995, self.env_id_base + env, episode)
            start = max(0, min(int(u2*(end - off - 50)), end - off - 51))
        q = np.array(root[off + start:end], float); v = np.array(vel[off + start:end], float)
        # the loader re-centres the CoM track before the task turns it into the root's (task_utils.com2root): the shift is the first row's CoM
        q0 = q[0].copy()
        com0 = q0[:3] + rotate_vec_with_quat(np.asarray(self.a['com_offset'], float), q0[3:]/np.linalg.norm(q0[3:]))
        q[:, :2] -= com0[:2]
        T = len(q)
        return dict(q=q, v=v, episode_steps=min(T, int(np.round(self.time_limit/self.dt))) - (self.future_steps + 1), row0=off + start, shift=com0[:2])


def _row(track, idx):
    return track[min(idx, len(track) - 1)]


# ------------------------------------------------------------------ the observation vector (engine.observation_layout order)
def observation(task, ep, st, first):
    """{key: values} of one environment.  st: dict of the exposed fields (1-D / reshaped below) with 'step' = the step counter the
    observation is made at, and 'sens_mean' = the mean of SENSORDATA over the control step's substeps; first: the FIRST step of an episode
    shows the sensors themselves."""
    a = task.a
    sm = np.asarray(st['sens'] if first else st['sens_mean'], float)
    xpos = st['xpos'].reshape(-1, 3); xquat = st['xquat'].reshape(-1, 4); sx = st['site_xpos'].reshape(-1, 3)
    R = quat_to_mat(xquat[task.thorax]); tp = xpos[task.thorax]
    nforce, ntouch = len(a['sensor_force_sites']), len(a['sensor_touch_sites'])
    oj = np.asarray(a['observable_joints'], int)
    o = collections.OrderedDict()
    o['accelerometer'] = sm[0:3]
    o['actuator_activation'] = np.asarray(st['act'], float)
    app = np.asarray(a['appendage_sites'], int)
    o['appendages_pos'] = ((sx[app] - tp) @ R).ravel() if len(app) else np.zeros(0)                 # fruitfly.py:674-684
    o['ball_qvel'] = np.asarray(st['qvel'][-3:], float) if task.kind == 'ball' else np.zeros(0)         # walk_on_ball.py:84-90
    o['force'] = sm[9:9 + 3*nforce]
    o['gyro'] = sm[3:6]
    o['joints_pos'] = st['qpos'][np.asarray(a['jnt_qposadr'])[oj]]
    o['joints_vel'] = st['qvel'][np.asarray(a['jnt_dofadr'])[oj]]
    if task.nf:
        rows = np.array([_row(ep['q'], st['step'] + k) for k in range(task.nf)])
        o['ref_displacement'] = ((rows[:, :3] - st['qpos'][:3]) @ R).ravel()                           # base.py:246-256
        o['ref_root_quat'] = get_dquat_local(st['qpos'][3:7], rows[:, 3:7]).ravel()                    # base.py:259-268
    else:
        o['ref_displacement'] = np.zeros(0); o['ref_root_quat'] = np.zeros(0)
    o['touch'] = sm[9 + 3*nforce:9 + 3*nforce + ntouch]
    o['velocimeter'] = sm[6:9]
    o['world_zaxis'] = R[2]                                                                            # xmat[6:]
    return o


def observation_operands(task, ep, st, sens_abs_sum):
    """{key: (c, scale)}: the FP32 build's a-priori bound on a key is c x 2^-24 x scale (tests/task_cases.py derives the c's); scale is
    the largest operand of the key, sens_abs_sum the per-sensor sum of |SENSORDATA| over the substeps (None on a FIRST step)."""
    a = task.a
    xpos = st['xpos'].reshape(-1, 3); sx = st['site_xpos'].reshape(-1, 3); tp = xpos[task.thorax]
    app = np.asarray(a['appendage_sites'], int)
    big = lambda *xs: max([float(np.abs(x).max()) for x in xs if np.size(x)] + [0.0])
    out = {k: (0, 0.0) for k in ('actuator_activation', 'ball_qvel', 'joints_pos', 'joints_vel')}
    nforce, ntouch = len(a['sensor_force_sites']), len(a['sensor_touch_sites'])
    sl = dict(accelerometer=slice(0, 3), gyro=slice(3, 6), velocimeter=slice(6, 9), force=slice(9, 9 + 3*nforce), touch=slice(9 + 3*nforce, 9 + 3*nforce + ntouch))
    for k in SENSOR_KEYS:
        out[k] = (0, 0.0) if sens_abs_sum is None else (1, big(sens_abs_sum[sl[k]]))
    out['appendages_pos'] = (24, big(sx[app], tp))
    out['world_zaxis'] = (8, 1.0)
    if task.nf:
        rows = np.array([_row(ep['q'], st['step'] + k) for k in range(task.nf)])
        raw = np.abs(rows[:, :3]); raw[:, :2] += np.abs(ep['shift'])                                  # the rows as the dataset holds them
        out['ref_displacement'] = (27, big(raw, st['qpos'][:3]))
        qn = float(np.linalg.norm(st['qpos'][3:7]))
        out['ref_root_quat'] = (48, big(rows[:, 3:7])/qn)
    else:
        out['ref_displacement'] = (0, 0.0); out['ref_root_quat'] = (0, 0.0)
    return out


# ------------------------------------------------------------------ rewards and terminations
def _physics_error(st):
    qacc = np.asarray(st['qacc'], float)
    n = np.linalg.norm(qacc)
    return bool(n > TERMINAL_QACC or np.isnan(n))


def joint_xaxis(a, qpos, xquat, j):
    """MuJoCo's xaxis of hinge j (mj_kinematics) from XQUAT: a body's joints rotate its frame one after the other, and a joint's axis is
    taken in the frame as its predecessors left it -- the body's final frame with the joints that FOLLOW j on the same body undone."""
    axis = np.asarray(a['jnt_axis'], float); body = np.asarray(a['jnt_bodyid']); qadr = np.asarray(a['jnt_qposadr'])
    q = np.asarray(xquat[int(body[j])], float)
    for l in sorted((int(l) for l in np.nonzero(body == body[j])[0] if l > j), reverse=True):
        assert int(a['jnt_type'][l]) == 3                                        # hinges (the free root has a body of its own)
        q = mult_quat(q, conj_quat(axis_angle_to_quat(axis[l], qpos[qadr[l]])[0]))
    return rotate_vec_with_quat(axis[j], q)


def walker_features(task, st):
    """rewards.py:37-62 from the exposed state (xaxis of a hinge = its body's frame applied to the joint's axis)"""
    a = task.a; jid = np.asarray(task.joint_ids, int); sid = np.asarray(task.site_ids, int)
    qpos, qvel = st['qpos'], st['qvel']
    xquat = st['xquat'].reshape(-1, 4); sx = st['site_xpos'].reshape(-1, 3)
    root_quat = qpos[3:7]
    xaxis = np.array([joint_xaxis(a, qpos, xquat, int(j)) for j in jid])
    xaxis = rotate_vec_with_quat(xaxis, reciprocal_quat(root_quat))
    jq = joint_orientation_quat(xaxis, qpos[np.asarray(a['jnt_qposadr'])[jid]])
    f = collections.OrderedDict()
    f['com'] = qpos[:3]
    f['qvel'] = np.concatenate([qvel[:6], qvel[np.asarray(a['jnt_dofadr'])[jid]]])
    f['root2site'] = get_egocentric_vec(qpos[:3], sx[sid], root_quat)
    f['joint_quat'] = np.vstack([root_quat, jq])
    return f


def reference_features(task, ep, tstep):
    """rewards.py:65-81 at frame tstep of the episode's snippet (its x / y start at 0: trajectory_loaders.py:249)"""
    ds = task.ds; T = len(ep['q'])
    row = ep['row0'] + min(tstep, T - 1)
    f = collections.OrderedDict()
    f['com'] = _row(ep['q'], tstep)[:3]
    f['qvel'] = np.asarray(ds.qvel[row], float)
    f['root2site'] = np.asarray(ds.root2site[row], float).reshape(-1, 3)
    f['joint_quat'] = np.vstack([np.asarray(ds.qpos[row, 3:7], float), np.asarray(ds.joint_quat[row], float).reshape(-1, 4)])
    return f


def outcome(task, ep, st):
    """What after_step decides for one environment: dict(reward, factors [5] or None, diffs, term, traj_end, predicates {name: (fired,
    compared quantity, threshold)}).  st['step'] is the step counter AFTER before_step's increment, st['prev'] the one before."""
    a = task.a; sens = np.asarray(st['sens'], float)
    pred = collections.OrderedDict()
    pred['physics_error'] = (_physics_error(st), float(np.linalg.norm(st['qacc'])), TERMINAL_QACC)
    factors = diffs = None
    traj_end = False
    if task.kind == 'template':                                               # template_task.py:75-84
        reward = 1.0
    elif task.kind == 'ball':                                                 # walk_on_ball.py:65-82
        linvel, angvel = float(np.linalg.norm(sens[6:9])), float(np.linalg.norm(sens[3:6]))
        pred['linvel'] = (linvel > TERMINAL_LINVEL, linvel, TERMINAL_LINVEL); pred['angvel'] = (angvel > TERMINAL_ANGVEL, angvel, TERMINAL_ANGVEL)
        reward = float(np.prod(tolerance_linear(st['qvel'][-3:] - np.array([0.0, -5, 0]), 6.0)))
    elif task.kind in ('walk', 'walk_ds'):                                    # walk_imitation.py:152-203
        linvel, angvel = float(np.linalg.norm(sens[6:9])), float(np.linalg.norm(sens[3:6]))
        tstep = task.clock_step(st['time'])
        com_dist = float(np.linalg.norm(_row(ep['q'], st['step'])[:3] - st['qpos'][:3]))
        traj_end = tstep == ep['episode_steps']
        pred['linvel'] = (linvel > TERMINAL_LINVEL, linvel, TERMINAL_LINVEL); pred['angvel'] = (angvel > TERMINAL_ANGVEL, angvel, TERMINAL_ANGVEL)
        pred['traj_end'] = (traj_end, tstep, ep['episode_steps'])
        pred['com_dist'] = (com_dist > task.terminal_com_dist, com_dist, task.terminal_com_dist)
        reward = 1.0
        if task.kind == 'walk_ds':
            f4, diffs = reward_factors_deep_mimic(walker_features(task, st), reference_features(task, ep, tstep))
            wj = np.asarray(a['jnt_qposadr'])[np.asarray(a['wing_jnt'], int)]
            wings = float(np.prod(tolerance_linear(st['qpos'][wj] - np.asarray(a['qpos_spring'], float)[wj], 3.0)))
            factors = np.concatenate([f4, [wings]]); reward = float(np.prod(factors))
    else:                                                                     # flight_imitation.py:170-223
        prev = st['prev']; dt = task.dt_real
        gq0 = _row(ep['q'], prev); gv = _row(ep['v'], prev)
        # the ghost: set to ref[prev] with ref's velocity in before_step (:161-166), then integrated over the control step as a free body
        gp = gq0[:3] + dt*gv[:3]
        w = gv[3:6]; wn = float(np.linalg.norm(w))
        rot = np.array([1.0, 0, 0, 0]) if wn == 0 else np.concatenate([[np.cos(wn*dt/2)], np.sin(wn*dt/2)*w/wn])
        gq = mult_quat(gq0[3:7]/np.linalg.norm(gq0[3:7]), rot); gq /= np.linalg.norm(gq)
        ghost_com = gp + rotate_vec_with_quat(np.asarray(a['com_offset'], float), gq)                  # task_utils.root2com
        disp = float(np.linalg.norm(ghost_com - st['com']))
        nxt = _row(ep['q'], st['step'])
        dq = get_dquat_local(st['qpos'][3:7], nxt[3:7])
        qd = float(quat_dist_short_arc(np.array([1.0, 0, 0, 0]), dq))
        lj = np.asarray(a['leg_joints'], int) if np.size(a['leg_joints']) else np.zeros(0, int)
        la = np.asarray(a['jnt_qposadr'])[lj]
        legs = float(np.prod(tolerance_linear(st['qpos'][la] - np.asarray(a['qpos_spring'], float)[la], 4.0))) if len(lj) else 1.0
        reward = float(tolerance_linear(disp, 0.4)*tolerance_linear(qd, np.pi)*legs)
        height = float(st['xpos'].reshape(-1, 3)[task.thorax, 2])
        com_dist = float(np.linalg.norm(nxt[:3] - st['qpos'][:3]))
        tstep = task.clock_step(st['time'])
        traj_end = tstep == ep['episode_steps']
        pred['height'] = (height < TERMINAL_HEIGHT, height, TERMINAL_HEIGHT)
        pred['com_dist'] = (com_dist > task.terminal_com_dist, com_dist, task.terminal_com_dist)
        pred['traj_end'] = (traj_end, tstep, ep['episode_steps'])
        diffs = dict(disp=disp, quat_dist=qd)
    term = any(p[0] for p in pred.values())
    return dict(reward=reward, factors=factors, diffs=diffs, term=term, traj_end=bool(traj_end), predicates=pred)


def step_end(task, out, time):
    """base.py:206-225 with the imitation tasks' get_discount (walk_imitation.py:194-203) and dm_control's time limit:
    (step_type, discount) of a step that is not the first of its episode; the step after a LAST is a FIRST (reward 0, discount 1)."""
    terminating = out['term'] or time >= task.time_limit
    discount = 0.0 if (out['term'] and not out['traj_end']) else 1.0
    return (LAST if terminating else MID), discount
