"""Cases, runner and bounds of tests/test_task_layer.py: the kernel's task layer (csrc/fb_task.hpp) against tests/task_reference.py at the
kernel's OWN state, so that neither FP32 physics drift nor contact chaos enters.

THE RUNNER (run_case).  A control step is walked by single-stage launches (Batch.stage over engine.stage_sequence; tests/test_gpu_parity.py::
test_single_stage_launches_equal_fused_step_gpu holds that walk equal to the fused step to the bit).  SENSORDATA is read after every
`velocity` stage -- the stage that closes a substep and adds the sensors to the control step's accumulators (fb_step.hpp: s_velocity) -- and
the substep mean is taken on the host in FP64.  In front of `task_post` the exposed state is read (and, in the quat*1.7 cases, QPOS's root
quaternion is scaled there), then `task_post` is launched and OBS, REWARD, DISCOUNT, STEP_TYPE and REWARD_FACTORS are read.  A step in
which an environment is auto-reset cannot be walked by stages (the stage walk has no reset branch), so whenever the previous step left a
LAST the fused step runs for the whole batch: task_post changes nothing of the exposed state but the step counter, so the state read
AFTER a fused step is the state in front of its task_post; only the sensor means are unknown there, and the sensor-mean keys of such a step
are checked for the environments that were reset (FIRST: the kernel packs the sensors themselves).  The termination rollouts use fused
steps throughout: they compare decisions, rewards and the keys that are no sensor means.

WHAT THE REFERENCE IS GIVEN.  The FP64 build: the configuration as it is.  The FP32 build: every real-valued input the kernel holds in
single precision -- reference track, dataset, model constants, terminal_com_dist -- rounded to single precision first (exact when read as
FP64, like the state fb_batch_get returns), so that the difference is the epilogue's own arithmetic.

BOUNDS.  FP64 build: OBS and REWARD are float32 outputs of FP64 values, |x - ref| <= 2^-24 |ref| + 1e-12 max|key|; REWARD_FACTORS (a double
field) 1e-10 relative; STEP_TYPE and DISCOUNT equal.  FP32 build, observation keys, |x - ref| <= c 2^-24 s with s the key's largest operand
(task_reference.observation_operands) and c counted from the operations, an a-priori worst case and not a measurement:
  actuator_activation, ball_qvel, joints_pos, joints_vel   c = 0: copies of single-precision state
  accelerometer, force, gyro, touch, velocimeter           c = 1, s = sum over the substeps of |sensor|: n - 1 additions, each rounding a partial sum
                                                           <= s, make (n - 1) 2^-24 s on the sum, / n, plus the division's own 2^-24 s / n; FIRST: c = 0
  world_zaxis                                              c = 8, s = 1: a row of quat2mat of a unit quaternion, at most 4 products and 3 sums of
                                                           terms whose absolute values add up to <= 1 (the diagonal entry)
  appendages_pos                                           c = 24 = 3 terms x 8, s = max(|site|, |thorax|): per term <= 4 roundings of the matrix
                                                           entry (above, halved: entries <= 1), 1 of the subtraction, 1 of the product, 2 of the
                                                           running sum; every term is bounded by the largest operand
  ref_displacement                                         c = 27: the same with one more subtraction per term in dataset mode (the loader's x / y shift)
  ref_root_quat                                            c = 48 = 4 terms x 12, s = max|ref quat| / |q|: qinv = conj(q) / n2 carries 7 roundings of n2
                                                           and 1 of the division, the Hamilton product 1 per product and 3 of the running sum
REWARD (by task) and REWARD_FACTORS (walk_imitation's dataset mode, by factor): REWARD_BOUND32 / FACTOR_BOUND32 below, 4 x the worst relative
difference measured on the emulation build, the ray-casting tests' rule; never above 1e-4, the project's north-star tolerance.

DECISIONS (termination rollouts).  Every environment's STEP_TYPE and DISCOUNT must equal the reference's at the kernel's own state.  A
decision is left out only where a compared quantity lies within the FP32 rounding band of its threshold:
  com_dist = |ref - qpos|      band 4 x 2^-24 max(com_dist, terminal_com_dist): 3 subtractions, 3 squares, 2 sums, the square root
  linvel, angvel = |sensor|    band 4 x 2^-24 max(value, threshold): the same without the subtractions
  height, the clock, the step counts: no band (a stored value against a constant; a double; integers).
None may be left out in FP64, at most 2 % in FP32 (asserted)."""
import collections
import os

import numpy as np

import task_reference as tr
from conftest import ROOT
from _synthetic_dataset import make_dataset
from _synthetic_flight_dataset import make_flight_dataset

U = 2.0**-24
STATE_FIELDS = ('QPOS', 'QVEL', 'ACT', 'XPOS', 'XQUAT', 'SITE_XPOS', 'SUBTREE_COM', 'QACC', 'SENSORDATA', 'STEP_COUNT', 'TIME')
# 4 x the worst relative difference to the numpy reference measured on the emulation build (test_task_layer.py's docstring has the figures
# beside the MI355X's): REWARD by task -- walk_imitation's inference reward and template_task's are the constant 1 --, REWARD_FACTORS by factor
# (com, qvel, root2site, joint_quat, wings).  All below 1e-4, the project's north-star tolerance.
REWARD_BOUND32 = dict(walk=0.0, template=0.0, ball=4*6.44e-7, flight=4*4.66e-6, flight_ds=4*4.66e-6, walk_ds=4*1.26e-5)
FACTOR_BOUND32 = 4*np.array([4.7e-8, 4.4e-8, 4.47e-8, 1.25e-5, 1.38e-7])
assert max(REWARD_BOUND32.values()) <= 1e-4 and FACTOR_BOUND32.max() <= 1e-4
FAR = np.array([50.0, -30.0])


def arrays(name):
    from flybody_amd.model_blob import load_npz
    if name == 'template_task':
        from law_helpers import template_arrays
        return template_arrays()
    return load_npz(os.path.join(ROOT, 'flybody_amd', 'assets', name + '.npz'))


def _round32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _arrays32(a):
    return {k: (_round32(v) if isinstance(v, np.ndarray) and v.dtype == np.float64 and not k.startswith('opt_') else v) for k, v in a.items()}


_CACHE = {}


def walk_dataset():
    """3 trajectories of 14 frames recorded from the oracle (tests/_synthetic_dataset.py): with future_steps 2 a snippet ends after 11 steps"""
    if 'walk_ds' not in _CACHE:
        from flybody_amd.model_blob import pack_model
        from oracle import fbo
        a = arrays('walk_imitation')
        ds = make_dataset(fbo.OracleModel(pack_model(a)), a, n_traj=3, length=14)
        _CACHE['walk_ds'] = (ds,) + tuple(ds.ids(a))
    return _CACHE['walk_ds']


def clock_dataset(n_frames, step=0.01):
    """Beside make_dataset, without the oracle: one trajectory whose CoM moves by `step` per frame, everything else at rest in the default
    pose.  A CoM that advanced for good would be 27 cm from a fly that stands still under zero actions by frame 2700, and the DeepMimic factor
    of the CoM, 20 exp(-81.2 d^2), underflows to 0 there: the track is a sawtooth instead, x = step (k mod 7) and y = step (k mod 5), so that
    it stays within 0.07 of the fly while any two of the frames k - 1, k, k + 1 are at least `step` apart in x and in y; one frame of
    misalignment moves the factor by 0.8 % or more."""
    from flybody_amd.trajectory_loaders import WalkingDataset
    ds0, jid, sid = walk_dataset()
    a = arrays('walk_imitation'); nj, ns = len(jid), len(sid)
    qpos = np.zeros((n_frames, 7 + nj)); qpos[:, :7] = a['qpos0'][:7]; qpos[:, 0] = step*(np.arange(n_frames) % 7); qpos[:, 1] = step*(np.arange(n_frames) % 5); qpos[:, 7:] = a['qpos0'][a['jnt_qposadr'][jid]]
    jq = np.tile(np.array([1.0, 0, 0, 0]), (n_frames, nj, 1))
    ds = WalkingDataset(np.array([0, n_frames], np.int32), qpos, np.zeros((n_frames, 6 + nj)), np.zeros((n_frames, ns, 3)), jq, ds0.joint_names, ds0.site_names, 2e-3)
    return ds, jid, sid


def _flight_track(n, shift=(0.0, 0.0), z=1.0):
    from flybody_amd.mjcf_compile import qrot
    from flybody_amd.reference import constant_speed_trajectory
    a = arrays('flight_imitation')
    cq, cv = constant_speed_trajectory(n, 20.0, init_pos=(0, 0, z), body_rot_angle_y=-47.5, control_timestep=2e-4)
    root = np.array(cq, float)
    for i in range(len(root)): root[i, :3] = cq[i, :3] + qrot(cq[i, 3:], -a['com_offset'])
    root[:, :2] += shift
    return root, np.array(cv, float)


# name -> dict(task asset, kind, n_env, steps, action range, and what configure() needs).  events: {step k: what happens in front of its
# task_post ('quat': the root quaternion x 1.7) or in front of the step ('qvel' / 'qpos': (env, index, value) written to the state)}
Case = collections.namedtuple('Case', 'name asset kind n_env steps amp seed cfg events staged')


def _c(name, asset, kind, n_env, steps, amp, seed, cfg, events=None, staged=True):
    return Case(name, asset, kind, n_env, steps, amp, seed, cfg, events or {}, staged)


def cases():
    from flybody_amd.reference import default_walking_reference
    qp, qv = default_walking_reference()
    far = np.array(qp[:8], float); far[:, :2] += FAR
    fq, fv = _flight_track(20); fqf, _ = _flight_track(20, FAR)
    walk = dict(ref_qpos=qp[:8], ref_qvel=qv[:8], future_steps=2, terminal_com_dist=0.3)
    flight = dict(ref_qpos=fq, ref_qvel=fv, future_steps=5, terminal_com_dist=2.0, time_limit=0.6)
    fds = dict(future_steps=5, terminal_com_dist=2.0, time_limit=20*2e-4, randomize_start_step=True, seed=7, env_id_base=100)
    return collections.OrderedDict((c.name, c) for c in (
        # ---- the epilogue at the kernel's own state: staged steps
        _c('walk', 'walk_imitation', 'walk', 5, 7, 1.0, 11, walk),                       # FIRST, MID, the trajectory ends at step 5 (LAST, discount 1), FIRST, MID
        _c('walk_far', 'walk_imitation', 'walk', 3, 2, 1.0, 12, dict(walk, ref_qpos=far)),
        _c('walk_quat', 'walk_imitation', 'walk', 3, 2, 1.0, 13, walk, {1: 'quat', 2: 'quat'}),
        _c('walk_ds', 'walk_imitation', 'walk_ds', 3, 3, 0.3, 1, dict(future_steps=2, terminal_com_dist=np.inf, seed=3, env_id_base=4)),
        _c('walk_ds_quat', 'walk_imitation', 'walk_ds', 3, 2, 0.3, 2, dict(future_steps=2, terminal_com_dist=np.inf, seed=5, env_id_base=1), {2: 'quat'}),
        _c('flight', 'flight_imitation', 'flight', 3, 3, 1.0, 1, flight),
        _c('flight_far', 'flight_imitation', 'flight', 3, 2, 1.0, 2, dict(flight, ref_qpos=fqf)),
        _c('flight_quat', 'flight_imitation', 'flight', 3, 2, 1.0, 3, flight, {2: 'quat'}),
        _c('flight_ds', 'flight_imitation', 'flight_ds', 3, 3, 1.0, 4, fds),
        _c('ball', 'walk_on_ball', 'ball', 3, 5, 0.5, 0, dict(time_limit=0.006)),       # LAST by the time limit at step 3, FIRST, MID
        _c('template', 'template_task', 'template', 3, 3, 0.5, 5, dict(time_limit=0.004)),
        # ---- termination rollouts: fused steps, thresholds brought into reach
        _c('walk_early', 'walk_imitation', 'walk', 4, 12, 1.0, 11, dict(walk, terminal_com_dist=0.005), {7: ('qvel', 1, 0, 80.0), 9: ('qvel', 2, 5, 400.0)}, staged=False),
        _c('walk_ds_end', 'walk_imitation', 'walk_ds', 3, 13, 0.3, 1, dict(future_steps=2, terminal_com_dist=np.inf, seed=3, env_id_base=4), staged=False),
        _c('flight_early', 'flight_imitation', 'flight', 4, 12, 1.0, 1, dict(flight, terminal_com_dist=0.002), {8: ('qpos', 3, 2, 0.15)}, staged=False),
        _c('flight_end', 'flight_imitation', 'flight', 3, 16, 0.3, 6, flight, staged=False),       # 20 frames, future_steps 5: the trajectory ends at step 14
        _c('flight_ds_limit', 'flight_imitation', 'flight_ds', 3, 16, 0.3, 4, fds, staged=False),
        _c('ball_limit', 'walk_on_ball', 'ball', 3, 8, 0.5, 0, dict(time_limit=0.012), staged=False),
        _c('template_limit', 'template_task', 'template', 3, 5, 0.5, 5, dict(time_limit=0.006), staged=False),
    ))



def configure(case, lib, precision, dense=False):
    """(Batch, task_reference.Task, nact) of a case on library `lib` (None: the GPU library)"""
    from flybody_amd import engine
    from flybody_amd.wbpg import build_tables
    a = arrays(case.asset)
    B = engine.Batch(engine.Model(a, lib_path=lib, dense=dense), case.n_env, precision=precision)
    r = _round32 if precision == 32 else (lambda x: np.asarray(x, float))
    ar = _arrays32(a) if precision == 32 else a
    cfg = dict(case.cfg)
    if case.asset == 'flight_imitation': B.set_wbpg(build_tables(), seed=5)
    if case.kind in ('walk', 'flight'):
        B.set_reference(cfg['ref_qpos'], cfg['ref_qvel'], **{k: v for k, v in cfg.items() if not k.startswith('ref_')})
        task = tr.Task(case.kind, ar, r(cfg['ref_qpos']), r(cfg['ref_qvel']), cfg['future_steps'], float(r(cfg['terminal_com_dist'])), cfg.get('time_limit', 10.0))
    elif case.kind == 'walk_ds':
        ds, jid, sid = cfg.pop('ds', None) or walk_dataset()
        B.set_walk_dataset(ds, jid, sid, **cfg)
        dsr = collections.namedtuple('DS', 'n_traj offsets qpos qvel root2site joint_quat')(ds.n_traj, ds.offsets, r(ds.qpos), r(ds.qvel), r(ds.root2site), r(ds.joint_quat))
        task = tr.Task('walk_ds', ar, None, None, cfg['future_steps'], float(r(cfg['terminal_com_dist'])), cfg.get('time_limit', 10.0), ds=dsr, joint_ids=jid,
                       site_ids=sid, seed=cfg['seed'], env_id_base=cfg['env_id_base'])
    elif case.kind == 'flight_ds':
        ds = make_flight_dataset(); root = ds.root_qpos(a['com_offset'])
        B.set_flight_dataset(ds.offsets, root, ds.com_qvel, **cfg)
        task = tr.Task('flight_ds', ar, None, None, cfg['future_steps'], float(r(cfg['terminal_com_dist'])), cfg['time_limit'], ds=(ds.offsets, r(root), r(ds.com_qvel)),
                       seed=cfg['seed'], env_id_base=cfg['env_id_base'], randomize_start_step=cfg['randomize_start_step'])
    elif case.kind == 'ball':
        B.set_time_limit(cfg['time_limit'])
        task = tr.Task('ball', ar, time_limit=cfg['time_limit'])
    else:
        root = np.tile(np.asarray(a['qpos0'][:7], float), (2, 1))
        B.set_reference(root, np.zeros((2, 6)), future_steps=0, terminal_com_dist=float('inf'), time_limit=cfg['time_limit'])
        task = tr.Task('template', ar, r(root), np.zeros((2, 6)), 0, np.inf, cfg['time_limit'])
    task.dt_real = float(np.float32(task.dt)) if precision == 32 else task.dt
    return B, task, B.model.dim('nact')


class Device:
    """Actions and launches of a batch on the GPU or on the emulation build (whose "device" memory is host memory)"""

    def __init__(self, B, on_gpu):
        self.B, self.on_gpu = B, on_gpu
        if on_gpu:
            import torch
            self.torch = torch; self.st = torch.cuda.current_stream().cuda_stream

    def action(self, a):
        a = np.ascontiguousarray(a, np.float32)
        if self.on_gpu:
            self._keep = self.torch.from_numpy(a).cuda(); return self._keep.data_ptr()
        self._keep = a; return a.ctypes.data

    def step(self, a):
        if self.on_gpu: self.B.step_ptr(self.action(a), self.st); self.B.synchronize(self.st)
        else: self.B.step_ptr(self.action(a))

    def stage(self, word, ptr):
        if self.on_gpu: self.B.stage(word, ptr, self.st)
        else: self.B.stage(word, ptr)


def read_state(B):
    return {f: B.get(f).copy() for f in STATE_FIELDS}


def read_outputs(B, factors):
    out = {f: B.get(f).copy() for f in ('OBS', 'REWARD', 'DISCOUNT', 'STEP_TYPE')}
    if factors: out['REWARD_FACTORS'] = B.get('REWARD_FACTORS').copy()
    return out


def env_state(S, e, step, prev, sens_mean=None):
    st = dict(qpos=S['QPOS'][e], qvel=S['QVEL'][e], act=S['ACT'][e], xpos=S['XPOS'][e], xquat=S['XQUAT'][e], site_xpos=S['SITE_XPOS'][e],
              com=S['SUBTREE_COM'][e], qacc=S['QACC'][e], sens=S['SENSORDATA'][e], time=float(S['TIME'][e, 0]), step=int(step), prev=int(prev))
    if sens_mean is not None: st['sens_mean'] = sens_mean
    return st


def scale_root_quat(B, factor=1.7):
    q = B.get('QPOS'); q[:, 3:7] *= factor; B.set('QPOS', q)


def run_case(case, lib, precision, on_gpu=False, dense=False):
    """The case's steps on library `lib`: a list of records, one per (control step, environment), index 0 the reset:
    dict(k, env, first, st: the state the epilogue saw (env_state), sens_abs_sum or None, episode: the environment's episode number,
    out: {OBS, REWARD, DISCOUNT, STEP_TYPE[, REWARD_FACTORS]} of the environment).  Returns (task, records)."""
    from flybody_amd import engine
    B, task, nact = configure(case, lib, precision, dense)
    dev = Device(B, on_gpu)
    n = case.n_env; factors = case.kind == 'walk_ds'
    seq = engine.stage_sequence(B.model.dim('nsubstep'))
    acts = np.random.default_rng(case.seed).uniform(-case.amp, case.amp, (case.steps, n, nact)).astype(np.float32)
    episode = np.zeros(n, int); recs = []
    B.reset()
    S, O = read_state(B), read_outputs(B, factors)
    for e in range(n):
        recs.append(dict(k=0, env=e, first=True, st=env_state(S, e, 0, 0), sens_abs_sum=None, episode=int(episode[e]), out={f: v[e] for f, v in O.items()}))
    pending = np.zeros(n, bool)                       # the environment's last step was a LAST: the next one resets it
    for k in range(1, case.steps + 1):
        ev = case.events.get(k)
        if isinstance(ev, tuple):
            kind, e, i, v = ev; f = 'QVEL' if kind == 'qvel' else 'QPOS'
            x = B.get(f); x[e, i] = v; B.set(f, x)
        a = acts[k - 1]
        if case.staged and not pending.any():
            ptr = dev.action(a); sens = []
            for name, word in seq[:-1]:
                dev.stage(word, ptr)
                if name == 'velocity': sens.append(B.get('SENSORDATA').copy())
            if ev == 'quat': scale_root_quat(B)
            S = read_state(B)
            dev.stage(seq[-1][1], ptr)
            O = read_outputs(B, factors)
            mean, asum = np.mean(sens, axis=0), np.sum(np.abs(sens), axis=0)
            for e in range(n):
                prev = int(S['STEP_COUNT'][e, 0])
                recs.append(dict(k=k, env=e, first=False, st=env_state(S, e, prev + 1, prev, mean[e]), sens_abs_sum=asum[e], episode=int(episode[e]),
                                 out={f: v[e] for f, v in O.items()}))
        else:
            dev.step(a)
            S, O = read_state(B), read_outputs(B, factors)
            for e in range(n):
                if pending[e]: episode[e] += 1
                step = int(S['STEP_COUNT'][e, 0])
                recs.append(dict(k=k, env=e, first=bool(pending[e]), st=env_state(S, e, step, step - 1), sens_abs_sum=None, episode=int(episode[e]),
                                 out={f: v[e] for f, v in O.items()}))
        pending = O['STEP_TYPE'][:, 0] == tr.LAST
    return task, recs


# ------------------------------------------------------------------ the comparison
def expected(task, rec, layout):
    """What the reference makes of a record's state: dict(obs {key: values}, operands {key: (c, s)}, reward, discount, step_type, factors, outcome)"""
    st = rec['st']; ep = task.episode(rec['env'], rec['episode'])
    obs = tr.observation(task, ep, st, rec['first']) if ('sens_mean' in st or rec['first']) else tr.observation(task, ep, dict(st, sens_mean=np.full(33, np.nan)), False)
    ops = tr.observation_operands(task, ep, st, None if rec['first'] else rec['sens_abs_sum'])
    assert [k for k in layout] == [k for k in obs] and all(layout[k][1] == obs[k].size for k in layout)
    if rec['first']:
        return dict(obs=obs, operands=ops, reward=0.0, discount=1.0, step_type=tr.FIRST, factors=None, outcome=None)
    out = tr.outcome(task, ep, st)
    step_type, discount = tr.step_end(task, out, st['time'])
    return dict(obs=obs, operands=ops, reward=out['reward'], discount=discount, step_type=step_type, factors=out['factors'], outcome=out)


def band32(out, task):
    """True where a compared quantity lies within the FP32 rounding band of its threshold (the module docstring has the formulas)"""
    for name, (_, x, thr) in out['predicates'].items():
        if name in ('com_dist', 'linvel', 'angvel') and np.isfinite(thr) and abs(x - thr) <= 4*U*max(abs(x), abs(thr)): return True
    return False


def rel(x, ref):
    return float(np.max(np.abs(np.asarray(x, float) - np.asarray(ref, float))/np.maximum(np.abs(np.asarray(ref, float)), 1e-300)))


def check_record(task, rec, layout, precision, figures):
    """Asserts the bounds of the module docstring on one record; appends the FP32 reward / factor differences to `figures`.  Returns the expectation."""
    x = expected(task, rec, layout); out = rec['out']; where = (rec['k'], rec['env'])
    no_means = not rec['first'] and 'sens_mean' not in rec['st']           # a fused step: the substeps' sensors were not read
    for key, (off, size, _) in layout.items():
        if size == 0 or (key in tr.SENSOR_KEYS and no_means): continue
        got = out['OBS'][off:off + size].astype(np.float64); ref = np.asarray(x['obs'][key], float)
        if precision == 64: bound = U*np.abs(ref) + 1e-12*np.abs(ref).max()
        else:
            c, s = x['operands'][key]
            bound = c*U*s*np.ones_like(ref)                                     # (the FP32 build's output conversion is exact)
        err = np.abs(got - ref)
        assert (err <= bound).all(), (where, key, float(err.max()), float(np.max(bound)), int(np.argmax(err - bound)))
    if x['outcome'] is None or not (precision == 32 and band32(x['outcome'], task)):
        assert int(out['STEP_TYPE'][0]) == x['step_type'] and float(out['DISCOUNT'][0]) == x['discount'], (where, out['STEP_TYPE'], out['DISCOUNT'], x['step_type'], x['discount'], x['outcome'] and x['outcome']['predicates'])
    r, ref = float(out['REWARD'][0]), x['reward']
    if precision == 64: assert abs(r - ref) <= U*abs(ref) + 1e-12, (where, r, ref)
    else:
        if ref != 0: figures.setdefault('reward', []).append(abs(r - ref)/abs(ref))
        assert abs(r - ref) <= REWARD_BOUND32[task.kind]*abs(ref), (where, r, ref)
    if x['factors'] is not None:
        d = np.abs(out['REWARD_FACTORS'] - x['factors'])/np.abs(x['factors'])
        if precision == 64: assert d.max() <= 1e-10, (where, out['REWARD_FACTORS'], x['factors'])
        else:
            for i in range(5): figures.setdefault('factor%d' % i, []).append(d[i])
            assert (d <= FACTOR_BOUND32).all(), (where, d, out['REWARD_FACTORS'], x['factors'])
    return x
