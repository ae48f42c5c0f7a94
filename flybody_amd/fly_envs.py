"""dm_env-compatible fly environments backed by the batched HIP engine.

Mirrors the public surface of the reference's ``flybody/fly_envs.py`` for the hot-path task:
``walk_imitation(...)`` (fly_envs.py:100-155) returns an object with ``reset() / step(action) /
action_spec() / observation_spec() / control_timestep() / physics.timestep() /
task._traj_generator.set_next_trajectory(qpos, qvel)`` -- the members the reference's tests use
(tests/test_walking_env.py:37-72).  dm_env itself is not a dependency: `TimeStep`, `StepType`
and the specs below are attribute-compatible stand-ins.

`BatchedFlyEnv` is the native interface (thousands of environments in lock-step on one GPU,
observations/rewards as torch tensors that alias the engine's device buffers); `walk_imitation`
with ``n_env=1`` wraps one of them as a single dm_env-style environment.
"""
from __future__ import annotations

import collections
import enum
from typing import Optional, Sequence

import numpy as np

from . import engine
from .engine import observation_layout
from .reference import constant_speed_trajectory, default_walking_reference


class StepType(enum.IntEnum):
    FIRST = 0
    MID = 1
    LAST = 2


class TimeStep(collections.namedtuple('TimeStep', ['step_type', 'reward', 'discount', 'observation'])):
    __slots__ = ()

    def first(self): return self.step_type == StepType.FIRST
    def mid(self): return self.step_type == StepType.MID
    def last(self): return self.step_type == StepType.LAST


class Array:
    def __init__(self, shape, dtype, name=None):
        self.shape = tuple(shape); self.dtype = np.dtype(dtype); self.name = name


class BoundedArray(Array):
    def __init__(self, shape, dtype, minimum, maximum, name=None):
        super().__init__(shape, dtype, name)
        self.minimum = np.asarray(minimum, dtype); self.maximum = np.asarray(maximum, dtype)


# observation layout (engine.observation_layout): the packed buffer is in sorted-key order (tasks/task_utils.py:12); the dict the
# reference returns lists the walker observables first and the two task observables last
# (tests/test_walking_env.py:11-23)
_DICT_ORDER = ['accelerometer', 'actuator_activation', 'appendages_pos', 'force', 'gyro', 'joints_pos', 'joints_vel',
               'touch', 'velocimeter', 'world_zaxis', 'ref_displacement', 'ref_root_quat', 'ball_qvel']


def action_spec_from_arrays(a) -> BoundedArray:
    """fruitfly.py:548-579: tab-joined actuator names in action order, per-actuator ctrl range, user actions in [-1, 1].
    The values are pinned literally by the reference's notebook outputs (tests/golden/notebook_specs.json)."""
    idx = a['action_to_ctrl']
    rng = a['actuator_ctrlrange'][idx]
    names = [str(a['names_actuator'][i]) for i in idx]
    lo, hi = list(rng[:, 0]), list(rng[:, 1])
    for k in range(int(a['num_user_actions'])):          # fruitfly.py:571-576
        lo.append(-1.0); hi.append(1.0); names.append(f'user_{k}')
    return BoundedArray((len(names),), float, lo, hi, name='\t'.join(names))


class _TrajGenerator:
    """Stand-in for InferenceWalkingTrajectoryLoader (tasks/trajectory_loaders.py:267-309)."""

    def __init__(self, owner):
        self._owner = owner
        self._snippet = None

    def set_next_trajectory(self, qpos, qvel):
        self._snippet = {'qpos': np.asarray(qpos, float), 'qvel': np.asarray(qvel, float)}
        self._owner._apply_reference()

    def get_trajectory(self, traj_idx=None):
        return self._snippet

    def get_joint_names(self): return []
    def get_site_names(self): return []


class _Task:
    def __init__(self, owner):
        self._traj_generator = _TrajGenerator(owner)
        self.prev_action = None            # the batched action the kernel was given last (after the action corruptor; fruitfly.py:532-544)


class _Physics:
    def __init__(self, owner): self._owner = owner
    def timestep(self): return float(self._owner.model.arrays['opt_timestep'])
    def time(self): return self._owner._time


class BatchedFlyEnv:
    """n_env walk_imitation environments stepped in lock-step by one kernel launch per control step."""

    def __init__(self, n_env: int = 1, device: int = 0, precision: int = 64, terminal_com_dist: float = 0.3,
                 joint_filter: float = 0.01, future_steps: int = 64, time_limit: float = 10.0, task: str = 'walk_imitation',
                 wbpg_tables=None, seed: int = 0, traj_loader=None, env_id_base: int = 0, force_actuators: bool = False,
                 use_wings: Optional[bool] = None, use_legs: Optional[bool] = None, dyntype_filterexact: bool = False,
                 use_mouth: bool = False, use_antennae: bool = False, adhesion_filter: Optional[float] = None, dense: Optional[bool] = None,
                 control_callback=None, models=None, env_model=None, resample_on_reset: bool = False, claw_friction: Optional[float] = None,
                 init_qpos=None, reward_fn=None, termination_fn=None, action_corruptor=None, random_state=None):
        """models: a list of array dicts (flybody_amd.randomization.vary_model / sample_models) that the batch steps side by side --
        per-environment physics models, engine.ModelGroup; they replace the task's compiled model (the first one answers the specs) and
        must share its tree.  env_model: the initial assignment [n_env] (default: e % len(models)); env_model() is its device view.
        resample_on_reset: after every control step, the environments whose step type is LAST draw a new model id from a generator
        seeded with `seed` (a torch op on the device, no host sync), so that their auto-reset starts the next episode under it.
        control_callback: a callable f(env) run before every CONTROL step of step() and step_tensor() -- the batched analogue of
        MuJoCo's mjcb_control, typically writing applied_forces() from the batch's state.  It runs once per control step, not once
        per physics substep: what it writes holds for all substeps of that step.  Feedback at the physics rate is a control law
        (set_control_law, flybody_amd.control_laws): per-dof gains that the step kernel evaluates in every substep.
        reward_fn(env) -> float tensor [n_env] and termination_fn(env) -> bool tensor [n_env], or (bool tensor, float32 discount tensor):
        a task written in PyTorch on top of the kernel's.  After the step kernel, on the same stream and without a host sync, the
        reward view becomes where(step_type == FIRST, 0, reward_fn(env)) and the environments the mask names end their episode
        (Batch.end_episode: LAST with that discount, default 0; auto-reset by the next step).  A control step runs, in this order:
        control_callback, action_corruptor, the kernel, reward_fn, termination_fn + end_episode, model resampling.
        action_corruptor(action, random_state): applied to the batched action (the tensor of step_tensor, the [n_env, nact] array of
        step) before the kernel sees it; task.prev_action holds what the kernel was given.
        template_task only: init_qpos, the root pose [7] an episode starts from (default qpos0[:7]); claw_friction."""
        from . import model_zoo
        self.task_name = task
        if task != 'template_task' and (claw_friction is not None or init_qpos is not None):
            raise ValueError(f'claw_friction and init_qpos belong to template_task; {task} takes its claw friction from its compiled model and '
                             'its start pose from its reference')
        # FruitFly._build's configuration space (fruitfly.py:123-386): the compiled tables come from the shipped assets, the
        # variant cache, or a fresh compile of the reference XML (model_zoo.get_model)
        compiled_filter = 0.0 if task == 'flight_imitation' else 0.01
        same_layout = (joint_filter > 0) == (compiled_filter > 0)
        cfg = model_zoo.task_config(task, force_actuators=force_actuators, use_wings=use_wings, use_legs=use_legs,
                                    joint_filter=None if same_layout else joint_filter, adhesion_filter=adhesion_filter,
                                    dyntype_filterexact=dyntype_filterexact, use_mouth=use_mouth, use_antennae=use_antennae,
                                    claw_friction=claw_friction)
        arrays = model_zoo.get_model(cfg)
        if same_layout and joint_filter > 0 and joint_filter != compiled_filter:
            # a different filter TIME CONSTANT keeps the activation layout: patch the table instead of recompiling
            arrays = dict(arrays)
            dyn = arrays['actuator_dynprm'].copy()
            dyn[arrays['actuator_trntype'] != 5] = joint_filter       # fruitfly.py:330-335
            arrays['actuator_dynprm'] = dyn
        self.config = cfg
        if dense is None:
            # the 12-environments-per-CU FP64 build (engine.HIP_LIB_DENSE) is the faster one for batches beyond the default build's
            # 2048 resident environments (substep scheduler) -- since round 4 for flight as well (8192 environments:
            # 2.63 M env-steps/s against 2.25 M, profiles/r4/flight_variants.txt)
            import os as _os
            want = precision == 64 and n_env > 2048
            dense = want and _os.path.exists(engine.HIP_LIB_DENSE)
            if want and not dense:
                import warnings
                warnings.warn(f'{engine.HIP_LIB_DENSE} is missing: FP64 batch of {n_env} environments runs on the default build '
                              '(8 instead of 12 environments per CU; build it with __graft_entry__.build())')
        self.model = engine.ModelGroup(models, dense=bool(dense)) if models is not None else engine.Model(arrays, dense=bool(dense))
        # which binary steps this environment (the implicit choice used to leave no trace): part of the config, logged once
        self.build = 'libflybody_hip_dense.so (FP64, 12 environments per CU)' if dense else 'libflybody_hip.so (default build)'
        if isinstance(self.config, dict): self.config['engine_build'] = self.build
        self.n_env = n_env; self.device = device
        self.batch = engine.Batch(self.model, n_env, device=device, precision=precision)
        self.future_steps = future_steps; self.terminal_com_dist = terminal_com_dist; self.time_limit = time_limit
        self.task = _Task(self); self.physics = _Physics(self)
        self._time = 0.0
        if task == 'flight_imitation' and traj_loader is not None:
            # reference dataset (fly_envs.py:71-76): every trajectory lives on the GPU, each environment picks its slice there
            from .wbpg import build_tables
            self.batch.set_wbpg(wbpg_tables or build_tables(), seed=seed)
            ds = traj_loader.dataset
            self.task._traj_generator = traj_loader
            self.batch.set_flight_dataset(ds.offsets, ds.root_qpos(arrays['com_offset']), ds.com_qvel, select=traj_loader.traj_indices,
                                          future_steps=future_steps, terminal_com_dist=terminal_com_dist, time_limit=time_limit,
                                          randomize_start_step=traj_loader.randomize_start_step, seed=seed, env_id_base=env_id_base)
            qp = qv = None
        elif task == 'flight_imitation':
            from .wbpg import build_tables
            self.batch.set_wbpg(wbpg_tables or build_tables(), seed=seed)
            # InferenceFlightTrajectoryLoader default (trajectory_loaders.py:161-163): 200 steps, 20 cm/s, z = 1, pitch -47.5 deg
            qp, qv = constant_speed_trajectory(200, 20.0, init_pos=(0, 0, 1), body_rot_angle_y=-47.5, control_timestep=2e-4)
        elif task == 'walk_on_ball':
            self.batch.set_time_limit(time_limit)             # fly_envs.py:177: 2 s; no reference trajectory
            qp = qv = None
        elif task == 'template_task':
            # no reference trajectory either: the "reference" is the start pose (fb_task.hpp: the walker's inference init reads row 0)
            if traj_loader is not None:
                raise ValueError('template_task takes no reference dataset')
            root = np.asarray(arrays['qpos0'][:7] if init_qpos is None else init_qpos, float)
            if root.shape != (7,) or not np.isfinite(root).all():
                raise ValueError('init_qpos must be a finite root pose [7]: position, then unit quaternion')
            qp, qv = np.tile(root, (2, 1)), np.zeros((2, 6))
        elif traj_loader is not None:
            # training mode (fly_envs.py:131-135): the whole dataset lives on the GPU, every environment picks its snippet there
            ds = traj_loader.dataset
            jid, sid = ds.ids(arrays)
            self.task._traj_generator = traj_loader
            self.batch.set_walk_dataset(ds, jid, sid, select=traj_loader.traj_indices, future_steps=future_steps,
                                        terminal_com_dist=terminal_com_dist, time_limit=time_limit, seed=seed, env_id_base=env_id_base)
            qp = qv = None
        else:
            qp, qv = default_walking_reference()
        if qp is not None:
            self.task._traj_generator.set_next_trajectory(qp, qv)
        self.layout, self.nobs = observation_layout(self.model, future_steps, ball=(task == 'walk_on_ball'))
        self._torch_views = None
        self.control_callback = control_callback
        self.reward_fn, self.termination_fn, self.action_corruptor = reward_fn, termination_fn, action_corruptor
        self.random_state = random_state if random_state is not None else np.random.RandomState(seed)
        self._force_views = None; self._law_views = None; self._end_args = None; self._state_views = None
        self._model_view = None; self._model_gen = None; self._seed = seed
        self._eye_cache = {}                                  # eye_depth: (size, fovy, see_body) -> (rays on the device, head body, geom mask)
        if (env_model is not None or resample_on_reset) and models is None:
            raise ValueError('env_model / resample_on_reset need models=[...]')
        self.resample_on_reset = bool(resample_on_reset)
        if env_model is not None:
            self.batch.set('ENV_MODEL', np.asarray(env_model, np.int32).reshape(n_env, 1))

    def _apply_reference(self):
        s = self.task._traj_generator._snippet
        if self.task_name == 'flight_imitation':
            # the flight loaders hand over a CoM trajectory; the task converts it to the root joint
            # (set_next_trajectory re-centres x,y: trajectory_loaders.py:172-173; com2root: flight_imitation.py:93-99)
            from .task_utils import com2root
            q = s['qpos'].copy(); q[:, :2] -= q[0, :2]
            quat = q[:, 3:7] / np.linalg.norm(q[:, 3:7], axis=1, keepdims=True)
            q[:, :3] = com2root(q[:, :3], quat, offset=self.model.arrays['com_offset'])
            s = {'qpos': q, 'qvel': s['qvel']}
        self.batch.set_reference(s['qpos'], s['qvel'], future_steps=self.future_steps,
                                 terminal_com_dist=self.terminal_com_dist, time_limit=self.time_limit)
        self._torch_views = None

    # ---- specs --------------------------------------------------------------------------------
    def action_spec(self) -> BoundedArray:
        return action_spec_from_arrays(self.model.arrays)

    def observation_spec(self):
        return collections.OrderedDict(('walker/' + k, Array(self.layout[k][2], np.float32, 'walker/' + k)) for k in self._keys())

    def _keys(self):
        return [k for k in _DICT_ORDER if self.layout[k][1] > 0 or k == 'actuator_activation']

    def control_timestep(self) -> float:
        return float(self.model.arrays['opt_control_timestep'])

    # ---- torch interface (zero-copy views of the engine's device buffers) -----------------------
    def torch_views(self):
        if self._torch_views is None:
            view = self.batch.device_view
            self._torch_views = dict(obs=view('OBS'), reward=view('REWARD').view(self.n_env), discount=view('DISCOUNT').view(self.n_env),
                                     step_type=view('STEP_TYPE').view(self.n_env))
        return self._torch_views

    def state_views(self):
        """Zero-copy torch views dict(qpos=[n_env, nq], qvel=[n_env, nv]) of the physics state at the batch's precision, for rewards and
        terminations computed on the device (reward_fn / termination_fn).  They are strided windows of the engine's arena: read them
        after a step; writing between steps is Batch.set without its checks."""
        if self._state_views is None:
            self._state_views = dict(qpos=self.batch.device_view('QPOS'), qvel=self.batch.device_view('QVEL'))
        return self._state_views

    def applied_forces(self):
        """Zero-copy torch views of the engine's external-force inputs, MuJoCo's qfrc_applied and xfrc_applied:
        dict(qfrc_applied=[n_env, nv], xfrc_applied=[n_env, nbody, 6]) at the batch's precision (float64 / float32); a body's row is
        force(3) then torque(3) in the world frame, applied at its centre of mass; the world body's row is ignored.  The first call
        allocates the arrays (zeroed) and puts the batch on the step kernel that reads them, every substep (Batch.forces_active).
        They are caller-owned inputs like the actions: they persist until changed and an auto-reset does NOT clear them (MuJoCo's
        reset does); the host-side reset() zeroes them.  perturbations.clear(env) frees them."""
        if not self.batch.forces_active:                  # freed behind our back (Batch.clear_forces): earlier views point at freed memory
            self._force_views = None
        if self._force_views is None:
            self._force_views = dict(qfrc_applied=self.batch.device_view('QFRC_APPLIED'),
                                     xfrc_applied=self.batch.device_view('XFRC_APPLIED').view(self.n_env, self.model.dim('nbody'), 6))
        return self._force_views

    def env_model(self):
        """Zero-copy int32 torch view [n_env] of the model index every environment is stepped with (FB_ENV_MODEL; needs models=[...]).
        The engine reads it when it picks an environment up; change an entry at an episode boundary only -- before a reset of that
        environment, or while its step type is LAST (resample_on_reset does the latter)."""
        if self._model_view is None:
            self._model_view = self.batch.device_view('ENV_MODEL').view(self.n_env)
        return self._model_view

    def _resample_models(self):
        """resample_on_reset: environments that just returned LAST get a new model id for the episode their auto-reset starts."""
        import torch
        if self._model_gen is None:
            self._model_gen = torch.Generator(device=f'cuda:{self.device}'); self._model_gen.manual_seed(int(self._seed))
        em = self.env_model()
        new = torch.randint(0, self.batch.n_models, (self.n_env,), generator=self._model_gen, device=em.device, dtype=torch.int32)
        em.copy_(torch.where(self.torch_views()['step_type'] == int(StepType.LAST), new, em))

    def clear_forces(self):
        """Free the applied-force arrays and return the batch to the plain step kernel; earlier applied_forces() views are dropped."""
        self._force_views = None
        self.batch.clear_forces()

    # ---- substep control law (flybody_amd.control_laws, csrc/fb_law.hpp) ------------------------
    def set_control_law(self, law):
        """Feedback at the physics rate: `law` (control_laws.ControlLaw, rows [nv] or [n_env, nv]) is evaluated by the step kernel in
        every substep, with that substep's actuator force.  The batch is stepped by the kernel that carries the law stage from now on."""
        self._law_views = None
        self.batch.set_control_law(**law.rows())

    def control_law(self):
        """Zero-copy torch views of the law on the device: the five rows bias / act_gain / pos_gain / pos_ref / vel_gain, each [n_rows, nv]
        at the batch's precision -- write per-environment gains between steps without a host copy (pos_gain stays zero on dofs that are
        no hinge's; values written here are not validated) -- and qfrc_law [n_env, nv], the law's force in the last substep (read-only)."""
        if not self.batch.control_law_active:
            raise engine.EngineError('no control law is set (set_control_law)')
        if self._law_views is None:
            block = self.batch.device_view('CONTROL_LAW').view(self.batch.control_law_rows, len(engine.LAW_ROWS), self.model.dim('nv'))
            self._law_views = dict({k: block[:, r] for r, k in enumerate(engine.LAW_ROWS)}, qfrc_law=self.batch.device_view('QFRC_LAW'))
        return self._law_views

    def clear_control_law(self):
        """Remove the law; earlier control_law() views are dropped.  The batch returns to the kernel it had before the law."""
        self._law_views = None
        self.batch.clear_control_law()
        if not self.batch.forces_active:
            self._force_views = None

    # ---- transition derivatives (flybody_amd.derivatives, csrc/fb_deriv.hpp) ---------------------
    def linearize(self, env_ids=None, **kw):
        """Linearise live environments between two control steps without disturbing them: engine.TransitionFD(A, B, C, D, status) of one
        physics substep (or n_substeps=...) around each listed environment's current state and held ctrl, as torch FP64 tensors on the
        device (Batch.transition_fd: eps, centered, n_substeps, sensors, want_A, want_B, pool_rows, stream).  The environments are only
        read -- the steps that follow are bit-identical to those of an environment that was never linearised.  The constraint solves
        warm-start from the acceleration the environment's next substep would start from.  FP64 batches without applied forces or a
        control law."""
        return self.batch.transition_fd(env_ids=env_ids, **kw)

    def lqr_gains(self, lin, Q, R, horizon, mu=None):
        """Stationary LQR gains around the linearisations `lin` = env.linearize(ids, ...), one model per listed environment, without
        leaving the device (Batch.lqr_backward in stationary mode: `horizon` Riccati steps from the terminal weight Q).  Q [ndx, ndx],
        R [nu, nu] (numpy or torch), mu [n] (None: no regularisation).  Returns engine.LQRBackward with P = (P_0, P_1) -- their
        difference tells convergence -- and K [n, 1, nu, ndx]: K.expand(-1, T, -1, -1).contiguous() is the gain of
        env.rollout(feedback=engine.Feedback(x_nom, u_nom, K)) over T intervals of the substeps `lin` was taken over."""
        import torch
        if lin.A is None or lin.B is None:
            raise ValueError('lqr_gains needs both A and B of the linearisation')
        dev = lin.A.device
        on = lambda x: None if x is None else torch.as_tensor(np.asarray(x, np.float64) if not isinstance(x, torch.Tensor) else x, dtype=torch.float64,
                                                              device=dev).contiguous()
        return self.batch.lqr_backward(lin.A.contiguous(), lin.B.contiguous(), on(Q), on(R), mu=on(mu), stationary=True, horizon=int(horizon),
                                       want_P=True)

    # ---- open-loop rollouts (flybody_amd.rollout, csrc/fb_rollout.hpp) ---------------------------
    def rollout(self, action=None, ctrl=None, env_ids=None, feedback=None, samples=None, **kw):
        """What happens if these inputs are applied from here?  Open-loop rollouts from live environments between two control steps,
        without disturbing them: engine.Rollout(state, qpos, qvel, act, sensordata, status) as torch tensors on the device
        (Batch.rollout: n_substeps, sensors, pool_rows, stream).  action: float32 [n, T, nact], one row per control step, through the
        task's before_step hook as step_tensor's actions go (for the flight task the wing-beat pattern generator advances inside the
        rollout); or ctrl: float64 [n, T, nu], the actuators' controls themselves.  Rollout r starts from environment env_ids[r] (None:
        r).  With a sample axis, [n_env_ids, K, T, .], every listed environment (None: all of them) gets K rollouts and the outputs
        come back as [n_env_ids, K, T, .] (status: [n_env_ids, K]).
        Modelled: the physics of T control steps and the action-to-control mapping.  NOT modelled: reward, termination and auto-reset
        (a rollout runs on through what would end the episode, and one from an environment at LAST continues its physics), the
        action corruptor, control_callback, reward_fn / termination_fn.  The environments are only read -- the steps that follow are
        bit-identical to those of an environment that never ran a rollout.  FP64 batches without applied forces or a control law.
        feedback=engine.Feedback(x_nom, u_nom, K, k, alpha): CLOSED-LOOP rollouts instead (Batch.rollout_feedback; neither action nor
        ctrl is given then) -- one nominal per listed environment, x_nom [n_env_ids, T, nx], u_nom / k [n_env_ids, T, nu],
        K [n_env_ids, T, nu, ndx]; rollout r of environment env_ids[r] follows nominal r.  samples=K gives every listed environment K
        rollouts that share its nominal, alpha [n_env_ids, K] (the step lengths of a line search), and the outputs come back as
        [n_env_ids, K, T, .]; the result carries ctrl, the inputs applied."""
        if feedback is not None:
            return self._rollout_feedback(engine.Feedback(*feedback), action, ctrl, env_ids, samples, **kw)
        x = action if action is not None else ctrl
        if x is None or x.dim() != 4:
            return self.batch.rollout(ctrl=ctrl, action=action, env_ids=env_ids, **kw)
        ne, K = int(x.shape[0]), int(x.shape[1])
        ids = engine.as_env_ids(env_ids, self.n_env)
        if len(ids) != ne:
            raise ValueError(f'the leading axis of the inputs ({ne}) must match the environments listed ({len(ids)})')
        flat = x.reshape(ne*K, x.shape[2], x.shape[3])
        return self._per_sample(ids, K, self.batch.rollout, ctrl=None if action is not None else flat, action=flat if action is not None else None, **kw)

    @staticmethod
    def _per_sample(ids, K, call, *args, **kw):
        """The sample axis: `call` runs K rollouts from every listed environment, rollout e K + s being sample s of ids[e], and its
        outputs [ne K, ...] come back as [ne, K, ...]."""
        r = call(*args, env_ids=np.repeat(ids, K), **kw)
        return engine.Rollout(*(None if t is None else t.reshape((len(ids), K) + tuple(t.shape[1:])) for t in r))

    def _rollout_feedback(self, fbk, action, ctrl, env_ids, samples, **kw):
        if action is not None or ctrl is not None:
            raise ValueError('a closed-loop rollout computes its inputs: give feedback alone, without action or ctrl')
        if fbk.nom_ids is not None:
            raise ValueError('the nominal of a rollout is its environment here (nominal r for env_ids[r]): leave Feedback.nom_ids None')
        ids = engine.as_env_ids(env_ids, self.n_env)
        ne = len(ids)
        if int(fbk.x_nom.shape[0]) != ne:
            raise ValueError(f'the leading axis of the nominals ({int(fbk.x_nom.shape[0])}) must match the environments listed ({ne})')
        if samples is None and (fbk.alpha is None or fbk.alpha.dim() == 1):
            return self.batch.rollout_feedback(fbk.x_nom, fbk.u_nom, fbk.K, fbk.k, fbk.alpha, env_ids=ids, **kw)
        K = int(samples) if samples is not None else int(fbk.alpha.shape[1])
        if K < 1 or (fbk.alpha is not None and tuple(fbk.alpha.shape) != (ne, K)):
            raise ValueError(f'alpha must be [{ne}, {K}]: one step length per sample of every listed environment')
        return self._per_sample(ids, K, self.batch.rollout_feedback, fbk.x_nom, fbk.u_nom, fbk.K, fbk.k,
                                None if fbk.alpha is None else fbk.alpha.reshape(ne*K), nom_ids=np.repeat(np.arange(ne, dtype=np.int32), K), **kw)

    # ---- ray casting (flybody_amd.vision, csrc/fb_ray.hpp) --------------------------------------
    def cast_rays(self, rays, **kw):
        """Rays against the live environments' geoms and an optional vision.Terrain, between two control steps and without disturbing
        them: engine.RayResult(dist, geomid) as torch tensors on the device (Batch.cast_rays: body, env_ids, geom_mask, bodyexclude,
        cutoff, terrain, terrain_ids, stream).  Range sensors, height above terrain, depth images."""
        return self.batch.cast_rays(rays, **kw)

    def eye_depth(self, size: int = 32, fovy: float = 150.0, terrain=None, terrain_ids=None, cutoff: Optional[float] = None,
                  see_body: bool = False):
        """Depth images of the fly's two eye cameras (vision.EYES, on the `head` body; the vision task's fovy 150 and 32 x 32 pixels):
        float32 [n_env, 2, size, size] on the device, in the order eye_right, eye_left, row 0 at the top; the distance along each
        pixel's ray, -1 where it meets nothing (or nothing within `cutoff`).  Both eye origins lie inside the head's collision geoms,
        so by default every geom of the fly is hidden and the eyes see the floor, other bodies and the terrain; see_body=True hides
        only the head's own geoms.  terrain_ids [n_env]: the grid of every environment (None: grid 0)."""
        from . import vision
        a = self.model.arrays
        # (the mask and the head's id come from names_body / geom_bodyid / body_rootid: integer tables, which every model of a group shares with
        #  the first one -- fb_batch_create_group refuses anything else -- so env_model() and resampling cannot invalidate the cache)
        key = (int(size), float(fovy), bool(see_body))
        cache = self._eye_cache
        if key not in cache:
            import torch
            names = [str(n) for n in a['names_body']]
            head, gbody, root = names.index('head'), np.asarray(a['geom_bodyid']), np.asarray(a['body_rootid'])
            hidden = (gbody == head) if see_body else (root[gbody] == root[head])
            rays = np.concatenate([vision.camera_rays(fovy, size, size, pos, quat) for pos, quat in vision.EYES.values()])
            cache[key] = (torch.from_numpy(rays).to(self.batch._torch_device()), head, ~hidden)
        rays, head, mask = cache[key]
        r = self.batch.cast_rays(rays, body=head, geom_mask=mask, cutoff=cutoff, terrain=terrain, terrain_ids=terrain_ids)
        return r.dist.reshape(self.n_env, 2, int(size), int(size))

    # ---- the parts of a control step around the kernel ------------------------------------------
    @property
    def _hooks_after(self) -> bool:
        return self.reward_fn is not None or self.termination_fn is not None or self.resample_on_reset

    def _corrupt(self, action):
        if self.action_corruptor is not None:
            action = self.action_corruptor(action, self.random_state)
        return action

    def _after_kernel(self, stream):
        """reward_fn, termination_fn + end_episode, model resampling: torch ops and one small kernel on the step's stream, no host sync."""
        import torch
        v = self.torch_views()
        if self.reward_fn is not None:
            r = self.reward_fn(self).to(torch.float32)
            v['reward'].copy_(torch.where(v['step_type'] == int(StepType.FIRST), torch.zeros_like(r), r))
        if self.termination_fn is not None:
            t = self.termination_fn(self)
            t, disc = t if isinstance(t, tuple) else (t, None)
            mask = t.to(torch.uint8).contiguous()
            disc = None if disc is None else disc.to(torch.float32).contiguous()
            if tuple(mask.shape) != (self.n_env,) or (disc is not None and tuple(disc.shape) != (self.n_env,)):
                raise ValueError(f'termination_fn must return a bool tensor [{self.n_env}], or (that, a discount tensor [{self.n_env}]); got '
                                 f'{tuple(mask.shape)}' + ('' if disc is None else f' and {tuple(disc.shape)}'))
            self._end_args = (mask, disc)
            self.batch.end_episode(mask.data_ptr(), 0 if disc is None else disc.data_ptr(), stream)
        if self.resample_on_reset:
            self._resample_models()

    def reset_all(self):
        import torch
        self.batch.reset(stream=torch.cuda.current_stream().cuda_stream)
        self._time = 0.0
        return self.torch_views()

    def step_tensor(self, action):
        """action: float32 CUDA tensor [n_env, nu] (contiguous).  Asynchronous on torch's current stream."""
        import torch
        assert action.is_cuda and action.dtype == torch.float32 and action.is_contiguous()
        assert tuple(action.shape) == (self.n_env, self.model.dim('nact'))
        if self.control_callback is not None:
            self.control_callback(self)
        if self.action_corruptor is not None:
            action = self._corrupt(action).to(torch.float32).contiguous()
        self.task.prev_action = action
        stream = torch.cuda.current_stream().cuda_stream
        self.batch.step_ptr(action.data_ptr(), stream)
        if self._hooks_after:
            self._after_kernel(stream)
        self._time += self.control_timestep()
        return self.torch_views()

    # ---- dm_env-style host interface ----------------------------------------------------------
    def _timestep(self, env: int = 0) -> TimeStep:
        obs = self.batch.get('OBS')[env]
        st = StepType(int(self.batch.get('STEP_TYPE')[env, 0]))
        od = collections.OrderedDict()
        for k in self._keys():
            off, n, shp = self.layout[k]
            od['walker/' + k] = obs[off:off + n].reshape(shp).copy()
        if st == StepType.FIRST:
            return TimeStep(st, None, None, od)
        return TimeStep(st, float(self.batch.get('REWARD')[env, 0]), float(self.batch.get('DISCOUNT')[env, 0]), od)

    def reset(self) -> TimeStep:
        if self.batch.forces_active:                      # MuJoCo's reset clears the applied forces; the engine leaves that to its caller
            import torch
            torch.cuda.synchronize()
            for t in self.applied_forces().values():
                t.zero_()
            torch.cuda.synchronize()
        self.batch.reset(); self.batch.synchronize()
        self._time = 0.0
        return self._timestep()

    def step(self, action) -> TimeStep:
        import torch
        a = np.broadcast_to(np.asarray(action, np.float32), (self.n_env, self.model.dim('nact')))
        if self.control_callback is not None:
            self.control_callback(self)
        a = np.array(self._corrupt(a), np.float32, copy=True)
        self.task.prev_action = a
        t = torch.from_numpy(a).to(f'cuda:{self.device}')
        stream = torch.cuda.current_stream().cuda_stream
        self.batch.step_ptr(t.data_ptr(), stream)
        if self._hooks_after:
            self._after_kernel(stream)
        torch.cuda.synchronize()
        ts = self._timestep()
        self._time = 0.0 if ts.first() else self._time + self.control_timestep()
        return ts


def walk_imitation(ref_path: Optional[str] = None, force_actuators: bool = False, disable_wings: bool = True,
                   traj_indices: Optional[Sequence[int]] = None, random_state=None, terminal_com_dist: float = 0.3,
                   joint_filter: float = 0.01, n_env: int = 1, device: int = 0, precision: int = 64, seed: int = 0,
                   env_id_base: int = 0, models=None, env_model=None, resample_on_reset: bool = False) -> BatchedFlyEnv:
    """Same keyword surface as flybody/fly_envs.py:100-106, plus n_env / device / precision / seed / env_id_base and the
    per-environment models of BatchedFlyEnv (models / env_model / resample_on_reset).

    ref_path: the reference's hdf5 walking dataset (needs h5py) or its .npz conversion (trajectory_loaders.WalkingDataset.save),
    or an already constructed loader; None = inference mode (reward == 1)."""
    traj_loader = None
    if ref_path is not None:
        from .trajectory_loaders import ArrayWalkingTrajectoryLoader, HDF5WalkingTrajectoryLoader
        if hasattr(ref_path, 'dataset'):
            traj_loader = ref_path
        elif str(ref_path).endswith('.npz'):
            traj_loader = ArrayWalkingTrajectoryLoader(str(ref_path), traj_indices=traj_indices, random_state=random_state)
        else:
            traj_loader = HDF5WalkingTrajectoryLoader(str(ref_path), traj_indices=traj_indices, random_state=random_state)
    return BatchedFlyEnv(n_env=n_env, device=device, precision=precision, terminal_com_dist=terminal_com_dist,
                         joint_filter=joint_filter, future_steps=64, time_limit=10.0, seed=seed, traj_loader=traj_loader,
                         env_id_base=env_id_base, force_actuators=force_actuators, use_wings=not disable_wings,
                         models=models, env_model=env_model, resample_on_reset=resample_on_reset)


def walk_on_ball(force_actuators: bool = False, disable_wings: bool = True, random_state=None, n_env: int = 1, device: int = 0,
                 precision: int = 64, seed: int = 0, models=None, env_model=None, resample_on_reset: bool = False) -> BatchedFlyEnv:
    """Tethered fly walking on a floating ball: same keyword surface as flybody/fly_envs.py:158-191, plus n_env / device /
    precision and the per-environment models of BatchedFlyEnv.  Observation = the walker observables + `ball_qvel`; reward = product of linear tolerances on the ball's
    angular velocity around the target (0, -5, 0) rad/s (tasks/walk_on_ball.py:62-73); 2 s episodes."""
    return BatchedFlyEnv(n_env=n_env, device=device, precision=precision, terminal_com_dist=float('inf'), joint_filter=0.01,
                         future_steps=0, time_limit=2.0, task='walk_on_ball', force_actuators=force_actuators,
                         use_wings=not disable_wings, seed=seed, models=models, env_model=env_model, resample_on_reset=resample_on_reset)


def template_task(random_state=None, force_actuators: bool = False, disable_wings: bool = True, joint_filter: float = 0.01,
                  adhesion_filter: float = 0.007, time_limit: float = 1.0, mjcb_control=None, observables_options=None,
                  action_corruptor=None, claw_friction: float = 1.0, n_env: int = 1, device: int = 0, precision: int = 64, seed: int = 0,
                  init_qpos=None, reward_fn=None, termination_fn=None) -> BatchedFlyEnv:
    """The starting point for a walking task of your own: same keyword surface as flybody/fly_envs.py:194-247, plus n_env / device /
    precision / seed, init_qpos (the root pose [7] an episode starts from; default: standing at z = 0.1278) and the PyTorch hooks
    reward_fn / termination_fn of BatchedFlyEnv.  The kernel's own task returns reward 1 and ends an episode at the time limit or on
    a physics error; the observation is the walker's ten observables.
    mjcb_control: a control_laws.ControlLaw, evaluated in every physics substep (BatchedFlyEnv.set_control_law).  A Python callable
    cannot run inside the step kernel: it raises TypeError; BatchedFlyEnv(control_callback=f) runs one once per control step."""
    from .control_laws import ControlLaw
    if observables_options is not None:
        raise NotImplementedError('template_task: observables_options is not supported (the observation layout is compiled into the kernel)')
    if mjcb_control is not None and not isinstance(mjcb_control, ControlLaw):
        raise TypeError('template_task: mjcb_control takes a flybody_amd.control_laws.ControlLaw, which the step kernel evaluates in every '
                        'physics substep; a Python callable cannot run there -- pass it as control_callback to BatchedFlyEnv (or set '
                        'env.control_callback), which runs it once per control step')
    env = BatchedFlyEnv(n_env=n_env, device=device, precision=precision, terminal_com_dist=float('inf'), joint_filter=joint_filter,
                        future_steps=0, time_limit=time_limit, task='template_task', force_actuators=force_actuators,
                        use_wings=not disable_wings, adhesion_filter=adhesion_filter, seed=seed, claw_friction=claw_friction,
                        init_qpos=init_qpos, reward_fn=reward_fn, termination_fn=termination_fn, action_corruptor=action_corruptor,
                        random_state=random_state)
    if mjcb_control is not None:
        env.set_control_law(mjcb_control)
    return env


def flight_imitation(ref_path: Optional[str] = None, wpg_pattern_path: Optional[str] = None, force_actuators: bool = False,
                     disable_legs: bool = True, traj_indices: Optional[Sequence[int]] = None, randomize_start_step: bool = True,
                     joint_filter: float = 0.0, future_steps: int = 5, random_state=None, terminal_com_dist: float = 2.0,
                     n_env: int = 1, device: int = 0, precision: int = 64, seed: int = 0, env_id_base: int = 0, dense=None,
                     models=None, env_model=None, resample_on_reset: bool = False) -> BatchedFlyEnv:
    """Same keyword surface as flybody/fly_envs.py:30-39, plus n_env / device / precision / seed / env_id_base / dense (engine build)
    and the per-environment models of BatchedFlyEnv (models / env_model / resample_on_reset).

    ref_path: the reference's hdf5 flight dataset (needs h5py), its .npz conversion (trajectory_loaders.FlightDataset.save) or an
    already constructed loader; None = InferenceFlightTrajectoryLoader (the synthetic straight flight)."""
    traj_loader = None
    if ref_path is not None:
        from .trajectory_loaders import ArrayFlightTrajectoryLoader, HDF5FlightTrajectoryLoader
        if hasattr(ref_path, 'dataset'):
            traj_loader = ref_path
        elif str(ref_path).endswith('.npz'):
            traj_loader = ArrayFlightTrajectoryLoader(str(ref_path), traj_indices=traj_indices, randomize_start_step=randomize_start_step,
                                                      random_state=random_state)
        else:
            traj_loader = HDF5FlightTrajectoryLoader(str(ref_path), traj_indices=traj_indices, randomize_start_step=randomize_start_step,
                                                     random_state=random_state)
    tables = None
    if wpg_pattern_path is not None:
        from .wbpg import build_tables
        tables = build_tables(np.load(wpg_pattern_path))
    return BatchedFlyEnv(n_env=n_env, device=device, precision=precision, terminal_com_dist=terminal_com_dist,
                         joint_filter=joint_filter, future_steps=future_steps, time_limit=0.6, task='flight_imitation',
                         wbpg_tables=tables, seed=seed, traj_loader=traj_loader, env_id_base=env_id_base,
                         force_actuators=force_actuators, use_legs=not disable_legs, dense=dense,
                         models=models, env_model=env_model, resample_on_reset=resample_on_reset)
