"""Thin ctypes shim over the C-ABI of libflybody_hip.so (include/flybody_engine.h).

The product path is HIP only: `load_library()` opens ``flybody_amd/libflybody_hip.so`` and every
entry point fails loudly if the library or a GPU is missing -- there is no CPU fallback.
(`lib_path` exists so the test-suite can point the same shim at the kernel-emulation build under
tests/_emu; nothing in the package does that.)
"""
from __future__ import annotations

import collections
import ctypes as C
import os
from typing import Dict, Optional

import numpy as np

from .model_blob import load_npz, pack_model

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB = os.path.join(_HERE, 'libflybody_hip.so')
# Same sources built with -DFB_F64_DENSE=1: 12 instead of 8 FP64 environments per CU (smaller LDS Delassus matrix, 168-VGPR
# stages; a longer per-environment chain, more of them resident).  With the substep scheduler (batches beyond the resident slots
# are handed out per substep, fb_engine.hip) it is the faster FP64 build for large batches -- 4096 walking environments in
# lock-step: 8.2 ms against 9.0 -- and the slower one for batches that fit the default build's 2048 slots.
# Model(..., dense=True); fly_envs picks it for FP64 batches of more than 2048 ground-contact environments unless told otherwise.
HIP_LIB_DENSE = os.path.join(_HERE, 'libflybody_hip_dense.so')
ASSETS = os.path.join(_HERE, 'assets')

MAXCON, MAXEFC, NSENSOR = 64, 192, 33
# fields (include/flybody_engine.h): name -> (id, dtype, width of an environment's row).  A width is a number, a model dimension
# (Model.dim; 'nobs': Batch.nobs) or a (factor, dimension) pair.  fb_batch_get returns physics fields as FP64 at either precision.
_F64, _F32, _I32 = np.float64, np.float32, np.int32
FIELDS = dict(
    QPOS=(0, _F64, 'nq'), QVEL=(1, _F64, 'nv'), ACT=(2, _F64, 'na'), CTRL=(3, _F64, 'nu'), QACC=(4, _F64, 'nv'),
    XPOS=(5, _F64, (3, 'nbody')), XQUAT=(6, _F64, (4, 'nbody')), SENSORDATA=(7, _F64, NSENSOR), OBS=(8, _F32, 'nobs'),
    REWARD=(9, _F32, 1), DISCOUNT=(10, _F32, 1), STEP_TYPE=(11, _I32, 1), NCON=(12, _I32, 1), NEFC=(13, _I32, 1),
    SOLVER_NITER=(14, _I32, 1), QFRC_BIAS=(15, _F64, 'nv'), QFRC_PASSIVE=(16, _F64, 'nv'), QACC_SMOOTH=(17, _F64, 'nv'),
    QM=(18, _F64, 'nM'), CONTACT=(19, _F64, MAXCON*8), EFC_FORCE=(20, _F64, MAXEFC), QFRC_ACTUATOR=(21, _F64, 'nv'),
    QFRC_CONSTRAINT=(22, _F64, 'nv'), STEP_COUNT=(23, _I32, 1), SUBTREE_COM=(24, _F64, 3), PROF=(25, _I32, 112),
    REWARD_FACTORS=(26, _F64, 5), GEOM_XPOS=(27, _F64, (3, 'ngeom')), GEOM_XMAT=(28, _F64, (9, 'ngeom')), CVEL=(29, _F64, (6, 'nbody')),
    STEP_TICKS=(30, _I32, 1), LAUNCH_ORDER=(31, _I32, 1), WARN=(32, _I32, 1), WARN_EVER=(33, _I32, 1), SIZE_STATS=(34, _I32, 4),
    SITE_XPOS=(35, _F64, (3, 'nsite')), IK_ERR=(36, _F64, 2), IK_STEPS=(37, _I32, 2), QFRC_INVERSE=(38, _F64, 'nv'),
    CONTACT_FORCE=(39, _F64, 3*MAXCON), QFRC_APPLIED=(40, _F64, 'nv'), XFRC_APPLIED=(41, _F64, (6, 'nbody')), ENV_MODEL=(42, _I32, 1),
    QFRC_LAW=(43, _F64, 'nv'), CONTROL_LAW=(44, _F64, (5, 'nv')), TIME=(45, _F64, 1))
TASK_IDS = dict(walk_imitation=0, flight_imitation=1, walk_on_ball=2, template_task=3)      # FB_TASK_* (csrc/fb_types.hpp)
LAW_ROWS = ('bias', 'act_gain', 'pos_gain', 'pos_ref', 'vel_gain')                          # rows of CONTROL_LAW (csrc/fb_law.hpp)
# bits of WARN / WARN_EVER (include/flybody_engine.h): the caps MuJoCo reports as nconmax / njmax warnings, and iteration limits
WARN_BITS = dict(CONTACT_CAP=1, EFC_CAP=2, SOLVER_MAXITER=4, CCD_MAXITER=8, SCHED_WAIT=16, SOLVER_FALLBACK=32, MODEL_ID=64)

# fb_step.hpp stage ids (ST_*) and the stage sequence of one control step as d_run walks it (profiling: fb_batch_stage)
ST = dict(ACT=0, ACC_PRE=1, SOLVE=2, ACC_SOLVE=3, ACC_POST=4, CONSTR_A=5, CONSTR_B=6, SENS=7, EULER_PRE=8, FACTOR=9, EULER_SOLVE=10,
          EULER_POST=11, KIN=12, COLL=13, SUBEND=14, PRE=32, POST=33)


def stage_sequence(nsubstep: int):
    """[(name, stage word)] of one control step: the task's before_step hook, `nsubstep` x (mj_step2, integration, mj_step1 in
    dm_control's legacy order, fb_step.hpp d_run), the task's after_step hook.  smooth_rhs / euler_rhs / substep_end keep their places in the
    walk, but the passes they were named after run inside factor_M / factor_M_hD / velocity (tools/stage_profile.py)."""
    DAMP, HALF, P = 1 << 8, 1 << 9, lambda m: m << 12
    sub = [('actuation', ST['ACT']), ('smooth_rhs', ST['ACC_PRE']), ('factor_M', ST['FACTOR']), ('solve_smooth', ST['SOLVE'] | HALF),
           ('qacc_smooth_copy', ST['ACC_POST'] | P(1)), ('project_constraint', ST['ACC_POST'] | P(2)), ('constraint_solve', ST['CONSTR_A']),
           ('solve_constraint', ST['SOLVE']), ('qacc', ST['CONSTR_B']), ('sensor_acc', ST['SENS']), ('euler_rhs', ST['EULER_PRE']),
           ('factor_M_hD', ST['FACTOR'] | DAMP), ('solve_euler', ST['SOLVE'] | HALF), ('integrate', ST['EULER_POST']),
           ('kinematics', ST['KIN'] | P(1)), ('com_pos', ST['KIN'] | P(2)), ('crb', ST['KIN'] | P(4)), ('collision', ST['COLL'] | P(1)),
           ('make_constraint', ST['COLL'] | P(2)), ('velocity', ST['COLL'] | P(4)), ('substep_end', ST['SUBEND'])]
    return [('task_pre', ST['PRE'])] + sub*nsubstep + [('task_post', ST['POST'])]


# Batch.transition_fd / derivatives.transition_fd: the Jacobians of one transition (None: not asked for) and the frames' warning bits
TransitionFD = collections.namedtuple('TransitionFD', ['A', 'B', 'C', 'D', 'status'])

# Batch.rollout / BatchedFlyEnv.rollout: state [n, T, nq + nv + na] and its views qpos / qvel / act, sensordata [n, T, 33] (None: not asked
# for) and the rollouts' warning bits [n]
Rollout = collections.namedtuple('Rollout', ['state', 'qpos', 'qvel', 'act', 'sensordata', 'status', 'ctrl'], defaults=(None,))
# ... and of a closed-loop one (Batch.rollout_feedback) ctrl [n, T, nu], the inputs the feedback law applied (an open-loop rollout: None)

# The feedback law of a closed-loop rollout, u_t = clamp(u_nom[t] + alpha k[t] + K[t] (x_t (-) x_nom[t])): the arguments of
# Batch.rollout_feedback as one value, for BatchedFlyEnv.rollout(feedback=...) and rollout.rollout(feedback=...)
Feedback = collections.namedtuple('Feedback', ['x_nom', 'u_nom', 'K', 'k', 'alpha', 'nom_ids'], defaults=(None, None, None, None))

# Batch.lqr_backward: the gains K [n_nom, T, nu, ndx] (a transposed view of the Kt the kernel wrote: K.transpose(2, 3) is contiguous and is
# what Batch.rollout_feedback streams, without a copy), k [n_nom, T, nu], the value's P [n_nom, T + 1, ndx, ndx] and p [n_nom, T + 1, ndx]
# (None: not asked for), the predicted change of the cost dV [n_nom, 2] and status [n_nom] (0, or 1 + the interval whose Quu + mu I was
# not positive definite); in stationary mode the time axes are 1 (K, k) and 2 (P, p)
LQRBackward = collections.namedtuple('LQRBackward', ['K', 'k', 'P', 'p', 'dV', 'status'])

# Batch.cast_rays: dist float32 [n_frames, n_ray], in units of |dir| (-1: a miss), and geomid int32 [n_frames, n_ray] (-1: a miss; ngeom: the
# terrain)
RayResult = collections.namedtuple('RayResult', ['dist', 'geomid'])

# The C prototypes of include/flybody_engine.h as (restype, argtypes), in the header's order; tests/test_abi.py checks every entry
# against the header.  Handles, arrays, streams and structs passed by reference are c_void_p; an out-parameter filled through byref() is a
# POINTER of its scalar.
_P, _I, _D, _Z = C.c_void_p, C.c_int, C.c_double, C.c_size_t
_SIGNATURES = {
    'fb_model_dim': (_I, [_P, C.c_char_p]),
    'fb_model_load': (_I, [_P, _Z, C.POINTER(_P)]),
    'fb_model_destroy': (None, [_P]),
    'fb_batch_create': (_I, [_P, _I, _I, _I, C.POINTER(_P)]),
    'fb_batch_destroy': (None, [_P]),
    'fb_batch_set_reference': (_I, [_P, _P, _P, _I, _I, _D, _D]),
    'fb_batch_set_time_limit': (_I, [_P, _D]),
    'fb_batch_set_wbpg': (_I, [_P, _P, _P, _P, _P, _I, _D, _D, _D, C.c_uint32]),
    'fb_batch_set_walk_dataset': (_I, [_P, _P]),
    'fb_batch_set_flight_dataset': (_I, [_P, _P]),
    'fb_batch_reset': (_I, [_P, _P, _I, _P]),
    'fb_batch_step': (_I, [_P, _P, _P]),
    'fb_batch_substep': (_I, [_P, _I, _P]),
    'fb_batch_forward': (_I, [_P, _P]),
    'fb_batch_stage': (_I, [_P, _I, _P, _P]),
    'fb_batch_row': (_I, [_P, _I, _I, _P, _Z, _I, C.POINTER(_Z)]),
    'fb_batch_get': (_I, [_P, _I, _P, _Z]),
    'fb_batch_set': (_I, [_P, _I, _P, _Z]),
    'fb_batch_device_ptr': (_P, [_P, _I]),
    'fb_batch_synchronize': (_I, [_P, _P]),
    'fb_batch_timing_begin': (_I, [_P, _P]),
    'fb_batch_timing_end': (_I, [_P, _P, C.POINTER(C.c_float), C.POINTER(_I)]),
    'fb_batch_timing_launches': (_I, [_P, _P, _I]),
    'fb_batch_scheduler': (_I, [_P, C.POINTER(_I)]),
    'fb_batch_forget_stream': (_I, [_P, _P]),
    'fb_random_actions': (_I, [_P, _P, _I, _I, C.c_uint64, _I, _I, _I, _P]),
    'fb_batch_ik': (_I, [_P, _P, _P, _P]),
    'fb_batch_inverse': (_I, [_P, _I, _P]),
    'fb_batch_transition_fd': (_I, [_P]*8),
    'fb_batch_fd_tickets': (_I, [_P, C.POINTER(C.c_int64)]),
    'fb_batch_rollout': (_I, [_P]*8),
    'fb_batch_rollouts_run': (_I, [_P, C.POINTER(C.c_int64)]),
    'fb_batch_rollout_feedback': (_I, [_P]*8),
    'fb_batch_lqr_backward': (_I, [_P]*17),
    'fb_riccati_gemm': (_I, [_P] + [_I]*5 + [_P]*5),
    'fb_batch_ray': (_I, [_P]*7),
    'fb_batch_clear_forces': (_I, [_P]),
    'fb_batch_forces_active': (_I, [_P]),
    'fb_batch_set_control_law': (_I, [_P, _P]),
    'fb_batch_control_law_active': (_I, [_P]),
    'fb_batch_end_episode': (_I, [_P, _P, _P, _P]),
    'fb_batch_create_group': (_I, [_P, _I, _I, _I, _I, C.POINTER(_P)]),
    'fb_batch_n_models': (_I, [_P]),
    'fb_last_error': (C.c_char_p, []),
    'fb_version': (C.c_char_p, []),
}

_libs: Dict[str, C.CDLL] = {}


class EngineError(RuntimeError):
    pass


def load_library(lib_path: Optional[str] = None) -> C.CDLL:
    path = lib_path or HIP_LIB
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise EngineError(f'{path} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                          '(hipcc --offload-arch=gfx950); there is no CPU fallback')
    if lib_path is None or lib_path == HIP_LIB_DENSE:
        # torch bundles its own libamdhip64; it must be the first HIP runtime loaded into the
        # process, otherwise torch.cuda later fails with "No HIP GPUs are available".
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(path)
    for name, (restype, argtypes) in _SIGNATURES.items():
        f = getattr(L, name, None)
        if f is None:
            raise EngineError(f'{path} does not export {name}: rebuild it with `python -c "import __graft_entry__ as g; g.build()"` '
                              '(hipcc --offload-arch=gfx950)')
        f.restype, f.argtypes = restype, argtypes
    _libs[path] = L
    return L


def version(lib_path: Optional[str] = None) -> str:
    """Build identity of the loaded engine library (fb_version)."""
    return load_library(lib_path).fb_version().decode()


def source_hash() -> str:
    """Hash of the kernel sources in this tree (csrc/ + the C-ABI header), as embedded into the library at build time."""
    import hashlib
    root = os.path.dirname(_HERE)
    files = [os.path.join(root, 'include', 'flybody_engine.h')]
    for base, _, names in os.walk(os.path.join(_HERE, 'csrc')):
        files += [os.path.join(base, f) for f in names if f.endswith(('.hip', '.hpp', '.h'))]
    h = hashlib.sha1()
    for f in sorted(files):
        h.update(os.path.relpath(f, root).encode()); h.update(open(f, 'rb').read())
    return h.hexdigest()[:12]


def _check(L, rc):
    if rc != 0:
        raise EngineError(L.fb_last_error().decode())


def _ptr(t):
    """The address of a tensor's data as the C calls take it (None stays None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def as_env_ids(env_ids, n_all: Optional[int] = None):
    """Environment (or nominal) ids as the C calls read them, a contiguous int32 vector; None: all `n_all` of them, or None without it."""
    if env_ids is None:
        return None if n_all is None else np.arange(n_all, dtype=np.int32)
    return np.ascontiguousarray(env_ids, np.int32).reshape(-1)


def _check_tensor(x, dtype, device, shape, message):
    """ValueError(message) unless x is a contiguous torch tensor of `dtype` on `device` whose shape is `shape`: an entry None leaves that
    axis free (so (None, None, nu) is a trailing shape), shape None leaves all of it to the caller."""
    import torch
    if not isinstance(x, torch.Tensor) or x.dtype != dtype or not x.is_contiguous() or x.device != device or (
            shape is not None and (x.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, x.shape)))):
        raise ValueError(message)


def state_views(state, nq: int, nv: int):
    """(state, qpos, qvel, act): the leading fields of a Rollout, the last three views into state [..., nq + nv + na]."""
    return state, state[..., :nq], state[..., nq:nq + nv], state[..., nq + nv:]


def as_model(name_or_model) -> 'Model':
    """The array API's model argument: an asset name loads that asset; a Model (or anything with its `.arrays`) is itself."""
    return Model.from_asset(name_or_model) if isinstance(name_or_model, str) else name_or_model


def helper_batches(model: 'Model', n: int, batch_size: int, device: int = 0, rows: Optional[int] = None):
    """The array API's helper batch: yields (batch, lo, hi) over n frames in chunks [lo, hi) of at most `batch_size`.  A chunk's FP64 batch
    has `rows` environments (None: one per frame of the chunk); it is reused while that count stays, so only a shorter last chunk makes
    another."""
    if int(batch_size) < 1:
        raise ValueError('batch_size must be >= 1')
    batch = None
    for lo in range(0, n, int(batch_size)):
        hi = min(n, lo + int(batch_size))
        need = hi - lo if rows is None else rows
        if batch is None or batch.n_env != need:
            batch = Batch(model, need, device=device, precision=64)
        yield batch, lo, hi


class _DeviceCall:
    """The surroundings of one torch-facing device call of a batch (transition_fd, rollout, rollout_feedback, lqr_backward, riccati_gemm, cast_rays):
    `device`, the torch.device the batch computes on -- the CPU for the kernel-emulation build (`emulated`), whose "device" memory is host
    memory --; `stream`, the handle the C call gets: the caller's, else torch's current stream of that device (None when emulated); and
    the call's outputs and temporaries, made in that stream's order: zero-filled before the kernel writes them and freed behind it.  A
    consumer on another stream orders itself behind the call's stream."""

    def __init__(self, batch: 'Batch', stream=None):
        import torch
        self.emulated = b'emulation' in batch.L.fb_version()
        self.device = torch.device('cpu') if self.emulated else torch.device('cuda', batch.device)
        current = None if self.emulated else torch.cuda.current_stream(batch.device).cuda_stream
        self.stream = current if stream is None else stream
        self._aside = not self.emulated and self.stream != current

    def _ordered(self, make):
        import torch
        if not self._aside:
            return make()
        with torch.cuda.stream(torch.cuda.ExternalStream(self.stream, device=self.device)):
            return make()

    def zeros(self, *shape, dtype=None):
        import torch
        return self._ordered(lambda: torch.zeros(shape, dtype=dtype or torch.float64, device=self.device))

    def empty(self, *shape, dtype=None):
        import torch
        return self._ordered(lambda: torch.empty(shape, dtype=dtype or torch.float64, device=self.device))

    def contiguous(self, t):
        return self._ordered(t.contiguous)


def observation_layout(model: 'Model', future_steps: int, ball: bool = False):
    """({observable: (offset, size, shape)}, width) of the packed observation vector (fb_task.hpp: d_pack_obs writes it).  The buffer is in
    sorted-key order (tasks/task_utils.py:12); walk_on_ball (ball=True) has no reference observables, its ball's velocity instead;
    template_task (the model's task id) has neither."""
    na, napp, nforce, nobsj, ntouch = (model.dim(k) for k in ('na', 'napp', 'nforce', 'nobsjnt', 'ntouch'))
    nf = 0 if ball or model.dim('task_id') == TASK_IDS['template_task'] else future_steps + 1
    sizes = collections.OrderedDict([
        ('accelerometer', (3,)), ('actuator_activation', (na,)), ('appendages_pos', (3*napp,)), ('ball_qvel', (3 if ball else 0,)),
        ('force', (3*nforce,)),
        ('gyro', (3,)), ('joints_pos', (nobsj,)), ('joints_vel', (nobsj,)), ('ref_displacement', (nf, 3)),
        ('ref_root_quat', (nf, 4)), ('touch', (ntouch,)), ('velocimeter', (3,)), ('world_zaxis', (3,))])
    layout = collections.OrderedDict(); off = 0
    for k, shp in sizes.items():
        n = int(np.prod(shp)); layout[k] = (off, n, shp); off += n
    return layout, off


class _WalkDataset(C.Structure):
    """fb_walk_dataset (include/flybody_engine.h)."""
    _fields_ = [('n_traj', C.c_int32), ('n_joints', C.c_int32), ('n_sites', C.c_int32), ('n_select', C.c_int32), ('traj_offset', _P), ('qpos', _P),
                ('qvel', _P), ('root2site', _P), ('joint_quat', _P), ('joint_ids', _P), ('site_ids', _P), ('select', _P), ('future_steps', C.c_int32),
                ('terminal_com_dist', _D), ('time_limit', _D), ('seed', C.c_uint32), ('env_id_base', C.c_int32)]


class _FlightDataset(C.Structure):
    """fb_flight_dataset (include/flybody_engine.h)."""
    _fields_ = [('n_traj', C.c_int32), ('n_select', C.c_int32), ('traj_offset', _P), ('qpos', _P), ('qvel', _P), ('select', _P),
                ('future_steps', C.c_int32), ('randomize_start_step', C.c_int32), ('terminal_com_dist', _D), ('time_limit', _D),
                ('seed', C.c_uint32), ('env_id_base', C.c_int32)]


class _IKConfig(C.Structure):
    """fb_ik_config (include/flybody_engine.h)."""
    _fields_ = [('n_site', C.c_int32), ('n_joint', C.c_int32), ('site_ids', C.c_void_p), ('joint_ids', C.c_void_p), ('include', C.c_void_p),
                ('reg_strength', C.c_double), ('lr', C.c_double), ('beta', C.c_double), ('progress_threshold', C.c_double), ('max_steps', C.c_int32)]


class _ControlLaw(C.Structure):
    """fb_control_law (include/flybody_engine.h)."""
    _fields_ = [(k, C.c_void_p) for k in LAW_ROWS] + [('n_rows', C.c_int32)]


class _FDConfig(C.Structure):
    """fb_fd_config (include/flybody_engine.h)."""
    _fields_ = [('eps', C.c_double), ('centered', C.c_int32), ('n_substeps', C.c_int32), ('n_frames', C.c_int32), ('env_ids', C.c_void_p),
                ('pool_rows', C.c_int32)]


class _RolloutConfig(C.Structure):
    """fb_rollout_config (include/flybody_engine.h)."""
    _fields_ = [('n_roll', C.c_int32), ('horizon', C.c_int32), ('n_substeps', C.c_int32), ('env_ids', C.c_void_p), ('pool_rows', C.c_int32)]


class _Feedback(C.Structure):
    """fb_feedback (include/flybody_engine.h)."""
    _fields_ = [('n_nom', C.c_int32), ('nom_ids', C.c_void_p), ('x_nom', C.c_void_p), ('u_nom', C.c_void_p), ('K', C.c_void_p), ('k', C.c_void_p),
                ('alpha', C.c_void_p)]


class _LQRConfig(C.Structure):
    """fb_lqr_config (include/flybody_engine.h)."""
    _fields_ = [('n_nom', C.c_int32), ('horizon', C.c_int32), ('ndx', C.c_int32), ('nu', C.c_int32), ('stationary', C.c_int32)]


class _Terrain(C.Structure):
    """fb_terrain (include/flybody_engine.h)."""
    _fields_ = [('nrow', C.c_int32), ('ncol', C.c_int32), ('n_terrain', C.c_int32), ('size', C.c_double*4), ('pos', C.c_double*3),
                ('data', C.c_void_p), ('terrain_ids', C.c_void_p)]


class _RayConfig(C.Structure):
    """fb_ray_config (include/flybody_engine.h)."""
    _fields_ = [('n_frames', C.c_int32), ('n_ray', C.c_int32), ('per_frame', C.c_int32), ('env_ids', C.c_void_p), ('body', C.c_int32),
                ('bodyexclude', C.c_int32), ('geom_mask', C.c_void_p), ('cutoff', C.c_double)]


class Model:
    """Compiled model handle (fb_model)."""

    def __init__(self, arrays: Dict[str, np.ndarray], lib_path: Optional[str] = None, dense: bool = False):
        if dense and lib_path is None:
            lib_path = HIP_LIB_DENSE
        self.L = load_library(lib_path)
        self.arrays = arrays
        self.blob = pack_model(arrays)
        h = C.c_void_p()
        _check(self.L, self.L.fb_model_load(self.blob, len(self.blob), C.byref(h)))
        self.h = h

    @classmethod
    def from_asset(cls, name: str = 'walk_imitation', lib_path: Optional[str] = None, dense: bool = False) -> 'Model':
        return cls(load_npz(os.path.join(ASSETS, name + '.npz')), lib_path, dense)

    def dim(self, name: str) -> int:
        return self.L.fb_model_dim(self.h, name.encode())

    def __del__(self):
        try:
            self.L.fb_model_destroy(self.h)
        except Exception:
            pass


class ModelGroup:
    """Models that one batch steps side by side (fb_batch_create_group): the same tree, different real-valued constants -- masses,
    friction, gains, damping, gravity, ... (flybody_amd.randomization builds such variants).  `models` are array dicts or Model
    objects of one library.  Compatibility (equal dimensions, integer arrays and time steps) is checked by the library when the
    group is made; an incompatible model raises EngineError naming the first array that differs."""

    def __init__(self, models, lib_path: Optional[str] = None, dense: bool = False):
        models = list(models)
        if not models:
            raise ValueError('ModelGroup needs at least one model')
        self.models = [m if isinstance(m, Model) else Model(m, lib_path, dense) for m in models]
        self.L = self.models[0].L
        if any(m.L is not self.L for m in self.models):
            raise ValueError('the models of a group must come from one engine library')
        self.handles = (C.c_void_p*len(self.models))(*(m.h for m in self.models))
        if len(self.models) > 1:
            # the library's own check, on a one-environment batch (nothing else of it is used)
            h = C.c_void_p()
            _check(self.L, self.L.fb_batch_create_group(self.handles, len(self.models), 1, 0, 64, C.byref(h)))
            self.L.fb_batch_destroy(h)

    def __len__(self):
        return len(self.models)

    def dim(self, name: str) -> int:
        return self.models[0].dim(name)

    @property
    def arrays(self):
        return self.models[0].arrays


class Batch:
    """n_env environments on one device (fb_batch).  `model`: a Model, or a ModelGroup for per-environment models (field ENV_MODEL)."""

    def __init__(self, model, n_env: int, device: int = 0, precision: int = 64):
        self.group = model if isinstance(model, ModelGroup) else None
        self.model = model.models[0] if self.group else model
        self.L = self.model.L; self.n_env = n_env; self.precision = precision; self.device = device
        h = C.c_void_p()
        if self.group:
            _check(self.L, self.L.fb_batch_create_group(self.group.handles, len(self.group), n_env, device, precision, C.byref(h)))
        else:
            _check(self.L, self.L.fb_batch_create(self.model.h, n_env, device, precision, C.byref(h)))
        self.h = h
        self.nobs = 0

    @property
    def n_models(self) -> int:
        """Number of models the batch steps (1 unless it was made from a ModelGroup)."""
        return self.L.fb_batch_n_models(self.h)

    def set_reference(self, ref_qpos, ref_qvel, future_steps=64, terminal_com_dist=0.3, time_limit=10.0):
        rq = np.ascontiguousarray(ref_qpos, np.float64); rv = np.ascontiguousarray(ref_qvel, np.float64)
        assert rq.ndim == 2 and rq.shape[1] == 7 and rv.shape == (rq.shape[0], 6)
        _check(self.L, self.L.fb_batch_set_reference(self.h, rq.ctypes.data, rv.ctypes.data, rq.shape[0],
                                                     int(future_steps), float(terminal_com_dist), float(time_limit)))
        self.nobs = observation_layout(self.model, future_steps)[1]

    def set_walk_dataset(self, ds, joint_ids, site_ids, select=None, future_steps=64, terminal_com_dist=0.3, time_limit=10.0,
                         seed: int = 0, env_id_base: int = 0):
        """Training-mode walk_imitation on a trajectory_loaders.WalkingDataset (fb_batch_set_walk_dataset)."""
        sel = np.arange(ds.n_traj, dtype=np.int32) if select is None else np.ascontiguousarray(select, np.int32)
        keep = [np.ascontiguousarray(ds.offsets, np.int32), np.ascontiguousarray(ds.qpos, np.float64), np.ascontiguousarray(ds.qvel, np.float64),
                np.ascontiguousarray(ds.root2site, np.float64), np.ascontiguousarray(ds.joint_quat, np.float64),
                np.ascontiguousarray(joint_ids, np.int32), np.ascontiguousarray(site_ids, np.int32), sel]
        assert keep[1].shape[1] == 7 + len(keep[5]) and keep[2].shape[1] == 6 + len(keep[5])
        d = _WalkDataset(ds.n_traj, len(keep[5]), len(keep[6]), len(sel), *(a.ctypes.data for a in keep), int(future_steps), float(terminal_com_dist),
                         float(time_limit), int(seed), int(env_id_base))
        _check(self.L, self.L.fb_batch_set_walk_dataset(self.h, C.byref(d)))
        self.nobs = observation_layout(self.model, future_steps)[1]

    def set_flight_dataset(self, offsets, root_qpos, qvel, select=None, future_steps=5, terminal_com_dist=2.0, time_limit=0.6,
                           randomize_start_step=True, seed: int = 0, env_id_base: int = 0):
        """flight_imitation on a reference dataset (fb_batch_set_flight_dataset); root_qpos = FlightDataset.root_qpos(com_offset)."""
        n_traj = len(offsets) - 1
        sel = np.arange(n_traj, dtype=np.int32) if select is None else np.ascontiguousarray(select, np.int32)
        keep = [np.ascontiguousarray(offsets, np.int32), np.ascontiguousarray(root_qpos, np.float64), np.ascontiguousarray(qvel, np.float64), sel]
        assert keep[1].shape == (keep[0][-1], 7) and keep[2].shape == (keep[0][-1], 6)
        d = _FlightDataset(n_traj, len(sel), keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, sel.ctypes.data, int(future_steps),
                           int(bool(randomize_start_step)), float(terminal_com_dist), float(time_limit), int(seed), int(env_id_base))
        _check(self.L, self.L.fb_batch_set_flight_dataset(self.h, C.byref(d)))
        self.nobs = observation_layout(self.model, future_steps)[1]

    def set_time_limit(self, time_limit: float = 2.0):
        """walk_on_ball: no reference trajectory, only the episode time limit."""
        _check(self.L, self.L.fb_batch_set_time_limit(self.h, float(time_limit)))
        self.nobs = observation_layout(self.model, 0, ball=True)[1]

    def set_wbpg(self, tables, seed: int = 0):
        t = np.ascontiguousarray(tables['traj'], np.float64); p = np.ascontiguousarray(tables['phase'], np.float64)
        o = np.ascontiguousarray(tables['offset'], np.int32); f = np.ascontiguousarray(tables['beat_freqs'], np.float64)
        _check(self.L, self.L.fb_batch_set_wbpg(self.h, t.ctypes.data, p.ctypes.data, o.ctypes.data, f.ctypes.data, len(f),
                                                float(tables['base_freq']), float(tables['rel_range']), float(tables['rate']), int(seed)))

    def reset(self, env_ids=None, stream=None):
        if env_ids is None:
            _check(self.L, self.L.fb_batch_reset(self.h, None, 0, stream))
        else:
            ids = np.ascontiguousarray(env_ids, np.int32)
            _check(self.L, self.L.fb_batch_reset(self.h, ids.ctypes.data, len(ids), stream))

    def step_ptr(self, action_dev_ptr: int, stream=None):
        """action_dev_ptr: device pointer to float32 [n_env][nu]."""
        _check(self.L, self.L.fb_batch_step(self.h, C.c_void_p(action_dev_ptr), stream))

    def random_actions(self, action_dev_ptr: int, step: int, seed: int = 0, env_id_base: int = 0, dist: int = 0, stream=None,
                       env_ids_dev_ptr: Optional[int] = None, n: Optional[int] = None):
        """Fill the device array action[n][nact] (float32) for control step `step`: one Philox stream per GLOBAL environment id
        (env_id_base + e, or the ids behind env_ids_dev_ptr), N(0,1) clipped to [-1, 1] (dist 0) or U(-1, 1) (dist 1)."""
        _check(self.L, self.L.fb_random_actions(C.c_void_p(action_dev_ptr), C.c_void_p(env_ids_dev_ptr) if env_ids_dev_ptr else None,
                                                self.n_env if n is None else int(n), self.model.dim('nact'), int(seed), int(step), int(env_id_base), int(dist), stream))

    def substep(self, n=1, stream=None):
        _check(self.L, self.L.fb_batch_substep(self.h, n, stream))

    def forward(self, stream=None):
        _check(self.L, self.L.fb_batch_forward(self.h, stream))

    def stage(self, stage_word: int, action_dev_ptr: int = 0, stream=None):
        """Profiling: one stage of a control step for every environment (fb_batch_stage; sequence: engine.stage_sequence)."""
        _check(self.L, self.L.fb_batch_stage(self.h, int(stage_word), C.c_void_p(action_dev_ptr) if action_dev_ptr else None, stream))

    def ik(self, site_ids, joint_ids, target_xpos, include=None, reg_strength=0.0, lr=0.01, beta=0.99, progress_threshold=0.01,
           max_steps=20_000, stream=None):
        """Multi-site inverse kinematics for every environment (fb_batch_ik): environment e fits target_xpos[e] ([n_env][n_site][3])
        from its QPOS and leaves the result there; per-environment results in IK_ERR (err_norm, err_norm_first_term) and IK_STEPS
        (steps, success).  include: [3 n_site] 0 / 1 mask of the components that enter the objective (None: all).  Asynchronous."""
        s = np.ascontiguousarray(site_ids, np.int32); j = np.ascontiguousarray(joint_ids, np.int32)
        inc = np.ones(3*len(s), np.int32) if include is None else np.ascontiguousarray(include, np.int32)
        t = np.ascontiguousarray(target_xpos, np.float64)
        if inc.shape != (3*len(s),) or t.shape != (self.n_env, len(s), 3):
            raise ValueError(f'include must be [{3*len(s)}] and target_xpos [{self.n_env}, {len(s)}, 3]')
        cfg = _IKConfig(len(s), len(j), s.ctypes.data, j.ctypes.data if len(j) else None, inc.ctypes.data, float(reg_strength), float(lr),
                        float(beta), float(progress_threshold), int(max_steps))
        _check(self.L, self.L.fb_batch_ik(self.h, C.byref(cfg), t.ctypes.data, stream))

    def inverse(self, discrete: bool = False, stream=None):
        """Inverse dynamics for every environment (fb_batch_inverse, MuJoCo's mj_inverse): the generalised force that gives the
        environment's QPOS / QVEL the acceleration QACC (set by the caller), in QFRC_INVERSE; per-contact forces in CONTACT_FORCE
        ([n_env][MAXCON][3], contact frame); EFC_FORCE / QFRC_CONSTRAINT hold the inverse's values.  discrete: QACC is (qvel+ - qvel) / h
        of the engine's Euler substep (FB_INV_DISCRETE).  Noslip is not inverted.  FP64 batches only.  Asynchronous after its checks."""
        _check(self.L, self.L.fb_batch_inverse(self.h, 1 if discrete else 0, stream))

    def transition_fd(self, env_ids=None, eps: float = 1e-6, centered: bool = True, n_substeps: int = 1, sensors: bool = False,
                      want_A: bool = True, want_B: bool = True, pool_rows: int = 0, stream=None) -> 'TransitionFD':
        """Transition derivatives of the listed environments (fb_batch_transition_fd, MuJoCo's mjd_transitionFD; None: all of them):
        TransitionFD(A [n, ndx, ndx], B [n, ndx, nu], C [n, 33, ndx], D [n, 33, nu], status [n]) as torch FP64 (status: int32) tensors
        on the batch's device, None for what was not asked for (want_A / want_B; sensors: C and D beside them).  ndx = 2 nv + na;
        x = (qpos, qvel, act) in the tangent space, u = ctrl.  The environments are only read.  Asynchronous on `stream` (None: torch's
        current stream of the device, so torch work that follows is ordered behind it).  A library without a GPU behind it (the tests'
        kernel-emulation build) gets CPU tensors: its "device" memory is host memory."""
        import torch
        call = _DeviceCall(self, stream)
        ids = as_env_ids(env_ids, self.n_env)
        n, nv, na, nu = len(ids), self.model.dim('nv'), self.model.dim('na'), self.model.dim('nu')
        ndx = 2*nv + na
        new = lambda want, *shape: call.zeros(n, *shape) if want and n else None
        A, B = new(want_A, ndx, ndx), new(want_B, ndx, nu)
        Cs, Ds = new(want_A and sensors, NSENSOR, ndx), new(want_B and sensors, NSENSOR, nu)
        status = call.zeros(max(n, 1), dtype=torch.int32)
        cfg = _FDConfig(float(eps), int(bool(centered)), int(n_substeps), n, ids.ctypes.data, int(pool_rows))
        _check(self.L, self.L.fb_batch_transition_fd(self.h, C.byref(cfg), _ptr(A), _ptr(B), _ptr(Cs), _ptr(Ds), _ptr(status), call.stream))
        return TransitionFD(A, B, Cs, Ds, status[:n])

    def fd_tickets(self) -> int:
        """Transitions (nominal + perturbed) the last transition_fd call ran (fb_batch_fd_tickets; synchronises the device)."""
        n = C.c_int64(0)
        _check(self.L, self.L.fb_batch_fd_tickets(self.h, C.byref(n)))
        return n.value

    def rollout(self, ctrl=None, action=None, env_ids=None, n_substeps: int = 0, sensors: bool = False, pool_rows: int = 0,
                stream=None) -> 'Rollout':
        """Open-loop rollouts from the listed environments as they stand (fb_batch_rollout, MuJoCo's rollout; env_ids None: rollout r
        starts from environment r; repeats are allowed -- K samples of one state).  Exactly one input, a contiguous torch tensor on the
        batch's device: ctrl float64 [n, T, nu], held over the n_substeps physics substeps of each of the T intervals (0: the model's
        own count, one control step), or action float32 [n, T, nact], which goes through the task's before_step hook as in a control
        step.  Returns Rollout(state [n, T, nq + nv + na] float64, its views qpos / qvel / act, sensordata [n, T, 33] or None, status
        int32 [n]: the OR of the WARN bits the rollout raised).  No reward, termination or reset; the environments are only read.
        Asynchronous on `stream` (None: torch's current stream of the device, so torch work that follows is ordered behind it).  A
        library without a GPU behind it (the tests' kernel-emulation build) takes and gives CPU tensors: its "device" memory is host
        memory."""
        import torch
        if (ctrl is None) == (action is None):
            raise ValueError('rollout takes exactly one of ctrl and action')
        x, dt, width, what = (ctrl, torch.float64, self.model.dim('nu'), 'ctrl') if action is None else (action, torch.float32, self.model.dim('nact'), 'action')
        call = _DeviceCall(self, stream)
        _check_tensor(x, dt, call.device, (None, None, width), f'{what} must be a contiguous {dt} tensor [n, T, {width}] on {call.device}')
        n, T = int(x.shape[0]), int(x.shape[1])
        ids = as_env_ids(env_ids)
        if ids is not None and len(ids) != n:
            raise ValueError(f'env_ids names {len(ids)} environments for {n} rollouts')
        nq, nv, na = self.model.dim('nq'), self.model.dim('nv'), self.model.dim('na')
        state = call.zeros(n, T, nq + nv + na)
        sens = call.zeros(n, T, NSENSOR) if sensors else None
        status = call.zeros(max(n, 1), dtype=torch.int32)
        cfg = _RolloutConfig(n, T, int(n_substeps), None if ids is None else ids.ctypes.data, int(pool_rows))
        _check(self.L, self.L.fb_batch_rollout(self.h, C.byref(cfg), _ptr(ctrl), _ptr(action), _ptr(state), _ptr(sens), _ptr(status), call.stream))
        return Rollout(*state_views(state, nq, nv), sens, status[:n])

    def rollout_feedback(self, x_nom, u_nom, K=None, k=None, alpha=None, nom_ids=None, env_ids=None, n_substeps: int = 0,
                         sensors: bool = False, pool_rows: int = 0, stream=None) -> 'Rollout':
        """Closed-loop rollouts from the listed environments as they stand (fb_batch_rollout_feedback): at the start of interval t rollout
        r applies u = clamp(u_nom[m, t] + alpha[r] k[m, t] + K[m, t] (x_t (-) x_nom[m, t])), m = nom_ids[r], evaluated on the device from
        the state the rollout has reached; (-) is the tangent-space difference of transition_fd (lqr.state_difference), clamp the
        actuators' ctrlrange.  Contiguous float64 torch tensors on the batch's device: x_nom [n_nom, T, nq + nv + na] -- the nominal
        state at the START of interval t --, u_nom [n_nom, T, nu], K [n_nom, T, nu, ndx] (None: zero; transposed once here, on the
        stream, to the layout the kernel reads), k [n_nom, T, nu] (None: zero), alpha [n] (None: 1; the step length of a line search).
        nom_ids [n] (None: rollout r follows nominal r, and n_nom == n); env_ids [n] (None: rollout r starts from environment r); the
        number of rollouts n is that of env_ids, else of nom_ids, else n_nom.  Returns Rollout as rollout() does, with ctrl [n, T, nu]:
        the inputs applied.  Feedback acts on ctrl only, not on a task's actions.  Asynchronous on `stream` like rollout()."""
        import torch
        call = _DeviceCall(self, stream)
        dev = call.device
        nq, nv, na, nu = (self.model.dim(d) for d in ('nq', 'nv', 'na', 'nu'))
        nx, ndx = nq + nv + na, 2*nv + na

        def chk(x, what, *tail):
            _check_tensor(x, torch.float64, dev, (None, None) + tail,
                          f'{what} must be a contiguous torch.float64 tensor [n_nom, T, {", ".join(map(str, tail))}] on {dev}')
        chk(x_nom, 'x_nom', nx)
        n_nom, T = int(x_nom.shape[0]), int(x_nom.shape[1])
        chk(u_nom, 'u_nom', nu)
        if K is not None:
            if isinstance(K, torch.Tensor) and K.dim() == 4 and not K.is_contiguous() and K.transpose(2, 3).is_contiguous():
                chk(K.transpose(2, 3), 'K (behind transpose(2, 3))', ndx, nu)     # lqr_backward's view of the array the kernel streams: no copy below
            else:
                chk(K, 'K', nu, ndx)
        if k is not None:
            chk(k, 'k', nu)
        for x, what in ((u_nom, 'u_nom'), (K, 'K'), (k, 'k')):
            if x is not None and tuple(x.shape[:2]) != (n_nom, T):
                raise ValueError(f'{what} must have the leading axes of x_nom, [{n_nom}, {T}]')
        ids, noms = as_env_ids(env_ids), as_env_ids(nom_ids)
        n = len(ids) if ids is not None else len(noms) if noms is not None else n_nom
        if noms is not None and len(noms) != n:
            raise ValueError(f'nom_ids names {len(noms)} nominals for {n} rollouts')
        if alpha is not None:
            _check_tensor(alpha, torch.float64, dev, (n,), f'alpha must be a contiguous torch.float64 tensor [{n}] on {dev}')
        Kt = None if K is None else call.contiguous(K.transpose(2, 3))
        state, ctrl = call.zeros(n, T, nx), call.zeros(n, T, nu)
        sens = call.zeros(n, T, NSENSOR) if sensors else None
        status = call.zeros(max(n, 1), dtype=torch.int32)
        cfg = _RolloutConfig(n, T, int(n_substeps), None if ids is None else ids.ctypes.data, int(pool_rows))
        fbk = _Feedback(n_nom, None if noms is None else noms.ctypes.data, _ptr(x_nom), _ptr(u_nom), _ptr(Kt), _ptr(k), _ptr(alpha))
        _check(self.L, self.L.fb_batch_rollout_feedback(self.h, C.byref(cfg), C.byref(fbk), _ptr(state), _ptr(sens), _ptr(ctrl), _ptr(status),
                                                        call.stream))
        return Rollout(*state_views(state, nq, nv), sens, status[:n], ctrl)

    def _torch_device(self):
        """The torch.device of this batch's arrays (the emulation build computes on CPU tensors)."""
        return _DeviceCall(self).device

    def lqr_backward(self, A, B, Q, R, Qf=None, q=None, r=None, mu=None, stationary: bool = False, horizon: Optional[int] = None,
                     want_P: bool = False, stream=None) -> 'LQRBackward':
        """The backward pass of LQR / iLQR for n_nom independent nominals on the device (fb_batch_lqr_backward; the formulas and the
        conventions of lqr.backward_pass).  Contiguous float64 torch tensors on the batch's device: A [n_nom, T, ndx, ndx],
        B [n_nom, T, ndx, nu] (what transition_fd returns, stacked), Q / Qf [ndx, ndx] (Qf None: Q), R [nu, nu]; optional q [n_nom, T + 1, ndx],
        r [n_nom, T, nu] (the cost's gradient along the nominal: iLQR) and mu [n_nom] (the regularisation of Quu).  stationary=True:
        A [n_nom, ndx, ndx], B [n_nom, ndx, nu], the recursion runs `horizon` times (required then) and only t = 0 is kept -- time axes
        1 (K, k) and 2 (P, p: P_0 and P_1), q [n_nom, 2, ndx] (running, terminal), r [n_nom, 1, nu].  ndx and nu are the arrays' own: the
        batch gives the device and the workspace only.  want_P: also return P and p.  Returns LQRBackward(K, k, P, p, dV, status);
        K [n_nom, T, nu, ndx] is a view whose transpose(2, 3) is contiguous -- the layout rollout_feedback streams, so the hand-over
        copies nothing.  A nominal whose Quu + mu I is not positive definite at interval t has status 1 + t and zero outputs from t
        down.  Asynchronous on `stream` (None: torch's current stream)."""
        import torch
        call = _DeviceCall(self, stream)

        def chk(x, what, shape, names):
            _check_tensor(x, torch.float64, call.device, shape, f'{what} must be a contiguous torch.float64 tensor [{names}] on {call.device}')
        chk(A, 'A', None, 'n_nom, ndx, ndx' if stationary else 'n_nom, T, ndx, ndx')
        if A.dim() != (3 if stationary else 4) or A.shape[-1] != A.shape[-2] or min(A.shape) < 1:
            raise ValueError('A must be [n_nom, ndx, ndx] (stationary) or [n_nom, T, ndx, ndx]')
        n_nom, ndx = int(A.shape[0]), int(A.shape[-1])
        if stationary:
            if horizon is None or int(horizon) < 1:
                raise ValueError('stationary mode needs horizon >= 1: the number of Riccati steps')
            T, lead, Tout, TP = int(horizon), (n_nom,), 1, 2
        else:
            T = int(A.shape[1])
            if horizon is not None and int(horizon) != T:
                raise ValueError(f'horizon {horizon} is not the time axis of A ({T})')
            lead, Tout, TP = (n_nom, T), T, T + 1
        chk(B, 'B', None, 'n_nom, ndx, nu' if stationary else 'n_nom, T, ndx, nu')
        if B.dim() != A.dim() or tuple(B.shape[:-1]) != lead + (ndx,) or B.shape[-1] < 1:
            raise ValueError(f'B must be [{", ".join(map(str, lead + (ndx,)))}, nu]')
        nu = int(B.shape[-1])
        chk(Q, 'Q', (ndx, ndx), 'ndx, ndx'); chk(R, 'R', (nu, nu), 'nu, nu')
        if Qf is not None:
            chk(Qf, 'Qf', (ndx, ndx), 'ndx, ndx')
        if q is not None:
            chk(q, 'q', (n_nom, TP, ndx), 'n_nom, T + 1 (stationary: 2), ndx')
        if r is not None:
            chk(r, 'r', (n_nom, Tout, nu), 'n_nom, T (stationary: 1), nu')
        if mu is not None:
            chk(mu, 'mu', (n_nom,), 'n_nom')
        e = call.empty                                                           # (the call zeroes what it needs zero)
        Kt, k, dV, status = e(n_nom, Tout, ndx, nu), e(n_nom, Tout, nu), e(n_nom, 2), e(n_nom, dtype=torch.int32)
        P, p = (e(n_nom, TP, ndx, ndx), e(n_nom, TP, ndx)) if want_P else (None, None)
        cfg = _LQRConfig(n_nom, T, ndx, nu, 1 if stationary else 0)
        _check(self.L, self.L.fb_batch_lqr_backward(self.h, C.byref(cfg), _ptr(A), _ptr(B), _ptr(Q), _ptr(R), _ptr(Qf), _ptr(q), _ptr(r), _ptr(mu),
                                                    _ptr(Kt), _ptr(k), _ptr(P), _ptr(p), _ptr(dV), _ptr(status), call.stream))
        return LQRBackward(Kt.transpose(2, 3), k, P, p, dV, status)

    def riccati_gemm(self, X, Y, D=None, trans_x: bool = False, trans_y: bool = False, stream=None):
        """C = op(X) op(Y) (+ D) through the product kernel of lqr_backward alone (fb_riccati_gemm; a test entry): contiguous float64
        2-D torch tensors on the batch's device."""
        import torch
        call = _DeviceCall(self, stream)
        for x, what in ((X, 'X'), (Y, 'Y')) + (((D, 'D'),) if D is not None else ()):
            _check_tensor(x, torch.float64, call.device, (None, None), f'{what} must be a contiguous 2-D torch.float64 tensor on {call.device}')
        m, k = (X.shape[1], X.shape[0]) if trans_x else X.shape
        k2, n = (Y.shape[1], Y.shape[0]) if trans_y else Y.shape
        if k != k2 or (D is not None and tuple(D.shape) != (m, n)):
            raise ValueError(f'op(X) is {m} x {k}, op(Y) {k2} x {n}: the inner sizes must agree and D be [{m}, {n}]')
        Cm = call.empty(m, n)
        _check(self.L, self.L.fb_riccati_gemm(self.h, int(m), int(n), int(k), int(trans_x), int(trans_y), _ptr(X), _ptr(Y), _ptr(D), _ptr(Cm), call.stream))
        return Cm

    def cast_rays(self, rays, body: int = -1, env_ids=None, geom_mask=None, bodyexclude: int = -1, cutoff: Optional[float] = None,
                  terrain=None, terrain_ids=None, stream=None) -> 'RayResult':
        """Rays against the geoms of live environments as the last step, reset or forward() left them, and against an optional
        vision.Terrain (fb_batch_ray, MuJoCo's mj_ray / mj_multiRay; the semantics are the header's).  rays: float64 [n_ray, 6] -- one
        set for every frame -- or [n_frames, n_ray, 6], rows (origin, dir), a torch tensor on the batch's device (anything else is
        copied there); dir need not be unit length.  A frame is the environment env_ids[f] (None: frame f is environment f; one
        shared ray set is cast in every environment); repeats are allowed.  body: the rays are given in this body's frame (-1: the
        world's).  geom_mask [ngeom]: False / 0 hides a geom; bodyexclude: a body whose geoms are skipped.  cutoff: hits beyond it are
        misses (None: no limit).  terrain_ids [n_frames]: which of the terrain's grids a frame sees (None: grid 0).  Returns
        RayResult(dist float32 [n_frames, n_ray] in units of |dir|, -1 for a miss; geomid int32, -1 for a miss, ngeom for the terrain).
        Both precisions; the environments are only read.  Asynchronous on `stream` (None: torch's current stream of the device)."""
        import torch
        call = _DeviceCall(self, stream)
        if not (isinstance(rays, torch.Tensor) and rays.dtype == torch.float64 and rays.device == call.device and rays.is_contiguous()):
            rays = call._ordered(lambda: torch.as_tensor(np.asarray(rays, np.float64) if not isinstance(rays, torch.Tensor) else rays,
                                                         dtype=torch.float64, device=call.device).contiguous())
        if rays.dim() not in (2, 3) or rays.shape[-1] != 6 or min(rays.shape) < 1:
            raise ValueError('rays must be [n_ray, 6] or [n_frames, n_ray, 6]: rows (origin, dir)')
        ids = as_env_ids(env_ids)
        per_frame = rays.dim() == 3
        n_frames = int(rays.shape[0]) if per_frame else (len(ids) if ids is not None else self.n_env)
        if ids is not None and len(ids) != n_frames:
            raise ValueError(f'env_ids names {len(ids)} environments for {n_frames} frames of rays')
        n_ray = int(rays.shape[-2])
        mask = None if geom_mask is None else np.ascontiguousarray(np.asarray(geom_mask).astype(bool), np.uint8).reshape(-1)
        if mask is not None and len(mask) != self.model.dim('ngeom'):
            raise ValueError(f'geom_mask must be [{self.model.dim("ngeom")}]')
        ter = tids = None
        if terrain is not None:
            if terrain.heights.device != call.device:
                raise ValueError(f'the terrain lives on {terrain.heights.device}, the batch computes on {call.device}')
            tids = as_env_ids(terrain_ids)
            if tids is not None and len(tids) != n_frames:
                raise ValueError(f'terrain_ids names {len(tids)} terrains for {n_frames} frames')
            ter = _Terrain(terrain.nrow, terrain.ncol, terrain.n_terrain, (C.c_double*4)(*terrain.size), (C.c_double*3)(*terrain.pos),
                           terrain.heights.data_ptr(), None if tids is None else tids.ctypes.data)
        elif terrain_ids is not None:
            raise ValueError('terrain_ids without a terrain')
        dist, gid = call.empty(n_frames, n_ray, dtype=torch.float32), call.empty(n_frames, n_ray, dtype=torch.int32)
        cfg = _RayConfig(n_frames, n_ray, int(per_frame), None if ids is None else ids.ctypes.data, int(body), int(bodyexclude),
                         None if mask is None else mask.ctypes.data, 0.0 if cutoff is None else float(cutoff))
        _check(self.L, self.L.fb_batch_ray(self.h, C.byref(cfg), _ptr(rays), None if ter is None else C.byref(ter), _ptr(dist), _ptr(gid), call.stream))
        return RayResult(dist, gid)

    def rollouts_run(self) -> int:
        """Rollouts the last rollout / rollout_feedback call finished (fb_batch_rollouts_run; synchronises the device)."""
        n = C.c_int64(0)
        _check(self.L, self.L.fb_batch_rollouts_run(self.h, C.byref(n)))
        return n.value

    def clear_forces(self):
        """Free the applied-force arrays (QFRC_APPLIED / XFRC_APPLIED) and return the batch to the plain step kernel
        (fb_batch_clear_forces).  Zero-copy views of the arrays are dangling afterwards."""
        _check(self.L, self.L.fb_batch_clear_forces(self.h))

    @property
    def forces_active(self) -> bool:
        """True while the applied-force arrays are allocated (the first set() / device_ptr() of QFRC_APPLIED or XFRC_APPLIED allocates
        both): control steps, substeps and forward evaluations then read them, every substep; the forward pass of a reset does not.
        The arrays are caller-owned inputs: they persist until changed and nothing clears them on a reset (unlike MuJoCo)."""
        return self.L.fb_batch_forces_active(self.h) == 1

    def set_control_law(self, bias=None, act_gain=None, pos_gain=None, pos_ref=None, vel_gain=None):
        """A substep control law (fb_batch_set_control_law, csrc/fb_law.hpp): in every physics substep and forward evaluation
            u = bias + act_gain*qfrc_actuator - pos_gain*(qpos[hinge of the dof] - pos_ref) - vel_gain*qvel
        is added to the generalised forces, with this substep's actuator force.  Every row is [nv] (one law for the batch) or
        [n_env, nv]; None is zeros.  pos_gain must be zero on dofs that are no hinge's.  u of the last substep: get('QFRC_LAW')."""
        nv = self.model.dim('nv')
        rows = [None if r is None else np.asarray(r, np.float64) for r in (bias, act_gain, pos_gain, pos_ref, vel_gain)]
        per_env = any(r is not None and r.ndim == 2 and r.shape[0] == self.n_env and self.n_env > 1 for r in rows)
        shape = (self.n_env if per_env else 1, nv)
        keep = []
        for name, r in zip(LAW_ROWS, rows):
            if r is not None:
                try:
                    r = np.ascontiguousarray(np.broadcast_to(r.reshape((1, nv)) if r.size == nv else r, shape))
                except ValueError:
                    raise ValueError(f'control law row {name} has shape {r.shape}; expected [{nv}] or [{self.n_env}, {nv}]') from None
            keep.append(r)
        law = _ControlLaw(*(None if r is None else r.ctypes.data for r in keep), shape[0])
        _check(self.L, self.L.fb_batch_set_control_law(self.h, C.byref(law)))
        self._law_rows = shape[0]

    def clear_control_law(self):
        """Remove the control law: the batch is stepped by the kernel it had before (fb_batch_set_control_law(batch, NULL)).  Zero-copy
        views of CONTROL_LAW / QFRC_LAW are dangling afterwards."""
        _check(self.L, self.L.fb_batch_set_control_law(self.h, None))

    @property
    def control_law_active(self) -> bool:
        return self.L.fb_batch_control_law_active(self.h) == 1

    @property
    def control_law_rows(self) -> int:
        """Rows of the law that is set: 1 (one for the batch) or n_env; 0 without a law."""
        return self._law_rows if self.control_law_active else 0

    def end_episode(self, mask_dev_ptr: int, discount_dev_ptr: int = 0, stream=None):
        """End the episodes of the environments whose byte in the device mask [n_env] is non-zero and whose last step was MID
        (fb_batch_end_episode): they turn LAST with the float32 discount [n_env] behind discount_dev_ptr (0: discount 0) and the next
        control step auto-resets them.  Asynchronous on `stream`."""
        _check(self.L, self.L.fb_batch_end_episode(self.h, C.c_void_p(mask_dev_ptr), C.c_void_p(discount_dev_ptr) if discount_dev_ptr else None, stream))

    def synchronize(self, stream=None):
        _check(self.L, self.L.fb_batch_synchronize(self.h, stream))

    def row_bytes(self, which: int = 0) -> int:
        """Bytes of one environment's workspace row (which = 0 real arena, 1 int arena): the stride between the environments' rows behind
        device_ptr('QPOS') / device_ptr('QVEL').  No copy, no synchronisation."""
        n = C.c_size_t(0)
        _check(self.L, self.L.fb_batch_row(self.h, which, 0, None, 0, 0, C.byref(n)))
        return n.value

    def row(self, which: int, env: int, data: Optional[np.ndarray] = None) -> np.ndarray:
        """Profiling: the raw workspace row of one environment as bytes (which = 0 real arena, 1 int arena); data: write it back."""
        n = C.c_size_t(0)
        _check(self.L, self.L.fb_batch_row(self.h, which, env, None, 0, 0, C.byref(n)))
        if data is not None:
            buf = np.ascontiguousarray(data, np.uint8); assert buf.size == n.value
            _check(self.L, self.L.fb_batch_row(self.h, which, env, buf.ctypes.data, n.value, 1, None))
            return buf
        buf = np.empty(n.value, np.uint8)
        _check(self.L, self.L.fb_batch_row(self.h, which, env, buf.ctypes.data, n.value, 0, None))
        return buf

    def _field(self, name):
        """(id, dtype, width) of a field of this batch (FIELDS)."""
        fid, dt, w = FIELDS[name]
        k, dim = w if isinstance(w, tuple) else (1, w)
        if isinstance(dim, str):
            dim = self.nobs if dim == 'nobs' else self.model.dim(dim)
        return fid, dt, k*dim

    def get(self, name: str) -> np.ndarray:
        fid, dt, w = self._field(name)
        out = np.zeros((self.n_env, w), dt)
        _check(self.L, self.L.fb_batch_get(self.h, fid, out.ctypes.data, out.nbytes))
        return out

    def set(self, name: str, value):
        fid, dt, w = self._field(name)
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(value, dt), (self.n_env, w)))
        _check(self.L, self.L.fb_batch_set(self.h, fid, v.ctypes.data, v.nbytes))

    def device_ptr(self, name: str) -> int:
        p = self.L.fb_batch_device_ptr(self.h, FIELDS[name][0])
        if not p:
            raise EngineError(f'no device pointer for {name}')
        return p

    def device_view(self, name: str):
        """A zero-copy torch tensor [n_env, width] over a field that device_ptr serves, on the batch's device (a GPU-backed library): the
        table's element type, FP64 physics fields at the batch's precision.  QPOS and QVEL are windows of the arena (row stride
        row_bytes(0)); CONTROL_LAW is [control_law_rows, 5 nv].  The view dangles once its array is freed (clear_forces, clear_control_law)."""
        import torch
        _, dt, w = self._field(name)
        dt = np.dtype(np.float32 if dt is _F64 and self.precision == 32 else dt)
        lead = self.control_law_rows if name == 'CONTROL_LAW' else self.n_env
        row = self.row_bytes(0) if name in ('QPOS', 'QVEL') else w*dt.itemsize
        iface = {'shape': (lead, w), 'strides': (row, dt.itemsize), 'typestr': dt.str, 'data': (self.device_ptr(name), False), 'version': 2}
        return torch.as_tensor(type('DevBuf', (), {'__cuda_array_interface__': iface})(), device=f'cuda:{self.device}')

    @property
    def substep_scheduler(self) -> bool:
        """True when fb_batch_step hands out (environment, substep) tickets (batch larger than the resident wave slots); scheduling only."""
        return self.L.fb_batch_scheduler(self.h, None) == 1

    @property
    def resident_slots(self) -> int:
        n = C.c_int(); self.L.fb_batch_scheduler(self.h, C.byref(n)); return n.value

    def forget_stream(self, stream):
        """Before destroying a HIP stream the batch was stepped on (the validated streams are remembered by handle: fb_batch_forget_stream)."""
        _check(self.L, self.L.fb_batch_forget_stream(self.h, stream))

    def timing_begin(self, stream=None):
        _check(self.L, self.L.fb_batch_timing_begin(self.h, stream))

    def timing_end(self, stream=None):
        ms = C.c_float(); n = C.c_int()
        _check(self.L, self.L.fb_batch_timing_end(self.h, stream, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def timing_launches(self, cap: int = 2048) -> np.ndarray:
        """Duration (ms) of every fb_batch_step kernel of the last timed region (fb_batch_timing_launches)."""
        out = np.zeros(cap, np.float32)
        n = self.L.fb_batch_timing_launches(self.h, out.ctypes.data, cap)
        if n < 0:
            raise EngineError(self.L.fb_last_error().decode())
        return out[:n].copy()

    def __del__(self):
        try:
            self.L.fb_batch_destroy(self.h)
        except Exception:
            pass
