"""The task layer (flybody_amd/csrc/fb_task.hpp) states the common parts of the tasks' init / pre / post hooks once.  It is a restatement:
every arithmetic expression and its order are the parent commit's, so a strict-IEEE build (tests/test_solver_handover.py: strict_emu_lib,
-ffp-contract=off, no -march=native) must give the parent's results TO THE BIT, in FP64 and FP32.

tests/golden/task_hooks_parent_503b35d.npz holds what the parent's sources (503b35d) compute in that build for seven rollouts of 3
environments each, with actions from fixed default_rng seeds:

  walk_end    walk_imitation, inference, 8-frame reference, future_steps 2, terminal_com_dist 0.3, U(-1, 1), 12 steps: the trajectory
              ends (LAST with discount 1), auto-reset (FIRST); a host reset of environments 0 and 2 after the 4th control step (MODE_RESET)
  walk_early  the same with terminal_com_dist 0.005: early terminations (LAST with discount 0), the environments fall out of phase
  walk_ds     walk_imitation on a dataset (tests/test_training_mode.py: seed 3, env_id_base 4), 28 steps: DeepMimic reward factors, LAST
              at the snippet's end, a new snippet
  flight      flight_imitation, inference: 20-frame constant-speed reference, wing-beat tables, 28 steps
  flight_early  the same with terminal_com_dist 0.002: flight's own termination predicate fires (LAST with discount 0)
  flight_ds   flight_imitation on a dataset with randomize_start_step, time_limit 20 control steps, 28 steps
  ball        walk_on_ball, time_limit 0.05, 28 steps: LAST by the time limit

Per control step (index 0: after the reset): REWARD, DISCOUNT, STEP_TYPE, REWARD_FACTORS (walk_ds) and an 8-byte BLAKE2 digest of every
environment's observation vector; the observation vectors themselves after the reset, after the host reset and at the end; QPOS, QVEL,
ACT, CTRL at the end.  (The observations of every step would be 1.1 MB; equal digests are equal bits.  The price: on a host
whose libm differs there is no comparison of the observations within a tolerance, and a failing digest does not say which observable moved.)

The physics and the rewards call the host's libm (sin, cos, exp, acos, atan2), and the synthetic walking dataset comes out of the CPU
oracle: the file is portable between hosts that agree on those.  `python tests/test_task_hooks.py LIB [OUT]` records it from a strict
build of the PARENT's sources; the parent's build reproduces the committed file on the development host and on the GPU host.

Three of the 150 arrays are no longer the parent's: walk_ds_64_REWARD_FACTORS, walk_ds_32_REWARD and walk_ds_32_REWARD_FACTORS were re-recorded
after d_walk_training_reward stopped scaling the egocentric site vectors by 1 / |root quaternion|^2 (tests/test_task_layer.py found it): the
product with |q|^2, one rounding from 1 for the quaternion the integrator leaves, moves them by at most 1.3e-7 relative.  Every other array,
the FP32 rows behind the double episode clock included, is the parent's to the bit."""
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from _synthetic_dataset import make_dataset
from _synthetic_flight_dataset import make_flight_dataset
from test_solver_handover import strict_emu_lib          # noqa: F401  (fixture)

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'task_hooks_parent_503b35d.npz')
N_ENV = 3
STEP_FIELDS = ('REWARD', 'DISCOUNT', 'STEP_TYPE')
END_FIELDS = ('QPOS', 'QVEL', 'ACT', 'CTRL')


def _digest(obs):
    return np.array([np.frombuffer(hashlib.blake2b(np.ascontiguousarray(o).tobytes(), digest_size=8).digest(), np.uint64)[0] for o in obs])


def _arrays(name):
    from flybody_amd.model_blob import load_npz
    return load_npz(os.path.join(ROOT, 'flybody_amd', 'assets', name + '.npz'))


def _roll(B, acts, fields=STEP_FIELDS, host_reset=None):
    """B.reset(), then one control step per row of acts; host_reset = (k, ids): fb_batch_reset of those environments before step k."""
    rec = {f: [] for f in fields + ('OBS_DIGEST',)}
    out = {}

    def take():
        for f in fields: rec[f].append(B.get(f).copy())
        rec['OBS_DIGEST'].append(_digest(B.get('OBS')))
    B.reset(); take(); out['OBS_FIRST'] = B.get('OBS').copy()
    for k, a in enumerate(acts):
        if host_reset and host_reset[0] == k:
            B.reset(host_reset[1])
            out.update({'HOST_RESET_' + f: B.get(f).copy() for f in fields + ('OBS',)})
        a = np.ascontiguousarray(a, np.float32); B.step_ptr(a.ctypes.data); take()
    out.update({f: np.array(v) for f, v in rec.items()})
    out.update({f: B.get(f).copy() for f in END_FIELDS + ('OBS',)})
    return out


def _walk(lib, precision, terminal_com_dist, host_reset=None):
    from flybody_amd import engine
    from flybody_amd.reference import default_walking_reference
    qp, qv = default_walking_reference()
    B = engine.Batch(engine.Model(_arrays('walk_imitation'), lib_path=lib), N_ENV, precision=precision)
    B.set_reference(qp[:8], qv[:8], future_steps=2, terminal_com_dist=terminal_com_dist)
    return _roll(B, np.random.default_rng(11).uniform(-1, 1, (12, N_ENV, 59)), host_reset=host_reset)


_DATASET = []


def _walk_ds(lib, precision):
    from flybody_amd import engine
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    arr = _arrays('walk_imitation')
    if not _DATASET: _DATASET.append(make_dataset(fbo.OracleModel(pack_model(arr)), arr, n_traj=3, length=90))
    jid, sid = _DATASET[0].ids(arr)
    B = engine.Batch(engine.Model(arr, lib_path=lib), N_ENV, precision=precision)
    B.set_walk_dataset(_DATASET[0], jid, sid, terminal_com_dist=float('inf'), seed=3, env_id_base=4)
    return _roll(B, np.random.default_rng(1).uniform(-0.3, 0.3, (28, N_ENV, 59)), fields=STEP_FIELDS + ('REWARD_FACTORS',))


def _flight(lib, precision, dataset, terminal_com_dist=2.0):
    from flybody_amd import engine
    from flybody_amd.mjcf_compile import qrot
    from flybody_amd.reference import constant_speed_trajectory
    from flybody_amd.wbpg import build_tables
    arr = _arrays('flight_imitation')
    B = engine.Batch(engine.Model(arr, lib_path=lib), N_ENV, precision=precision)
    B.set_wbpg(build_tables(), seed=5)
    if dataset:
        ds = make_flight_dataset()
        B.set_flight_dataset(ds.offsets, ds.root_qpos(arr['com_offset']), ds.com_qvel, future_steps=5, terminal_com_dist=2.0, time_limit=20*2e-4,
                             randomize_start_step=True, seed=7, env_id_base=100)
    else:
        cq, cv = constant_speed_trajectory(20, 20.0, init_pos=(0, 0, 1), body_rot_angle_y=-47.5, control_timestep=2e-4)
        root = cq.copy()
        for i in range(len(root)): root[i, :3] = cq[i, :3] + qrot(cq[i, 3:], -arr['com_offset'])
        B.set_reference(root, cv, future_steps=5, terminal_com_dist=terminal_com_dist, time_limit=0.6)
    return _roll(B, np.random.default_rng(1).uniform(-1, 1, (28, N_ENV, 12)))


def _ball(lib, precision):
    from flybody_amd import engine
    B = engine.Batch(engine.Model(_arrays('walk_on_ball'), lib_path=lib), N_ENV, precision=precision)
    B.set_time_limit(0.05)
    return _roll(B, np.random.default_rng(0).uniform(-0.5, 0.5, (28, N_ENV, 59)))


FLIGHT_EARLY_DIST = 0.002
ROLLOUTS = {'walk_end': lambda l, p: _walk(l, p, 0.3, host_reset=(4, [0, 2])), 'walk_early': lambda l, p: _walk(l, p, 0.005), 'walk_ds': _walk_ds,
            'flight': lambda l, p: _flight(l, p, False), 'flight_early': lambda l, p: _flight(l, p, False, FLIGHT_EARLY_DIST),
            'flight_ds': lambda l, p: _flight(l, p, True), 'ball': _ball}


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize('precision', [64, 32])
@pytest.mark.parametrize('name', list(ROLLOUTS))
def test_rollout_equal_to_the_parent_to_the_bit(strict_emu_lib, golden, name, precision):
    got = ROLLOUTS[name](strict_emu_lib, precision)
    keys = [k for k in golden.files if k.startswith('%s_%d_' % (name, precision))]
    assert sorted(keys) == sorted('%s_%d_%s' % (name, precision, f) for f in got)
    for f, v in got.items():
        g = golden['%s_%d_%s' % (name, precision, f)]
        assert v.dtype == g.dtype and np.array_equal(v, g), (f, np.argwhere(v != g)[:4].tolist() if v.shape == g.shape else (v.shape, g.shape))


@pytest.mark.parametrize('precision', [64, 32])
def test_golden_reaches_every_branch_of_the_shared_epilogue(golden, precision):
    """A rollout that stops exercising a branch must not pass silently (index 0 of the per-step arrays is the state after the reset)."""
    t = {n: golden['%s_%d_STEP_TYPE' % (n, precision)][1:, :, 0] for n in ROLLOUTS}
    d = {n: golden['%s_%d_DISCOUNT' % (n, precision)][1:, :, 0] for n in ROLLOUTS}
    assert ((t['walk_end'] == 2) & (d['walk_end'] == 1)).any()                    # trajectory end: LAST, discount 1
    assert ((t['walk_early'] == 2) & (d['walk_early'] == 0)).any()                # failure: LAST, discount 0
    assert ((t['flight_early'] == 2) & (d['flight_early'] == 0)).any()            # ... by flight's predicate as well
    assert len({tuple(c) for c in t['walk_early'].T}) > 1                          # ... and the environments fall out of phase
    for n in ROLLOUTS:                                                            # every rollout: a LAST, then FIRST through the auto-reset
        assert ((t[n][:-1] == 2) & (t[n][1:] == 0)).any(), n
        assert ((t[n] != 0) | ((golden['%s_%d_REWARD' % (n, precision)][1:, :, 0] == 0) & (d[n] == 1))).all(), n
    assert (golden['walk_end_%d_HOST_RESET_STEP_TYPE' % precision].ravel() == [0, 1, 0]).all()      # MODE_RESET with ids
    # walk_on_ball: LAST by the time limit alone -- mid-episode (simtime < time_limit) one step earlier, no termination, discount 1
    k = np.argwhere((t['ball'][1:] == 2) & (t['ball'][:-1] == 1) & (d['ball'][1:] == 1))
    assert len(k) and (golden['ball_%d_REWARD' % precision][1:, :, 0] > 0).any()
    assert (golden['walk_ds_%d_REWARD_FACTORS' % precision][1:] > 0).all()


if __name__ == '__main__':          # LIB: compare what LIB computes with the committed file (exit status 1: differs); LIB OUT: record OUT
    lib = os.path.abspath(sys.argv[1])
    rec = {'%s_%d_%s' % (n, p, f): v for n in ROLLOUTS for p in (64, 32) for f, v in ROLLOUTS[n](lib, p).items()}
    if len(sys.argv) > 2:
        np.savez_compressed(sys.argv[2], **rec)
        print('wrote %s: %d arrays, %d bytes' % (sys.argv[2], len(rec), os.path.getsize(sys.argv[2])))
    else:
        g = np.load(GOLDEN)
        bad = [k for k in rec if k not in g.files or not np.array_equal(rec[k], g[k])] + [k for k in g.files if k not in rec]
        print('%s against %s: %s' % (lib, GOLDEN, 'differs in %s' % bad if bad else 'all %d arrays equal to the bit' % len(rec)))
        sys.exit(1 if bad else 0)
