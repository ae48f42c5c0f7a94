"""The kernels beside k_fly -- k_inverse, k_transition_fd / k_fd_assemble, k_rollout, k_closedloop_rollout -- state their shared frame, scratch
row, stage sequences, state record and tangent-space difference once (csrc/fb_side.hpp).  That is a restatement: the same
stage calls in the same order, the same loads, subtractions and stores, so every one of their calls must give the PARENT commit's results
to the bit.  tests/golden/side_kernels_parent_5d2e861.npz was recorded on an MI355X from libraries built from 5d2e861, with this file's
recorder, the way tests/test_gpu_stage_glue.py makes its records:

    python tests/test_gpu_side_kernels.py LIB,LIB_DENSE OUT        (LIB,LIB_DENSE alone: compare with the committed file, exit status 1 = differs)

Every case runs on both engine libraries (the default build: one wave per workgroup; the dense build: four, which share the LDS tables).  All FP64.
The walking cases share one batch per library: 4 environments of walk_imitation advanced by STEPS control steps of U(-1, 1) Philox actions,
so that contacts and limit rows are present (asserted: a record without contacts cannot pass).  In the order the calls are made:
  deriv_centered    2 frames, centred, with sensors, n_substeps 2, pool_rows 3 (rows are reused by several tickets): A, B, C, D, status, fd_tickets()
  deriv_forward     1 frame, forward differences, no sensors (the skip_tail path): A, B, status, fd_tickets()
  rollout_rows      3 rollouts by ctrl, horizon 3, n_substeps 2, sensors, pool_rows 2: a row runs a second ticket, the priority counters are off
  rollout_prio      the same rollouts with pool_rows 0: a rollout per row, the tail-aware priorities on
  feedback          3 closed-loop rollouts on 2 nominals through nom_ids, dense K, k, alpha, pool_rows 2; the nominals are the open-loop
                    rollouts' states at the start of each interval, a tangent step away (root rotation included, so dx has quaternion parts);
                    ctrl_out recorded
  inverse           the 4 environments without and with FB_INV_DISCRETE: QFRC_INVERSE, CONTACT_FORCE
  sources           QPOS / QVEL of the environments after all of it: the side kernels leave them alone (also asserted against their values before)
  flight_action     (a batch of its own) 2 action rollouts of flight_imitation, horizon 2, after set_wbpg and 3 control steps: the path that keeps
                    the two pattern-generator words of the int row
Large arrays (DIGEST_OVER elements and more) are stored as their SHA-256 and SAMPLES entries at a fixed stride, small ones whole."""
import hashlib
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'side_kernels_parent_5d2e861.npz')
pytestmark = pytest.mark.gpu

LIBS = ('default', 'dense')
CASES = ('deriv_centered', 'deriv_forward', 'rollout_rows', 'rollout_prio', 'feedback', 'inverse', 'sources', 'flight_action')
STEPS = 6
DIGEST_OVER, SAMPLES = 2048, 48


def _pack(out, name, x):
    """x whole, or its digest and a few entries."""
    x = np.ascontiguousarray(x)
    if x.size < DIGEST_OVER:
        out[name] = x
    else:
        out[name + '__sha256'] = np.frombuffer(hashlib.sha256(x.tobytes()).digest(), np.uint8).copy()
        out[name + '__shape'] = np.array(x.shape, np.int64)
        out[name + '__samples'] = x.ravel()[::max(1, x.size // SAMPLES)][:SAMPLES].copy()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _walking(lib, dev):
    import torch
    from flybody_amd import derivatives, engine
    from flybody_amd.model_blob import load_npz
    from flybody_amd.reference import default_walking_reference
    import feedback_cases as fc
    a = dict(load_npz(os.path.join(engine.ASSETS, 'walk_imitation.npz')))
    B = engine.Batch(engine.Model(a, lib_path=lib), 4, precision=64)
    B.set_reference(*default_walking_reference(), terminal_com_dist=float('inf'))
    B.reset()
    act = torch.empty(4, B.model.dim('nact'), device=dev)
    for k in range(STEPS):
        B.random_actions(act.data_ptr(), k, seed=17, dist=1); B.step_ptr(act.data_ptr())
    B.synchronize()
    ncon, nefc = B.get('NCON')[:, 0], B.get('NEFC')[:, 0]
    assert (ncon > 0).any() and (nefc > ncon).any(), (ncon, nefc)              # contacts, and rows beside theirs
    before = {f: B.get(f) for f in ('QPOS', 'QVEL', 'ACT', 'CTRL', 'QACC')}
    out = {'NCON': ncon, 'NEFC': nefc}
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    fd = B.transition_fd(env_ids=[1, 3], centered=True, n_substeps=2, sensors=True, pool_rows=3)
    for f in 'ABCD':
        _pack(out, 'deriv_centered__' + f, _np(getattr(fd, f)))
    out['deriv_centered__status'] = _np(fd.status); out['deriv_centered__tickets'] = np.array([B.fd_tickets()], np.int64)
    fd = B.transition_fd(env_ids=[2], centered=False, n_substeps=1, sensors=False)
    assert fd.C is None and fd.D is None
    for f in 'AB':
        _pack(out, 'deriv_forward__' + f, _np(getattr(fd, f)))
    out['deriv_forward__status'] = _np(fd.status); out['deriv_forward__tickets'] = np.array([B.fd_tickets()], np.int64)

    c = fc.Ctx(a, [(before['QPOS'][e], before['QVEL'][e], before['ACT'][e], before['CTRL'][e]) for e in range(4)], None, to, _np)
    assert fc.T == 3
    rng = np.random.default_rng(23)
    ctrl = c.lo + (c.hi - c.lo)*rng.uniform(0.3, 0.7, (3, fc.T, c.nu))
    envs = [0, 2, 3]
    for name, pool in (('rollout_rows', 2), ('rollout_prio', 0)):
        res = B.rollout(ctrl=to(ctrl), env_ids=envs, n_substeps=2, sensors=True, pool_rows=pool)
        _pack(out, name + '__state', _np(res.state)); _pack(out, name + '__sensordata', _np(res.sensordata))
        out[name + '__status'] = _np(res.status); out[name + '__run'] = np.array([B.rollouts_run()], np.int64)
    open_state = _np(res.state)

    # nominal m: the open-loop rollout m at the START of every interval, a tangent step of 0.01 away
    x_nom = np.empty((2, fc.T, c.nx))
    for m in range(2):
        for t in range(fc.T):
            x = c.x0[envs[m]] if t == 0 else open_state[m, t - 1]
            x_nom[m, t] = np.r_[derivatives.integrate_pos(c.shim, x[:c.nq], 0.01*rng.normal(size=c.nv)), x[c.nq:] + 0.01*rng.normal(size=c.nv + c.na)]
    K, k = fc.dense_gains(c, 2, seed=29, scale=0.3)
    res = fc.run(c, B, x_nom, ctrl[:2], K, k, np.array([1.0, 0.5, 0.25]), nom_ids=[0, 1, 0], env_ids=[0, 2, 0], n_substeps=2, sensors=True, pool_rows=2)
    _pack(out, 'feedback__state', _np(res.state)); _pack(out, 'feedback__sensordata', _np(res.sensordata)); _pack(out, 'feedback__ctrl', _np(res.ctrl))
    out['feedback__status'] = _np(res.status); out['feedback__run'] = np.array([B.rollouts_run()], np.int64)
    assert not np.array_equal(_np(res.ctrl)[0], ctrl[0])                          # (the feedback term is live)

    for name, discrete in (('plain', False), ('discrete', True)):
        B.inverse(discrete=discrete); B.synchronize()
        _pack(out, 'inverse__%s_QFRC_INVERSE' % name, B.get('QFRC_INVERSE')); _pack(out, 'inverse__%s_CONTACT_FORCE' % name, B.get('CONTACT_FORCE'))
    assert np.abs(out['inverse__plain_CONTACT_FORCE']).max() > 0

    for f in ('QPOS', 'QVEL'):
        out['sources__' + f] = B.get(f)
        assert np.array_equal(out['sources__' + f], before[f]), f
    return out


def _flight(lib, dev):
    import torch
    from flybody_amd import engine
    from flybody_amd.reference import constant_speed_trajectory
    from flybody_amd.wbpg import build_tables
    B = engine.Batch(engine.Model.from_asset('flight_imitation', lib_path=lib), 2, precision=64)
    B.set_wbpg(build_tables(), seed=0)
    qp, qv = constant_speed_trajectory(200, 20.0, init_pos=(0, 0, 1), body_rot_angle_y=-47.5, control_timestep=2e-4)
    B.set_reference(qp, qv, future_steps=5, terminal_com_dist=2.0, time_limit=0.6)
    B.reset()
    nact = B.model.dim('nact')
    act = torch.empty(2, nact, device=dev)
    for k in range(3):
        B.random_actions(act.data_ptr(), k, seed=31, dist=0); B.step_ptr(act.data_ptr())
    B.synchronize()
    rows = (0.1*np.random.default_rng(37).normal(size=(2, 2, nact))).astype(np.float32)
    res = B.rollout(action=torch.from_numpy(rows).to(dev))
    out = {}
    _pack(out, 'flight_action__state', _np(res.state))
    out['flight_action__status'] = _np(res.status); out['flight_action__run'] = np.array([B.rollouts_run()], np.int64)
    return out


def _record(lib):
    """{'<case>__<array>': array} of one library."""
    import torch  # noqa: F401  (torch's HIP runtime must be the first one in the process: engine.load_library does this for its own two paths only)
    from flybody_amd import engine
    dev = 'cpu' if 'emulation' in engine.version(lib) else 'cuda'
    out = _walking(lib, dev)
    out.update(_flight(lib, dev))
    return out


@pytest.fixture(scope='module')
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


_got = {}


@pytest.fixture
def got(request):
    """The tree's results of one library, computed once for all its cases."""
    from flybody_amd import engine
    which = request.param
    if which not in _got:
        _got[which] = _record({'default': engine.HIP_LIB, 'dense': engine.HIP_LIB_DENSE}[which])
    return which, _got[which]


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('got', LIBS, indirect=True)
def test_side_kernels_equal_to_the_parent_to_the_bit(golden, got, case):
    which, rec = got
    mine = {'%s__%s' % (which, k): v for k, v in rec.items() if k.startswith(case + '__')}
    keys = [k for k in golden if k.startswith('%s__%s__' % (which, case))]
    assert mine and sorted(keys) == sorted(mine)
    for k, v in mine.items():
        g = golden[k]
        assert v.dtype == g.dtype and np.array_equal(v, g), (k, np.argwhere(v != g)[:4].tolist() if v.shape == g.shape else (v.shape, g.shape))


def test_golden_has_contacts_and_every_case(golden):
    """A record without contacts, or one that lost a case, must not pass silently."""
    for which in LIBS:
        assert (golden[which + '__NCON'] > 0).any() and (golden[which + '__NEFC'] > golden[which + '__NCON']).any()
        for case in CASES:
            assert [k for k in golden if k.startswith('%s__%s__' % (which, case))], (which, case)
        assert golden[which + '__deriv_centered__A__shape'].tolist()[0] == 2 and golden[which + '__deriv_forward__A__shape'].tolist()[0] == 1
        assert golden[which + '__rollout_rows__run'].tolist() == [3] and golden[which + '__feedback__run'].tolist() == [3]
        assert np.abs(golden[which + '__inverse__plain_CONTACT_FORCE']).max() > 0


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
    libs = [os.path.abspath(p) for p in sys.argv[1].split(',')]
    assert len(libs) == 2, 'LIB,LIB_DENSE'
    rec = {}
    for which, lib in zip(LIBS, libs):
        r = _record(lib)
        rec.update({'%s__%s' % (which, k): v for k, v in r.items()})
        print('%s: NCON %s NEFC %s, fd tickets %s / %s' % (which, r['NCON'].tolist(), r['NEFC'].tolist(), r['deriv_centered__tickets'].tolist(), r['deriv_forward__tickets'].tolist()))
    if len(sys.argv) > 2:
        np.savez_compressed(sys.argv[2], **rec)
        print('wrote %s: %d arrays, %d bytes' % (sys.argv[2], len(rec), os.path.getsize(sys.argv[2])))
        sys.exit(0)
    g = np.load(GOLDEN)
    bad = [k for k in rec if k not in g.files or rec[k].dtype != g[k].dtype or not np.array_equal(rec[k], g[k])] + [k for k in g.files if k not in rec]
    print('differs from the committed record: %s' % bad if bad else 'equal to the committed record (%d arrays)' % len(rec))
    sys.exit(1 if bad else 0)
