"""The stage machine of the step kernels (csrc/fb_step.hpp: d_run / s_run) keeps no workspace descriptor of its own: every pass it ran inline between
the stage calls sits inside a stage now.  That is a restatement -- same loads, same single add or subtract, same stores -- so
every kernel built from the interpreter must give the PARENT commit's results to the bit.  tests/golden/stage_glue_parent_c197808.npz was
recorded on an MI355X from libraries built from c197808, with this file's recorder:

    python tests/test_gpu_stage_glue.py LIB,LIB_DENSE OUT        (LIB,LIB_DENSE alone: compare with the committed files, exit status 1 = differs)

OUT is named like the committed record whose cases are to be recorded (RECORDS).  The second record, step_variants_parent_59dad35.npz, was
made the same way from libraries built from 59dad35, when the step kernels' rows, model-id flagging, parameter lists and launches were each
stated once: the variants the first record holds at FP64 only, at FP32, and the grouped kernel with forces.

What the file holds, per case: after the reset and after every control step, REWARD and STEP_TYPE in full and one 64-bit digest PER
ENVIRONMENT of QPOS, QVEL, ACT and OBS (the words of the row, each times an odd constant of its position, summed modulo 2^64: a change of any one
word changes the digest); QPOS in full at the end.  Digests instead of the states themselves because 96 environments x 13 samples of QPOS and
QVEL are 2 MB per FP64 case, against a limit of 1 MiB per committed file; equality of the digests is `np.array_equal` all the same.

Cases (each a few seconds):
  plain_{64,32}, plain_dense_64   96 environments x 12 control steps of walk_imitation, terminal_com_dist 0.02 (environments end and auto-reset,
                                  out of phase); before step 6 a host reset of five environments, after step 8 a MODE_FORWARD evaluation
                                  (fb_batch_forward); each ONCE PER SCHEDULER -- one environment per wave (FB_NO_TICKETS=1) and substep tickets
                                  forced (FB_TICKET_SLOTS=1, the switch of test_gpu_parity's scheduler stress test) -- against the same record:
                                  k_fly, k_fly_reset, both copies of the interpreter, the auto-reset branch, the last-substep epilogue, the
                                  zero-fill pass of a reset
  forces_64, law_64, group_64     32 environments x 6 steps: k_step_forces (qfrc_applied + xfrc_applied), k_step_law (a per-environment law),
                                  k_group_step / k_group_reset (two models), the same two schedulers
  forces_32, law_32, group_32,    (second record) the same at FP32, and a two-model group WITH the forces of forces_64: k_group_step<true>
  group_forces_64"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'stage_glue_parent_c197808.npz')
GOLDEN_VARIANTS = os.path.join(HERE, 'golden', 'step_variants_parent_59dad35.npz')
pytestmark = pytest.mark.gpu

DIGESTED = ('QPOS', 'QVEL', 'ACT', 'OBS')
TERMINAL_COM_DIST = 0.02      # (emulation build, 16 environments, these actions: the first episodes end at step 4, 1-8 environments per step from there on)


def _digest(a):
    """[n_env] uint64: one digest per environment row."""
    a = np.ascontiguousarray(a)
    w = a.reshape(a.shape[0], -1).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).astype(np.uint64)
    mult = (np.arange(w.shape[1], dtype=np.uint64)*np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x632BE59BD9B4E019)) | np.uint64(1)
    with np.errstate(over='ignore'):
        return (w*mult[None, :]).sum(axis=1, dtype=np.uint64)


def _arrays():
    from flybody_amd.model_blob import load_npz
    from flybody_amd import engine
    return dict(load_npz(os.path.join(engine.ASSETS, 'walk_imitation.npz')))


def _roll(B, steps, seed, events=None):
    """Reset, `steps` control steps of U(-1, 1) Philox actions; events: {k: callable(B)} run before step k (k == steps: after the last)."""
    import torch
    rec = {f: [] for f in DIGESTED + ('REWARD', 'STEP_TYPE')}

    def take():
        B.synchronize()
        for f in DIGESTED: rec[f].append(_digest(B.get(f)))
        for f in ('REWARD', 'STEP_TYPE'): rec[f].append(B.get(f).copy())
    out = {}
    B.reset(); take()
    act = torch.empty(B.n_env, B.model.dim('nact'), device='cuda')
    for k in range(steps + 1):
        if events and k in events:
            out.update(events[k](B))
        if k == steps: break
        B.random_actions(act.data_ptr(), k, seed=seed, dist=1); B.step_ptr(act.data_ptr()); take()
    out.update({('DIGEST_' + f if f in DIGESTED else f): np.array(v) for f, v in rec.items()})
    out['QPOS_END'] = B.get('QPOS').copy()
    out['WARN_EVER'] = B.get('WARN_EVER').copy()
    return out


def _host_reset(B):
    B.reset([0, 5, 17, 64, 95]); B.synchronize()
    return {'HOST_RESET_STEP_TYPE': B.get('STEP_TYPE').copy(), 'HOST_RESET_DIGEST_QPOS': _digest(B.get('QPOS')), 'HOST_RESET_DIGEST_OBS': _digest(B.get('OBS')),
            'HOST_RESET_DIGEST_QACC': _digest(B.get('QACC'))}


def _forward(B):
    B.forward(); B.synchronize()
    return {'FORWARD_DIGEST_QACC': _digest(B.get('QACC')), 'FORWARD_DIGEST_SENSORDATA': _digest(B.get('SENSORDATA')), 'FORWARD_DIGEST_QFRC_CONSTRAINT': _digest(B.get('QFRC_CONSTRAINT'))}


def _plain(lib, precision):
    from flybody_amd import engine
    from flybody_amd.reference import default_walking_reference
    qp, qv = default_walking_reference()
    B = engine.Batch(engine.Model(_arrays(), lib_path=lib), 96, precision=precision)
    B.set_reference(qp, qv, terminal_com_dist=TERMINAL_COM_DIST)
    return _roll(B, 12, seed=3, events={6: _host_reset, 8: _forward})


def _small(lib, kind, precision=64):
    from flybody_amd import engine
    from flybody_amd.randomization import vary_model
    from flybody_amd.reference import default_walking_reference
    a = _arrays(); n = 32
    qp, qv = default_walking_reference()
    rng = np.random.default_rng(9)
    model = engine.Model(a, lib_path=lib) if 'group' not in kind else \
        engine.ModelGroup([a, vary_model(a, friction_scale=0.5, gain_scale=0.8, damping_scale=1.5)], lib_path=lib)
    B = engine.Batch(model, n, precision=precision)
    B.set_reference(qp, qv, terminal_com_dist=TERMINAL_COM_DIST)
    nv, nb = len(a['dof_damping']), len(a['body_mass'])
    if 'forces' in kind:
        w = float(np.sum(a['body_mass']))*9.81
        xf = np.zeros((n, nb, 6)); xf[:, 1:, :3] = rng.normal(size=(n, nb - 1, 3))*w*0.02; xf[:, 1:, 3:] = rng.normal(size=(n, nb - 1, 3))*w*1e-3
        B.set('XFRC_APPLIED', xf.reshape(n, -1)); B.set('QFRC_APPLIED', rng.normal(size=(n, nv))*w*1e-3)
        assert B.forces_active
    if kind == 'law':
        hinge = np.asarray(a['jnt_type'])[np.asarray(a['dof_jntid'])] == 3
        k = float(np.median(a['jnt_stiffness'][a['jnt_stiffness'] > 0])); d = float(np.median(a['dof_damping'][a['dof_damping'] > 0]))
        B.set_control_law(bias=rng.normal(size=(n, nv))*k*0.03, act_gain=rng.uniform(-0.3, 0.3, (n, nv)), pos_gain=rng.uniform(0, k, (n, nv))*hinge,
                          pos_ref=rng.uniform(-0.3, 0.3, (n, nv)), vel_gain=rng.uniform(0, d, (n, nv)))
        assert B.control_law_active
    if 'group' in kind:
        assert B.n_models == 2
    return _roll(B, 6, seed=5, events={3: lambda B_: (B_.reset([1, 2, 30]), {})[1]})


# name -> (which library, rollout)
CASES = {'plain_64': (0, lambda lib: _plain(lib, 64)), 'plain_32': (0, lambda lib: _plain(lib, 32)), 'plain_dense_64': (1, lambda lib: _plain(lib, 64)),
         'forces_64': (0, lambda lib: _small(lib, 'forces')), 'law_64': (0, lambda lib: _small(lib, 'law')), 'group_64': (0, lambda lib: _small(lib, 'group')),
         'forces_32': (0, lambda lib: _small(lib, 'forces', 32)), 'law_32': (0, lambda lib: _small(lib, 'law', 32)), 'group_32': (0, lambda lib: _small(lib, 'group', 32)),
         'group_forces_64': (0, lambda lib: _small(lib, 'group_forces'))}
# committed record -> its cases
RECORDS = {GOLDEN: ('plain_64', 'plain_32', 'plain_dense_64', 'forces_64', 'law_64', 'group_64'),
           GOLDEN_VARIANTS: ('forces_32', 'law_32', 'group_32', 'group_forces_64')}
SCHEDULERS = {'per_wave': {'FB_NO_TICKETS': '1'}, 'tickets': {'FB_TICKET_SLOTS': '1'}}


def _run(name, sched, libs, setenv, delenv):
    import torch  # noqa: F401  (torch's HIP runtime must be the first one in the process: engine.load_library does this for its own two paths only)
    for v in ('FB_NO_TICKETS', 'FB_TICKET_SLOTS'): delenv(v)
    for k, v in SCHEDULERS[sched].items(): setenv(k, v)
    which, fn = CASES[name]
    return fn(libs[which])


def _load_records():
    """{array name: array} of every committed record; the case names are distinct, so the arrays' are."""
    out = {}
    for path, names in RECORDS.items():
        g = np.load(path)
        assert {k.split('__')[0] for k in g.files} == set(names), path
        out.update({k: g[k] for k in g.files})
    return out


@pytest.fixture(scope='module')
def golden():
    return _load_records()


@pytest.mark.parametrize('sched', list(SCHEDULERS))
@pytest.mark.parametrize('name', list(CASES))
def test_rollout_equal_to_the_parent_to_the_bit(golden, name, sched, monkeypatch):
    from flybody_amd import engine
    got = _run(name, sched, (engine.HIP_LIB, engine.HIP_LIB_DENSE), monkeypatch.setenv, lambda v: monkeypatch.delenv(v, raising=False))
    keys = [k for k in golden if k.startswith(name + '__')]
    assert sorted(keys) == sorted('%s__%s' % (name, f) for f in got)
    for f, v in got.items():
        g = golden['%s__%s' % (name, f)]
        assert v.dtype == g.dtype and np.array_equal(v, g), (f, np.argwhere(v != g)[:4].tolist() if v.shape == g.shape else (v.shape, g.shape))


def test_golden_reaches_the_branches():
    """A record that stops exercising a branch must not pass silently (index 0 of the per-step arrays is the state after the reset)."""
    golden = _load_records()
    for name in CASES:
        t = golden[name + '__STEP_TYPE'][1:, :, 0]
        assert ((t[:-1] == 2) & (t[1:] == 0)).any(), name                      # an episode ends, the next step auto-resets
        assert (t == 1).any(axis=0).all(), name                                # every environment also steps mid-episode
        if name.startswith('plain'):
            assert len({tuple(c) for c in t.T}) > 1, name                      # the environments fall out of phase
            assert (golden[name + '__HOST_RESET_STEP_TYPE'].ravel()[[0, 5, 17, 64, 95]] == 0).all()


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(HERE))
    libs = [os.path.abspath(p) for p in sys.argv[1].split(',')]
    assert len(libs) == 2, 'LIB,LIB_DENSE'
    setenv = os.environ.__setitem__; delenv = lambda v: os.environ.pop(v, None)
    rec, same = {}, True
    out = [p for p in RECORDS if len(sys.argv) > 2 and os.path.basename(p) == os.path.basename(sys.argv[2])]
    assert out or len(sys.argv) == 2, 'OUT is named like one of %s' % [os.path.basename(p) for p in RECORDS]
    for name in (RECORDS[out[0]] if out else CASES):
        runs = {s: _run(name, s, libs, setenv, delenv) for s in SCHEDULERS}
        for f, v in runs['per_wave'].items():
            if not np.array_equal(v, runs['tickets'][f]): same = False; print('%s: %s differs between the schedulers' % (name, f))
            rec['%s__%s' % (name, f)] = v
        t = runs['per_wave']['STEP_TYPE'][1:, :, 0]
        print('%s: LAST per step %s' % (name, (t == 2).sum(axis=1).tolist()))
    if len(sys.argv) > 2:
        np.savez_compressed(sys.argv[2], **rec)
        print('wrote %s: %d arrays, %d bytes' % (sys.argv[2], len(rec), os.path.getsize(sys.argv[2])))
    else:
        g = _load_records()
        bad = [k for k in rec if k not in g or not np.array_equal(rec[k], g[k])]
        print('differs from the committed records: %s' % bad if bad else 'equal to the committed records (%d arrays)' % len(rec))
        same = same and not bad
    sys.exit(0 if same else 1)
