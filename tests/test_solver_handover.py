"""The end of the constraint stage (fb_constraint.hpp: d_constraint_a) without memory hand-overs.

For a system of at most 64 rows with its Delassus matrix in LDS -- matrix slot, parked factor or wide placement -- the FP64 Newton solver
hands the final force and the residual res = b + AR f to the noslip passes IN REGISTERS (fb_newton.hpp: NwOut), and the J'f pass behind
them takes the force from the same register: no fence waits for the store of efc_force, the force is not reloaded, res is one more
product of the solver instead of a column-by-column rebuild.  FB_NO_SOLVER_HANDOVER=1, read at model
load, keeps the hand-over through the environment's row.  The two differ in the ROUNDING of res only, so both are held against the FP64
oracle at the tolerances of tests/test_gpu_parity.py::test_solver_paths_by_system_size_gpu (1e-6 relative in FP64; 3e-2 in FP32, whose
build keeps the rebuild -- its residual is accumulated in FP64 -- and takes the switch without effect).  Systems of more than 64 rows
(d_newton_wide) keep the old hand-over: there the two settings must agree to the bit.

The states are the forward evaluations of tests/test_delassus_entry_lanes.py: systems of 0, 1, 3, 10, 11, 15, 16, 17, 33, 40 and 65 / 66
rows, with a common trunk (walk_imitation) and without one (walk_on_ball) -- the empty system, no friction contact, the register tile
(<= 16 rows), lane == row in the slot, the parked factor, the wide placement, d_newton_wide.

The noslip passes are a routine of their own now (d_noslip: block constants read once per solve, the two row updates of a visit in one
round of LDS reads) that d_pgs calls behind its sweeps.  Same operations in the same order: a model with opt_solver = 0 (PGS) must give the
parent commit's results TO THE BIT.  tests/golden/pgs_forward_parent_5c99d4a.npz holds them (NEFC, SOLVER_NITER, EFC_FORCE, QFRC_CONSTRAINT,
QACC of the same states, FP64 and FP32), computed by the parent's sources in a kernel-emulation build with -ffp-contract=off and without
-march=native: plain IEEE operations in source order, so the comparison does not depend on which products a compiler chooses to fuse
(the default emulation build lets g++ contract, and its choices move with any change of the surrounding code) nor on the machine."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_delassus_entry_lanes import BALL_STATES, SIZES, WALK_STATES, _state

FIELDS = (('EFC_FORCE', 'efc_force'), ('QFRC_CONSTRAINT', 'qfrc_constraint'), ('QACC', 'qacc'))
TOL = {64: 1e-6, 32: 3e-2}            # tests/test_gpu_parity.py::test_solver_paths_by_system_size_gpu
STATES = {'walk': (WALK_STATES, False), 'ball': (BALL_STATES, True)}


def _rel(a, b):
    a = np.asarray(a, float).ravel(); b = np.asarray(b, float).ravel()
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _set_switch(monkeypatch, flag):
    if flag is None: monkeypatch.delenv('FB_NO_SOLVER_HANDOVER', raising=False)
    else: monkeypatch.setenv('FB_NO_SOLVER_HANDOVER', flag)


@pytest.fixture(scope='module')
def emu_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    return g.build_emu()


@pytest.fixture(scope='module')
def strict_emu_lib():
    """The kernel sources as plain IEEE arithmetic in source order (see the module docstring)."""
    out = os.path.join(ROOT, 'tests', '_emu', 'libflybody_emu_strict.so')
    srcs = [os.path.join(b, f) for b, _, fs in os.walk(os.path.join(ROOT, 'flybody_amd', 'csrc')) for f in fs] + [os.path.join(ROOT, 'include', 'flybody_engine.h')]
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in srcs)):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-x', 'c++', '-DFB_EMULATE', '-DFB_BUILD_ID="strict"', '-shared', '-fPIC',
                               '-I' + os.path.join(ROOT, 'flybody_amd', 'csrc'), '-o', out, os.path.join(ROOT, 'flybody_amd', 'csrc', 'fb_engine.hip')], cwd=ROOT)
    return out


@pytest.fixture(scope='module')
def arrays(walk_arrays):
    from flybody_amd.model_blob import load_npz
    return {'walk': walk_arrays, 'ball': load_npz(os.path.join(ROOT, 'flybody_amd', 'assets', 'walk_on_ball.npz'))}


@pytest.fixture(scope='module')
def oracle_forward(arrays):
    """FP64 oracle forward evaluations of the states of one model, computed once per (model, precision): the FP32 cases start from the
    state rounded to single precision, as the engine holds it."""
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    cache, models = {}, {}

    def get(name, precision):
        if (name, precision) not in cache:
            if name not in models: models[name] = fbo.OracleModel(pack_model(arrays[name]))
            states, ball = STATES[name]
            res = []
            for s in states:
                q, v = _state(arrays[name], ball, *s)
                if precision == 32: q = q.astype(np.float32).astype(float); v = v.astype(np.float32).astype(float)
                od = fbo.OracleData(models[name]); od.field('qpos')[:] = q; od.field('qvel')[:] = v; od.call('forward')
                n = int(od.scalar('nefc'))
                res.append(dict(q=q, v=v, nefc=n, **{of: od.field(of).copy() for _, of in FIELDS}))
            cache[(name, precision)] = res
        return cache[(name, precision)]
    return get


def _forward(model_arrays, lib, ref, precision, **model_kw):
    from flybody_amd import engine
    M = engine.Model(model_arrays, lib_path=lib, **model_kw)
    B = engine.Batch(M, len(ref), precision=precision)
    B.set('QPOS', np.array([r['q'] for r in ref])); B.set('QVEL', np.array([r['v'] for r in ref])); B.forward()
    out = {f: B.get(f).copy() for f in ('NEFC', 'SOLVER_NITER', 'WARN_EVER') + tuple(f for f, _ in FIELDS)}
    del B, M
    return out


def _check_forward(got, ref, precision, tag):
    """every field of every environment against the oracle; the figures are printed before they are asserted"""
    worst = {}
    for e, r in enumerate(ref):
        n = r['nefc']
        for f, of in FIELDS:
            if f == 'EFC_FORCE' and n == 0: continue
            x, y = (got[f][e][:n], r[of][:n]) if f == 'EFC_FORCE' else (got[f][e], r[of])
            if np.abs(y).max() == 0: assert np.abs(x).max() == 0, (tag, e, f); continue
            worst[(e, n, f)] = _rel(x, y)
    k = max(worst, key=worst.get)
    print('%s FP%d: largest relative difference to the oracle %.2e at (environment, rows, field) %s' % (tag, precision, worst[k], k))
    bad = {k: v for k, v in worst.items() if not v < TOL[precision]}
    assert not bad, (tag, bad)


def _assert_sizes(nefc):
    assert set(SIZES) <= set(nefc) and any(32 < n <= 64 for n in nefc) and any(n > 64 for n in nefc), nefc


@pytest.mark.parametrize('precision', [64, 32])
@pytest.mark.parametrize('name', ['walk', 'ball'])
def test_forward_both_handovers_match_the_oracle(emu_lib, arrays, oracle_forward, name, precision, monkeypatch):
    ref = oracle_forward(name, precision)
    out = {}
    for flag in (None, '1'):
        _set_switch(monkeypatch, flag)
        out[flag] = _forward(arrays[name], emu_lib, ref, precision)
        nefc = out[flag]['NEFC'].ravel().tolist()
        _assert_sizes(nefc)
        assert nefc == [r['nefc'] for r in ref]
        _check_forward(out[flag], ref, precision, '%s, %s' % (name, 'hand-over through the row' if flag else 'hand-over in registers'))
    # d_newton_wide is untouched: beyond 64 rows the switch changes nothing
    for e, r in enumerate(ref):
        if r['nefc'] > 64:
            for f in ('SOLVER_NITER',) + tuple(f for f, _ in FIELDS):
                assert np.array_equal(out[None][f][e], out['1'][f][e]), (e, f)
    assert np.array_equal(out[None]['SOLVER_NITER'], out['1']['SOLVER_NITER'])          # the solver itself does not see the switch
    if precision == 32:           # the FP32 build keeps the rebuild
        for f, _ in FIELDS:
            assert np.array_equal(out[None][f], out['1'][f]), f


@pytest.mark.parametrize('precision', [64, 32])
@pytest.mark.parametrize('name', ['walk', 'ball'])
def test_pgs_path_equal_to_the_parent_to_the_bit(strict_emu_lib, arrays, name, precision):
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'pgs_forward_parent_5c99d4a.npz'))
    a = dict(arrays[name]); a['opt_solver'] = np.array(0, np.int32)          # mjtSolver numbering: 0 = PGS
    states, ball = STATES[name]
    ref = [dict(zip(('q', 'v'), _state(a, ball, *s))) for s in states]
    got = _forward(a, strict_emu_lib, ref, precision)
    _assert_sizes(got['NEFC'].ravel().tolist())
    assert np.abs(got['EFC_FORCE']).max() > 0 and int(got['SOLVER_NITER'].max()) > 1
    for f in ('NEFC', 'SOLVER_NITER') + tuple(f for f, _ in FIELDS):
        assert np.array_equal(got[f], g['%s_%d_%s' % (name, precision, f)]), f


ROLL_STEPS = 20


def _roll_actions(n):
    return np.random.default_rng(31).uniform(-1, 1, (ROLL_STEPS, n, 59)).astype(np.float32)


@pytest.fixture(scope='module')
def oracle_short_episodes(oracle_model, reference_traj):
    """3 oracle environments x 20 control steps of U(-1, 1) actions on an 8-frame reference: the episode ends and restarts several
    times inside the rollout (LAST -> FIRST).  Computed once for both settings."""
    from oracle import fbo
    qp, qv = reference_traj
    acts = _roll_actions(3)
    ods = []
    for _ in range(3):
        od = fbo.OracleData(oracle_model); od.configure_env(qp[:8], qv[:8], future_steps=2, terminal_com_dist=float('inf')); od.env_reset(); ods.append(od)
    types = []
    for k in range(ROLL_STEPS):
        fbo.step_batch(ods, acts[k].astype(np.float64)); types.append([int(od.scalar('step_type')) for od in ods])
    return acts, np.array(types), np.array([od.field('qpos').copy() for od in ods]), np.array([od.field('qvel').copy() for od in ods])


@pytest.mark.parametrize('flag', [None, '1'])
def test_rollout_through_auto_reset_matches_the_oracle(emu_lib, walk_arrays, reference_traj, oracle_short_episodes, flag, monkeypatch):
    from flybody_amd import engine
    qp, qv = reference_traj
    acts, types, oq, ov = oracle_short_episodes
    assert (types == 2).any() and (types == 0).any()               # the episode ended and restarted inside the rollout
    _set_switch(monkeypatch, flag)
    M = engine.Model(walk_arrays, lib_path=emu_lib)
    B = engine.Batch(M, 3, precision=64)                           # (the emulation build has 2 slots: the ticket path runs)
    B.set_reference(qp[:8], qv[:8], future_steps=2, terminal_com_dist=float('inf')); B.reset()
    seen = 0
    for k in range(ROLL_STEPS):
        a = np.ascontiguousarray(acts[k]); B.step_ptr(a.ctypes.data)
        assert B.get('STEP_TYPE').ravel().tolist() == types[k].tolist(), k
        seen = max(seen, int(B.get('NEFC').max()))
    assert seen > 0
    eq = max(_rel(B.get('QPOS')[e], oq[e]) for e in range(3)); ev = max(_rel(B.get('QVEL')[e], ov[e]) for e in range(3))
    print('emulation rollout, switch %s: qpos %.2e qvel %.2e relative to the oracle after %d control steps' % (flag, eq, ev, ROLL_STEPS))
    assert eq < 1e-6 and ev < 1e-6


# ------------------------------------------------------------------ on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize('precision', [64, 32])
@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('name', ['walk', 'ball'])
def test_gpu_forward_both_handovers_match_the_oracle(arrays, oracle_forward, name, dense, precision, monkeypatch):
    """The same states on the default and on the 12-per-CU library (there the LDS placements end at 54 rows: the 65 / 66-row states and
    nothing else of this list take the matrix from global memory)."""
    from flybody_amd import engine
    ref = oracle_forward(name, precision)
    out = {}
    for flag in (None, '1'):
        _set_switch(monkeypatch, flag)
        out[flag] = _forward(arrays[name], engine.HIP_LIB_DENSE if dense else None, ref, precision)
        assert out[flag]['NEFC'].ravel().tolist() == [r['nefc'] for r in ref]
        _check_forward(out[flag], ref, precision, '%s, %s library, %s' % (name, '12-per-CU' if dense else 'default', 'through the row' if flag else 'in registers'))
    assert np.array_equal(out[None]['WARN_EVER'], out['1']['WARN_EVER'])
    for e, r in enumerate(ref):
        if r['nefc'] > 64:
            for f, _ in FIELDS:
                assert np.array_equal(out[None][f][e], out['1'][f][e]), (e, f)


GPU_ENVS = 64


@pytest.fixture(scope='module')
def oracle_gpu_rollout(oracle_model, reference_traj):
    """64 oracle environments x 20 control steps, half under U(-0.5, 0.5), half under the bench's clipped N(0, 1); once for both
    libraries and both settings."""
    from oracle import fbo
    qp, qv = reference_traj
    rng = np.random.default_rng(77)
    acts = np.where(np.arange(GPU_ENVS)[None, :, None] < GPU_ENVS//2, rng.uniform(-0.5, 0.5, (ROLL_STEPS, GPU_ENVS, 59)),
                    np.clip(rng.normal(size=(ROLL_STEPS, GPU_ENVS, 59)), -1.0, 1.0)).astype(np.float32)
    ods = []
    for _ in range(GPU_ENVS):
        od = fbo.OracleData(oracle_model); od.configure_env(qp, qv, terminal_com_dist=float('inf')); od.env_reset(); ods.append(od)
    for k in range(ROLL_STEPS):
        fbo.step_batch(ods, acts[k].astype(np.float64))
    return acts, np.array([od.field('qpos').copy() for od in ods]), np.array([od.field('qvel').copy() for od in ods])


@pytest.mark.gpu
@pytest.mark.parametrize('dense', [False, True])
def test_gpu_rollout_both_handovers_match_the_oracle(oracle_gpu_rollout, reference_traj, dense, monkeypatch):
    """64 environments x 20 control steps with the ticket path forced (FB_TICKET_SLOTS=1, as tests/test_gpu_parity.py does): consecutive
    substeps of an environment run on different waves -- nothing of the hand-over may live longer than the stage."""
    import torch
    from flybody_amd import engine
    qp, qv = reference_traj
    acts, oq, ov = oracle_gpu_rollout
    dev = torch.from_numpy(acts).cuda()
    st = torch.cuda.current_stream().cuda_stream
    monkeypatch.setenv('FB_TICKET_SLOTS', '1'); monkeypatch.delenv('FB_NO_TICKETS', raising=False)
    warn = []
    for flag in (None, '1'):
        _set_switch(monkeypatch, flag)
        M = engine.Model.from_asset('walk_imitation', dense=dense)
        B = engine.Batch(M, GPU_ENVS, device=0, precision=64)
        assert B.substep_scheduler
        B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
        for k in range(ROLL_STEPS):
            B.step_ptr(dev[k].data_ptr(), st)
        torch.cuda.synchronize()
        Q, V = B.get('QPOS'), B.get('QVEL')
        eq = max(_rel(Q[e], oq[e]) for e in range(GPU_ENVS)); ev = max(_rel(V[e], ov[e]) for e in range(GPU_ENVS))
        print('GPU rollout, %s library, switch %s: qpos %.2e qvel %.2e relative to the oracle' % ('12-per-CU' if dense else 'default', flag, eq, ev))
        assert eq < 1e-6 and ev < 1e-6
        assert int(B.get('NEFC').max()) > 0
        warn.append(B.get('WARN_EVER').copy())
        del B, M
    assert np.array_equal(warn[0], warn[1])
