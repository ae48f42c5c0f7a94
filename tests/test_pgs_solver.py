"""Block PGS (fb_constraint.hpp: d_pgs, selected by opt_solver = 0) against the FP64 oracle's PGS (oracle/fbo_constraint.c), which
tests/test_oracle_closed_form.py pins to an independent cone solver (SLSQP, KKT conditions, dual cost).  What runs only behind
opt_solver = 0: the two sweep loops (at most 64 rows: lane == row, row types on a ballot mask; more: three registers per lane), both
matrix placements (LDS and global pointer), the warm-start pass of d_constraint_a and its fall-back to zero force.  The kernel emulation
runs one lane per pair with exact division; fb_div / fb_rsqrt, v_readlane, the address-space-3 loads, the parked factor and the
12-per-CU library's thresholds exist on the GPU alone, so every comparison runs there as well, on both libraries.

States, dispatch table and assertions: tests/pgs_cases.py.  Three models: walk_imitation and walk_on_ball with opt_solver = 0, and
walk_imitation with opt_solver = 0 and opt_noslip_iterations = 0 ("walk_raw": no d_noslip behind the sweeps -- the raw PGS forces, the
quantity the closed-form tests pin).

TOLERANCES are the project's (tests/test_solver_handover.py: TOL, from tests/test_gpu_parity.py): FP64 1e-6 relative on EFC_FORCE,
QFRC_CONSTRAINT and QACC of every state (the sweeps stop on a 1e-8 bound on the scaled improvement, so the last sweep may differ: the
sweep counts are printed, not compared -- in FP64 emulation they differ by one or two already, 43 against 45 at 79 rows); FP32 3e-2 on QACC,
the forces are printed.  Rollouts: 1e-6 relative on qpos / qvel after 20 control steps, the project's rollout tolerance.

MEASURED, worst relative difference to the oracle over all states and models:
                                   FP64 EFC_FORCE   FP64 QFRC_CONSTRAINT   FP64 QACC   FP32 EFC_FORCE   FP32 QACC
  kernel emulation (CPU)           2.4e-9           1.2e-9                 2.0e-9      9.1e-3           6.5e-3
  MI355X, default library          3.4e-9           2.3e-9                 3.0e-9      4.5e-3           4.2e-3
  MI355X, 12-per-CU library        3.4e-9           2.3e-9                 3.0e-9      4.5e-3           4.2e-3
(the two libraries agree in every printed digit: the placement of the matrix does not change the arithmetic).  Rollouts, qpos / qvel:
emulation, 4 environments, 1.1e-11 / 1.0e-9 (8-frame reference) and 1.8e-11 / 1.1e-10 (full reference); MI355X, 64 environments, both
libraries, 7.7e-15 / 1.4e-12 and 5.4e-11 / 1.5e-10.  Some substep of every rollout runs all 100 sweeps: those results depend on where the
sweeps start, which is what holds the warm start to the oracle's.

WHAT A WRONG KERNEL WOULD TRIP (both tried on emulation builds of mutated sources, outside the repository):
  * res_axpy3<false> leaves out the second register (rows 64 ... 127 never see a friction block's change): the forward test fails on
    every state of more than 64 rows, 6e-3 (66 rows) ... 1e+26 on EFC_FORCE, QFRC_CONSTRAINT and QACC; states of at most 64 rows and the
    rollouts (at most 21 rows) do not notice, hence the PRESSED states;
  * the warm start's first zone test with the wrong sign (N <= mu T: a contact in the middle zone starts from zero force): the forward
    tests pass -- a forward evaluation of a set state starts from qacc_warmstart = 0 -- and both rollouts fail, qpos 9e-4 ... 2e-3 and
    qvel 2e-2 ... 4e-2 after 20 control steps against the bound of 1e-6."""
import os

import numpy as np
import pytest

from conftest import ROOT
from pgs_cases import (PRESSED, REQUIRED_ROWS, ROLL_CASES, ROLL_ENVS, ROW_CAP, SIZES, WALK_EXTRA, assert_columns, check_forward, check_rollout,
                       oracle_forward, oracle_rollout, pgs_arrays, placements, states)
from test_solver_handover import _forward

MODELS = {'walk': ('walk', None), 'ball': ('ball', None), 'walk_raw': ('walk', 0)}          # name -> (asset, opt_noslip_iterations)


@pytest.fixture(scope='module')
def emu_lib():
    import __graft_entry__ as g
    return g.build_emu()


@pytest.fixture(scope='module')
def arrays(walk_arrays):
    from flybody_amd.model_blob import load_npz
    base = {'walk': walk_arrays, 'ball': load_npz(os.path.join(ROOT, 'flybody_amd', 'assets', 'walk_on_ball.npz'))}
    return {name: pgs_arrays(base[asset], noslip) for name, (asset, noslip) in MODELS.items()}


@pytest.fixture(scope='module')
def oracle_pgs(arrays):
    """The oracle's PGS results of every state of one model, computed once per (model, precision)."""
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    cache, models = {}, {}

    def get(name, precision):
        if (name, precision) not in cache:
            if name not in models: models[name] = fbo.OracleModel(pack_model(arrays[name]))
            cache[(name, precision)] = oracle_forward(models[name], states(arrays[name], MODELS[name][0]), precision)
        return cache[(name, precision)]
    return get


@pytest.fixture(scope='module')
def oracle_rollouts(arrays, reference_traj):
    """8 oracle environments x 20 control steps per case, PGS with the model's noslip setting; computed once for the CPU and the GPU tests."""
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    model = fbo.OracleModel(pack_model(arrays['walk']))
    cache = {}

    def get(case):
        if case not in cache: cache[case] = oracle_rollout(model, reference_traj, case)
        return cache[case]
    return get


def test_states_reach_every_branch(arrays, oracle_pgs, emu_lib):
    """The oracle alone: the states have the properties the other tests rely on."""
    from flybody_amd import engine
    max_it = int(arrays['walk']['opt_iterations'])
    assert max_it == int(arrays['ball']['opt_iterations']) == 100 and int(arrays['walk']['opt_solver']) == 0
    assert int(arrays['walk']['opt_noslip_iterations']) > 0 and int(arrays['walk_raw']['opt_noslip_iterations']) == 0
    ref = {(name, p): oracle_pgs(name, p) for name in MODELS for p in (64, 32)}
    for name in MODELS:
        r64, r32 = ref[(name, 64)], ref[(name, 32)]
        assert [r['nefc'] for r in r64] == [r['nefc'] for r in r32], name          # equal row counts for the states rounded to single precision
        assert set(SIZES) <= {r['nefc'] for r in r64} and any(r['nefc'] > 64 for r in r64), name
        assert any(r['niter'] > 1 for r in r64) and any(np.abs(r['efc_force']).max() > 0 for r in r64), name
    walk = ref[('walk', 64)]
    nefc = [r['nefc'] for r in walk]
    print('walk_imitation: (rows, contacts, sweeps)', [(r['nefc'], r['ncon'], r['niter']) for r in walk])
    assert nefc == [r['nefc'] for r in ref[('walk_raw', 64)]]
    assert set(REQUIRED_ROWS) <= set(nefc) and any(56 <= n <= 63 for n in nefc), sorted(nefc)
    assert nefc[-len(PRESSED) - len(WALK_EXTRA):] == [23, 24, 43, 44, 46, 47, 54, 55, 56, 60, 63, 64, 65, 79, 90, 114, 129, 153, 158, 192]
    # the thresholds of the default build (the emulation library is one) and the columns they make; the 12-per-CU library's are read
    # from that library on the GPU (test_gpu_forward_matches_the_oracle) -- 23 | 24 and 54 | 55 are in REQUIRED_ROWS
    pl = placements(engine.Model(arrays['walk'], lib_path=emu_lib))
    assert pl == {64: (43, 64), 32: (46, 64)}, pl
    for p in (64, 32): assert_columns(nefc, *pl[p])
    assert_columns(nefc, 23, 54)
    # a friction block across each register boundary, starting two rows and one row in front of it
    for b in (64, 128):
        for first in (b - 2, b - 1):
            assert any(first in r['blocks'] and r['nefc'] > b for r in walk), (b, first)
    # both ends of the sweep loop, on the lane == row loop and on the three-register loop
    for lo, hi in ((1, 64), (65, ROW_CAP)):
        its = [r['niter'] for r in walk if lo <= r['nefc'] <= hi]
        assert max_it in its and any(1 < k < max_it for k in its), (lo, hi, its)
    # the row cap: 64 contacts, and no other state is near it
    assert [r['ncon'] for r in walk if r['nefc'] == ROW_CAP] == [64] and all(r['ncon'] < 64 for r in walk if r['nefc'] != ROW_CAP)


@pytest.mark.parametrize('precision', [64, 32])
@pytest.mark.parametrize('name', list(MODELS))
def test_forward_matches_the_oracle(emu_lib, arrays, oracle_pgs, name, precision):
    ref = oracle_pgs(name, precision)
    got = _forward(arrays[name], emu_lib, ref, precision)
    check_forward(got, ref, precision, '%s, emulation' % name, int(arrays[name]['opt_iterations']))


@pytest.mark.parametrize('case', list(ROLL_CASES))
def test_rollout_matches_the_oracle(emu_lib, arrays, reference_traj, oracle_rollouts, case):
    """The warm start from the previous acceleration and its fall-back run only between steps: 4 environments x 20 control steps."""
    from flybody_amd import engine
    ref = oracle_rollouts(case)
    n = ROLL_ENVS//2
    M = engine.Model(arrays['walk'], lib_path=emu_lib)
    B = engine.Batch(M, n, precision=64)                           # (the emulation build has 2 slots: the ticket path runs)

    def step(k):
        a = np.ascontiguousarray(ref['acts'][k][:n]); B.step_ptr(a.ctypes.data)
    check_rollout(B, n, reference_traj, case, ref, step, 'emulation')


# ------------------------------------------------------------------ on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize('precision', [64, 32])
@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('name', list(MODELS))
def test_gpu_forward_matches_the_oracle(arrays, oracle_pgs, name, dense, precision):
    from flybody_amd import engine
    lib = engine.HIP_LIB_DENSE if dense else None
    ref = oracle_pgs(name, precision)
    if name == 'walk':
        # this library's thresholds, read off its LdsCfg: the states sit on both sides of each
        pl = placements(engine.Model(arrays[name], lib_path=lib))
        assert pl == ({64: (23, 54), 32: (46, 64)} if dense else {64: (43, 64), 32: (46, 64)}), pl
        assert_columns([r['nefc'] for r in ref], *pl[precision])
    got = _forward(arrays[name], lib, ref, precision)
    check_forward(got, ref, precision, '%s, %s library' % (name, '12-per-CU' if dense else 'default'), int(arrays[name]['opt_iterations']))


GPU_COPIES = 8


@pytest.mark.gpu
@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('case', list(ROLL_CASES))
def test_gpu_rollout_matches_the_oracle(arrays, reference_traj, oracle_rollouts, case, dense, monkeypatch):
    """The oracle's 8 environments x 20 control steps with the ticket path forced (FB_TICKET_SLOTS=1, as tests/test_solver_handover.py
    does): consecutive substeps of an environment run on different waves.  The batch holds 8 copies of the 8 environments, each copy
    compared: a wave draws its tickets from the queue of its own XCD, so the forced ticket path steps every environment only if the
    launch has a workgroup on every XCD -- 64 environments are 16 workgroups of the 12-per-CU library (4 environments each), 8 are
    two, and then six of the eight queues are never drawn (measured: environments 2 ... 7 keep STEP_TYPE 0; the same with Newton).  The
    product takes the ticket path only for batches beyond the resident slots, thousands of workgroups."""
    import torch
    from flybody_amd import engine
    ref = oracle_rollouts(case)
    n = GPU_COPIES*ROLL_ENVS
    dev = torch.from_numpy(np.ascontiguousarray(np.tile(ref['acts'], (1, GPU_COPIES, 1)))).cuda()
    st = torch.cuda.current_stream().cuda_stream
    monkeypatch.setenv('FB_TICKET_SLOTS', '1'); monkeypatch.delenv('FB_NO_TICKETS', raising=False)
    M = engine.Model(arrays['walk'], dense=dense)
    B = engine.Batch(M, n, device=0, precision=64)
    assert B.substep_scheduler

    def step(k):
        B.step_ptr(dev[k].data_ptr(), st); torch.cuda.synchronize()
    check_rollout(B, n, reference_traj, case, ref, step, 'GPU, %s library' % ('12-per-CU' if dense else 'default'))
