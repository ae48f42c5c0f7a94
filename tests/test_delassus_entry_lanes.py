"""The Delassus matrix AR = Y Y' + R of a system of at most 64 rows is built with ONE LANE PER ENTRY of the packed lower triangle
(fb_constraint.hpp: ar_entry_lanes_t): pass k gives lane l the entry 64 k + l, the lane fetches the Y of its row and its column from their
owner lanes and accumulates the entry in exactly the order of the lane == column row loop it replaces (ar_from_registers_t), which stays in
the source behind FB_NO_AR_ENTRY_LANES=1 (read at model load).  Same sums in the same order: everything downstream of the matrix must be
equal TO THE BIT with and without the switch, for every environment -- at the sizes where the number of passes changes (10 -> 11 rows:
1 -> 2 passes, 15 -> 16: 2 -> 3), at the empty and the one-row system, beyond 32 rows, with a common trunk (walk_imitation) and without
one (walk_on_ball: a forest of limb trees, TRUNK = 0), in FP64 and FP32."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

SIZES = (0, 1, 3, 10, 11, 15, 16, 17)          # row counts every model / precision case must contain, plus one above 32

# (seed, joint spread, clip the joints into their ranges) of the states below; chosen on the CPU (kernel emulation) so that the
# systems have the sizes in the comment in FP64 and FP32 alike -- the tests assert them
WALK_STATES = [(0, 0.0, False), (17, 0.1, False), (105, 0.0, False), (1, 0.05, False), (178, 0.2, False), (45, 0.0, False),
               (53, 0.2, False), (212, 0.1, False), (49, 0.3, False), (16, 0.05, False), (10, 0.0, False)]      # 0 1 3 10 11 15 16 17 33 40 66 rows
BALL_STATES = [(1408, 0.4, True), (1502, 0.8, True), (1254, 0.8, True), (1004, 0.4, True), (1118, 0.8, True), (1016, 0.4, True), (1373, 0.6, True),
               (1052, 0.4, True), (38, 0.2, False), (37, 0.1, False), (7, 0.1, False)]                           # 0 3 1 10 11 15 16 17 33 40 65 rows


def _state(a, ball, seed, spread, clip):
    rng = np.random.default_rng(seed)
    nq, nv = len(a['qpos0']), len(a['dof_bodyid'])
    q = a['qpos0'].copy()
    if ball:            # tethered fly on a ball: hinge joints, then the ball's quaternion
        nj = nq - 4
        q[:nj] += rng.uniform(-spread, spread, nj)
        if clip:        # no joint-limit rows: what is left are the contacts of the legs that still reach the ball
            lo, hi = a['jnt_range'][:nj, 0], a['jnt_range'][:nj, 1]
            q[:nj] = np.where(a['jnt_limited'][:nj] != 0, np.clip(q[:nj], lo + 0.1*(hi - lo), hi - 0.1*(hi - lo)), q[:nj])
        bq = np.array([1., 0, 0, 0]) + rng.uniform(-0.3, 0.3, 4); q[nj:] = bq/np.linalg.norm(bq)
    else:               # free fly at a random height above / inside the floor
        q[7:] += rng.uniform(-spread, spread, nq - 7)
        q[2] = rng.uniform(0.10, 0.16)
        quat = np.array([1.0, 0, 0, 0]) + rng.uniform(-0.1, 0.1, 4); q[3:7] = quat/np.linalg.norm(quat)
    return q, rng.normal(size=nv)


@pytest.fixture(scope='module')
def emu_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    return g.build_emu()


@pytest.fixture(scope='module')
def ball_arrays():
    from flybody_amd.model_blob import load_npz
    return load_npz(os.path.join(ROOT, 'flybody_amd', 'assets', 'walk_on_ball.npz'))


def _set_switch(monkeypatch, flag):
    if flag is None: monkeypatch.delenv('FB_NO_AR_ENTRY_LANES', raising=False)
    else: monkeypatch.setenv('FB_NO_AR_ENTRY_LANES', flag)


def _forward_both(arrays, lib, states, ball, precision, monkeypatch):
    from flybody_amd import engine
    QV = [_state(arrays, ball, *s) for s in states]
    out = []
    for flag in (None, '1'):
        _set_switch(monkeypatch, flag)
        M = engine.Model(arrays, lib_path=lib)
        B = engine.Batch(M, len(QV), precision=precision)
        B.set('QPOS', np.array([q for q, _ in QV])); B.set('QVEL', np.array([v for _, v in QV])); B.forward()
        out.append({f: B.get(f).copy() for f in ('NEFC', 'EFC_FORCE', 'QACC')})
        del B, M
    return out


@pytest.mark.parametrize('precision', [64, 32])
def test_forward_equal_with_and_without_entry_lanes_walk(emu_lib, walk_arrays, precision, monkeypatch):
    new, old = _forward_both(walk_arrays, emu_lib, WALK_STATES, False, precision, monkeypatch)
    nefc = new['NEFC'].ravel().tolist()
    assert set(SIZES) <= set(nefc) and any(32 < n <= 64 for n in nefc), nefc
    assert np.isfinite(new['QACC']).all() and np.abs(new['EFC_FORCE']).max() > 0
    for f in ('NEFC', 'EFC_FORCE', 'QACC'):
        assert np.array_equal(new[f], old[f]), f


@pytest.mark.parametrize('precision', [64, 32])
def test_forward_equal_with_and_without_entry_lanes_ball(emu_lib, ball_arrays, precision, monkeypatch):
    """walk_on_ball has no common trunk (TRUNK = 0 instantiation)."""
    assert int(np.sum(ball_arrays['dof_parentid'] < 0)) > 1
    new, old = _forward_both(ball_arrays, emu_lib, BALL_STATES, True, precision, monkeypatch)
    nefc = new['NEFC'].ravel().tolist()
    assert set(SIZES) <= set(nefc) and any(32 < n <= 64 for n in nefc), nefc
    assert np.isfinite(new['QACC']).all() and np.abs(new['EFC_FORCE']).max() > 0
    for f in ('NEFC', 'EFC_FORCE', 'QACC'):
        assert np.array_equal(new[f], old[f]), f


def test_rollout_equal_with_and_without_entry_lanes(emu_lib, walk_arrays, reference_traj, monkeypatch):
    """4 environments x 8 control steps through an auto-reset (a short episode: the rollout crosses LAST -> FIRST)."""
    from flybody_amd import engine
    qp, qv = reference_traj
    acts = np.random.default_rng(13).uniform(-1, 1, (8, 4, 59)).astype(np.float32)
    out = []
    for flag in (None, '1'):
        _set_switch(monkeypatch, flag)
        M = engine.Model(walk_arrays, lib_path=emu_lib)
        B = engine.Batch(M, 4, precision=64)
        B.set_reference(qp[:8], qv[:8], future_steps=2, terminal_com_dist=float('inf')); B.reset()
        rec = []
        for k in range(8):
            a = np.ascontiguousarray(acts[k]); B.step_ptr(a.ctypes.data)
            rec.append([B.get(f).copy() for f in ('QPOS', 'QVEL', 'NEFC', 'OBS', 'STEP_TYPE')])
        out.append(rec)
        del B, M
    types = np.array([r[4].ravel() for r in out[0]])
    assert (types == 2).any() and (types == 0).any()               # the episode ended and restarted inside the rollout
    assert max(int(r[2].max()) for r in out[0]) > 0                # there were constraint rows
    for ra, rb in zip(*out):
        for x, y in zip(ra, rb):
            assert np.array_equal(x, y)


GPU_FIELDS = ('QPOS', 'QVEL', 'ACT', 'NEFC', 'EFC_FORCE', 'OBS')


def _gpu_rollout(model_kw, nenv, nsteps, nact, precision, monkeypatch, setup):
    import torch
    from flybody_amd import engine
    acts = torch.from_numpy(np.random.default_rng(21).uniform(-1, 1, (nsteps, nenv, nact)).astype(np.float32)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    out, seen = [], []
    for flag in (None, '1'):
        _set_switch(monkeypatch, flag)
        M = engine.Model.from_asset(**model_kw)
        B = engine.Batch(M, nenv, device=0, precision=precision)
        setup(B)
        for k in range(nsteps):
            B.step_ptr(acts[k].data_ptr(), stream)
            if flag is None:
                torch.cuda.synchronize(); seen.append(B.get('NEFC').copy())
        torch.cuda.synchronize()
        out.append([B.get(f).copy() for f in GPU_FIELDS])
        del B, M
    return out, np.array(seen)


@pytest.mark.gpu
@pytest.mark.parametrize('precision', [64, 32])
@pytest.mark.parametrize('dense', [False, True])
def test_gpu_walk_rollout_equal_with_and_without_entry_lanes(reference_traj, precision, dense, monkeypatch):
    """512 walk_imitation environments x 20 control steps of U(-1, 1) actions, on the default and on the 12-per-CU library."""
    qp, qv = reference_traj

    def setup(B):
        B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    (new, old), seen = _gpu_rollout(dict(name='walk_imitation', dense=dense), 512, 20, 59, precision, monkeypatch, setup)
    assert (seen[seen > 0] <= 16).any() and (seen >= 17).any(), (seen.min(), seen.max())
    for f, x, y in zip(GPU_FIELDS, new, old):
        assert np.array_equal(x, y), f


@pytest.mark.gpu
@pytest.mark.parametrize('precision', [64, 32])
def test_gpu_flight_rollout_equal_with_and_without_entry_lanes(precision, monkeypatch):
    """64 flight_imitation environments x 10 control steps."""
    from flybody_amd.mjcf_compile import qrot
    from flybody_amd.reference import constant_speed_trajectory
    from flybody_amd.wbpg import build_tables
    from flybody_amd import engine
    arr = engine.Model.from_asset('flight_imitation').arrays
    cq, cv = constant_speed_trajectory(200, 20.0, init_pos=(0, 0, 1), body_rot_angle_y=-47.5, control_timestep=2e-4)
    root = cq.copy()
    for i in range(len(root)):
        root[i, :3] = cq[i, :3] + qrot(cq[i, 3:], -arr['com_offset'])
    tabs = build_tables()

    def setup(B):
        B.set_wbpg(tabs, seed=3)
        B.set_reference(root, cv, future_steps=5, terminal_com_dist=2.0, time_limit=0.6); B.reset()
    (new, old), _ = _gpu_rollout(dict(name='flight_imitation'), 64, 10, 12, precision, monkeypatch, setup)
    assert np.isfinite(new[0]).all()
    for f, x, y in zip(GPU_FIELDS, new, old):
        assert np.array_equal(x, y), f
