"""fb_batch_end_episode (fb_engine.hip: k_end_episode) through the kernel-source emulation build: masked MID environments turn LAST with
the caller's discount and come back FIRST at the start pose; unmasked, FIRST and already-LAST environments stay what a twin batch that
never made the call has, to the bit.  (reward_fn / termination_fn of BatchedFlyEnv are torch code on device views: tests/test_gpu_template_task.py.)
No GPU needed."""
import sys

import numpy as np
import pytest

from conftest import ROOT
import law_helpers as H

FIELDS = ('QPOS', 'QVEL', 'OBS', 'REWARD', 'DISCOUNT', 'STEP_TYPE', 'STEP_COUNT')


@pytest.fixture(scope='module')
def emu_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    return g.build_emu()


def _end(B, mask, disc=None):
    m = np.ascontiguousarray(mask, np.uint8)
    d = None if disc is None else np.ascontiguousarray(disc, np.float32)
    B.end_episode(m.ctypes.data, 0 if d is None else d.ctypes.data)          # (the emulation build's "device" memory is the host's)


@pytest.mark.parametrize('tickets', [True, False])
def test_end_episode_against_a_twin_that_never_calls_it(emu_lib, walk_arrays, reference_traj, tickets, monkeypatch):
    from flybody_amd import engine
    if tickets: monkeypatch.delenv('FB_NO_TICKETS', raising=False)
    else: monkeypatch.setenv('FB_NO_TICKETS', '1')
    qp, qv = reference_traj
    M = engine.Model(walk_arrays, lib_path=emu_lib)
    B, T = engine.Batch(M, 5, precision=64), engine.Batch(M, 5, precision=64)
    assert B.substep_scheduler == tickets
    for X in (B, T):
        X.set_reference(qp[:8], qv[:8], future_steps=2, terminal_com_dist=float('inf')); X.reset()      # the kernel's own LAST comes at step 5
    start = B.get('QPOS').copy()
    acts = np.random.default_rng(4).uniform(-0.7, 0.7, (7, 5, 59)).astype(np.float32)

    def step(k):
        a = np.ascontiguousarray(acts[k]); B.step_ptr(a.ctypes.data); T.step_ptr(a.ctypes.data)

    def same(envs, what):
        for name in FIELDS:
            assert np.array_equal(B.get(name)[envs], T.get(name)[envs]), (what, name)
    _end(B, np.ones(5), np.full(5, 0.5))                                     # every environment is FIRST: nothing happens
    same(slice(None), 'FIRST')
    step(0); step(1)
    same(slice(None), 'two steps after a call on FIRST environments')
    assert (B.get('STEP_TYPE') == 1).all()
    _end(B, [1, 0, 7, 0, 0], [0.3, 0.9, 0.4, 0.9, 0.9])
    assert B.get('STEP_TYPE').ravel().tolist() == [2, 1, 2, 1, 1]
    assert np.allclose(B.get('DISCOUNT').ravel(), [0.3, 1, 0.4, 1, 1], rtol=1e-7)
    same([1, 3, 4], 'unmasked')
    assert np.array_equal(B.get('QPOS'), T.get('QPOS')) and np.array_equal(B.get('REWARD'), T.get('REWARD'))      # the state itself is not touched
    step(2)
    assert B.get('STEP_TYPE').ravel().tolist() == [0, 1, 0, 1, 1]
    assert np.array_equal(B.get('QPOS')[[0, 2]], start[[0, 2]]) and not B.get('QVEL')[[0, 2]].any() and not B.get('STEP_COUNT')[[0, 2]].any()
    assert (B.get('REWARD').ravel()[[0, 2]] == 0).all() and (B.get('DISCOUNT').ravel()[[0, 2]] == 1).all()
    same([1, 3, 4], 'unmasked, a step later')
    step(3); step(4)
    assert T.get('STEP_TYPE').ravel().tolist() == [2]*5 and B.get('STEP_TYPE').ravel().tolist() == [1, 2, 1, 2, 2]
    _end(B, [0, 1, 0, 1, 1])                                                 # already LAST (the trajectory's end, discount 1): left alone
    same([1, 3, 4], 'already LAST')
    assert (B.get('DISCOUNT').ravel()[[1, 3, 4]] == 1).all()
    _end(B, [1, 0, 0, 0, 0])                                                 # no discount array: 0
    assert B.get('STEP_TYPE').ravel().tolist() == [2, 2, 1, 2, 2] and B.get('DISCOUNT').ravel().tolist() == [0, 1, 1, 1, 1]
    step(5)
    assert B.get('STEP_TYPE').ravel().tolist() == [0, 0, 1, 0, 0]
    same([1, 3, 4], 'auto-reset after the kernel\'s own LAST')
    assert np.array_equal(B.get('QPOS')[0], start[0])
    with pytest.raises(engine.EngineError, match='null argument'):
        B.end_episode(0)


def test_end_episode_on_the_template_task_with_a_law(emu_lib):
    """Every task, every step kernel: the template task under a control law."""
    from flybody_amd import engine
    M = engine.Model(H.template_arrays(), lib_path=emu_lib)
    B = H.template_batch(M, 3, time_limit=1.0)
    B.set_control_law(vel_gain=np.full(108, 1e-5))
    B.reset()
    start = B.get('QPOS').copy()
    a = np.random.default_rng(1).uniform(-0.5, 0.5, (3, 59)).astype(np.float32)
    B.step_ptr(a.ctypes.data)
    assert B.get('QFRC_LAW').any()
    _end(B, [0, 1, 0], [1, 0.25, 1])
    assert B.get('STEP_TYPE').ravel().tolist() == [1, 2, 1] and B.get('DISCOUNT').ravel().tolist() == [1, 0.25, 1]
    B.step_ptr(a.ctypes.data)
    assert B.get('STEP_TYPE').ravel().tolist() == [1, 0, 1] and np.array_equal(B.get('QPOS')[1], start[1])
    assert not B.get('QFRC_LAW')[1].any() and B.get('QFRC_LAW')[0].any()      # the forward pass of a reset skips the law
