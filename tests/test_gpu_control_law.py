"""Substep control laws (csrc/fb_law.hpp, k_step_law) on the MI355X: the stiffness and motor identities against the CPU oracle over 100
control steps of 64 environments on both engine builds, a zero law against the other step kernels, the reference's control-callback
test as a law, the substep scheduler against one environment per wave, the torch views, and an FP32 batch."""
import numpy as np
import pytest

import law_helpers as H

pytestmark = pytest.mark.gpu

# the bound tests/test_gpu_parity.py holds for FP64 rollouts against the oracle
TOL_ROLLOUT = 1e-6


def _walk_batch(n, dense=False, precision=64):
    from flybody_amd import engine
    from flybody_amd.reference import default_walking_reference
    M = engine.Model.from_asset('walk_imitation', dense=dense)
    B = engine.Batch(M, n, precision=precision)
    qp, qv = default_walking_reference()
    B.set_reference(qp, qv, terminal_com_dist=float('inf'))
    return M, B


def _rollout(B, steps, seed):
    import torch
    act = torch.empty(B.n_env, B.model.dim('nact'), device='cuda')
    for k in range(steps):
        B.random_actions(act.data_ptr(), k, seed=seed, dist=1)
        B.step_ptr(act.data_ptr())
    torch.cuda.synchronize()


@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('which', ['stiffness', 'motors'])
def test_law_identity_rollout_matches_oracle(which, dense):
    """Identities (c) and (d) of tests/test_control_law_emulation.py, 64 environments x 100 control steps, against the oracle (never
    against the engine itself).  Over 30 steps the changed constants move the oracle by 1e-2 and more: a kernel that ignores the law fails.
    Measured at any tenth step, both builds: stiffness qpos 3.0e-10 qvel 4.5e-8, motors 2.0e-9 / 1.4e-8."""
    from flybody_amd import engine
    pair = H.stiffness_pair() if which == 'stiffness' else H.motor_pair()
    eq, ev = H.law_rollout(engine.HIP_LIB_DENSE if dense else None, pair, 64, 100, on_gpu=True)
    print('%s identity, %s build, 64 x 100 control steps: qpos %.2e qvel %.2e' % (which, '12-per-CU' if dense else 'default', eq, ev))
    assert eq < TOL_ROLLOUT and ev < TOL_ROLLOUT, (eq, ev)


@pytest.mark.parametrize('dense', [False, True])
def test_zero_law_and_the_callback_law_at_4_environments(dense):
    """(a) an all-zero law equals k_step_forces with zero forces and k_fly, output for output; (f) the reference's test_ctrl_callback as
    a law: FB_QFRC_LAW == FB_QFRC_ACTUATOR * noise on its dofs after every step, zero elsewhere."""
    from flybody_amd.control_laws import ControlLaw
    out = []
    for kind in ('plain', 'forces', 'law'):
        M, B = _walk_batch(4, dense=dense)
        if kind == 'forces': B.set('QFRC_APPLIED', 0.0)
        if kind == 'law': B.set_control_law()
        B.reset(); _rollout(B, 6, seed=11)
        out.append({f: B.get(f) for f in ('QPOS', 'QVEL', 'OBS', 'REWARD', 'STEP_TYPE', 'QACC', 'SENSORDATA')})
        if kind == 'law':
            assert B.control_law_active and not B.get('QFRC_LAW').any()
    for f in out[0]:
        assert np.array_equal(out[0][f], out[2][f]) and np.array_equal(out[1][f], out[2][f]), f
    import torch
    M, B = _walk_batch(4, dense=dense)
    noise = np.sin(np.arange(len(H.CALLBACK_DOFS)))
    B.set_control_law(**ControlLaw.from_dofs(M, H.CALLBACK_DOFS, act_gain=noise).rows())
    B.reset()
    comp = [i for i in range(108) if i not in H.CALLBACK_DOFS]
    act = torch.empty(4, 59, device='cuda')
    for k in range(20):
        B.random_actions(act.data_ptr(), k, seed=2, dist=1); B.step_ptr(act.data_ptr()); torch.cuda.synchronize()
        u, fa = B.get('QFRC_LAW'), B.get('QFRC_ACTUATOR')
        assert np.abs(fa[:, H.CALLBACK_DOFS]).max() > 0
        assert np.allclose(u[:, H.CALLBACK_DOFS], fa[:, H.CALLBACK_DOFS]*noise, rtol=1e-14, atol=0) and (u[:, comp] == 0).all()


@pytest.mark.parametrize('dense', [False, True])
def test_substep_scheduler_bit_equal_to_per_wave_with_a_law(dense, monkeypatch):
    """4096 environments, per-environment random laws, 3 control steps: the ticket scheduler gives the results of FB_NO_TICKETS=1 to the bit."""
    a = H.walk_arrays()
    rng = np.random.default_rng(5)
    hinge = np.asarray(a['jnt_type'])[np.asarray(a['dof_jntid'])] == 3
    k = float(np.median(a['jnt_stiffness'][a['jnt_stiffness'] > 0])); d = float(np.median(a['dof_damping'][a['dof_damping'] > 0]))
    shape = (4096, 108)
    law = dict(bias=rng.normal(size=shape)*k*0.03, act_gain=rng.uniform(-0.3, 0.3, shape), pos_gain=rng.uniform(0, k, shape)*hinge,
               pos_ref=rng.uniform(-0.3, 0.3, shape), vel_gain=rng.uniform(0, d, shape))
    out = []
    for tickets in (True, False):
        if tickets: monkeypatch.delenv('FB_NO_TICKETS', raising=False)
        else: monkeypatch.setenv('FB_NO_TICKETS', '1')
        M, B = _walk_batch(4096, dense=dense)
        assert B.substep_scheduler == tickets
        B.set_control_law(**law); B.reset(); _rollout(B, 3, seed=7)
        out.append({f: B.get(f) for f in ('QPOS', 'QVEL', 'OBS', 'QFRC_LAW', 'STEP_TYPE')})
        assert not B.get('WARN_EVER').any()
    for f in out[0]:
        assert np.array_equal(out[0][f], out[1][f]), f
    assert np.abs(out[0]['QFRC_LAW']).max() > 0
    M, P = _walk_batch(64, dense=dense); P.reset(); _rollout(P, 3, seed=7)
    assert not np.array_equal(P.get('QVEL'), out[0]['QVEL'][:64])              # (the law matters)


def test_torch_views_rewrite_gains_between_steps():
    """BatchedFlyEnv.control_law(): the rows on the device, written from torch, are what the next step uses; qfrc_law is the kernel's u."""
    import torch
    from flybody_amd import control_laws, engine, fly_envs
    env = fly_envs.walk_imitation(n_env=8)
    with pytest.raises(engine.EngineError, match='no control law'):
        env.control_law()
    law = control_laws.ControlLaw(108, n_env=8)
    env.set_control_law(law)
    v = env.control_law()
    assert v['act_gain'].shape == (8, 108) and v['qfrc_law'].shape == (8, 108) and v['act_gain'].dtype == torch.float64
    v['act_gain'][3] = 0.25; v['bias'][5, 40] = 1e-3
    env.reset_all()
    act = (torch.rand(8, 59, device='cuda') - 0.5).contiguous()
    env.step_tensor(act); torch.cuda.synchronize()
    fa = torch.from_numpy(env.batch.get('QFRC_ACTUATOR')).cuda()
    u = v['qfrc_law']
    assert torch.allclose(u[3], 0.25*fa[3], rtol=1e-14, atol=0) and float(u[3].abs().max()) > 0
    assert float(u[5, 40]) == 1e-3 and int((u != 0).sum()) == int((u[3] != 0).sum()) + 1
    env.clear_control_law()
    assert not env.batch.control_law_active and not env.batch.forces_active


def test_fp32_batch_with_a_law_stays_finite():
    M, B = _walk_batch(64, precision=32)
    a = H.walk_arrays()
    _, _, law = H.stiffness_pair()
    B.set_control_law(act_gain=np.full(108, 0.2), vel_gain=np.asarray(a['dof_damping'])*0.5, **law)
    B.reset(); _rollout(B, 30, seed=3)
    assert np.isfinite(B.get('QPOS')).all() and np.isfinite(B.get('QVEL')).all() and np.isfinite(B.get('QFRC_LAW')).all()
    assert np.abs(B.get('QFRC_LAW')).max() > 0 and (B.get('STEP_TYPE') == 1).all()
    B.reset([40, 3, 63]); B.synchronize()                                    # a partial reset zeroes the law force of its environments only
    u = B.get('QFRC_LAW')
    assert not u[[3, 40, 63]].any() and (np.abs(np.delete(u, [3, 40, 63], 0)).max(1) > 0).all()
