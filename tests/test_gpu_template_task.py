"""template_task on the MI355X: the oracle twin over 110 control steps on both engine builds, the factory's surface (the reference's
tests/test_core.py restated), the action corruptor, and a task written in PyTorch on top of it -- reward_fn / termination_fn through
fb_batch_end_episode -- at 64 environments and on the ticket path."""
import numpy as np
import pytest

import law_helpers as H

pytestmark = pytest.mark.gpu

# the bound tests/test_gpu_parity.py holds for FP64 rollouts against the oracle
TOL_ROLLOUT = 1e-6


@pytest.mark.parametrize('dense', [False, True])
def test_template_twin_rollout_gpu(dense):
    """64 environments x 110 control steps at time_limit = 0.1: LAST at steps 50 and 101, FIRST right after, on both sides; the state is
    bit-equal to a walk_imitation batch after every step and within TOL_ROLLOUT of the oracle at EVERY step (measured on both
    builds: qpos 2.1e-9, qvel 7.9e-8 at worst)."""
    from flybody_amd import engine
    gaps, te, to, rew, disc = H.template_twin_rollout(engine.HIP_LIB_DENSE if dense else None, 64, 110, on_gpu=True)
    print('template twin %s build, 64 x 110: qpos %.2e qvel %.2e obs %.2e x allclose(1e-5, 1e-4)' % ('12-per-CU' if dense else 'default', gaps['qpos'], gaps['qvel'], gaps['obs']))
    assert gaps['qpos'] < TOL_ROLLOUT and gaps['qvel'] < TOL_ROLLOUT and gaps['obs'] < 1
    assert np.array_equal(te, to) and (te[49] == 2).all() and (te[50] == 0).all() and (te[100] == 2).all() and (te[101] == 0).all()
    assert (rew[te != 0] == 1).all() and (rew[te == 0] == 0).all() and (disc == 1).all()


def test_factory_restates_the_reference_core_test():
    """tests/test_core.py:23-69 of the reference: specs, key order, reward 1, a clean prev_action, the action corruptor."""
    from flybody_amd import fly_envs
    env = fly_envs.template_task()
    names = ['walker/' + k for k in H.CORE_OBS_NAMES]
    assert list(env.observation_spec()) == names and env.action_spec().shape == (59,)
    ts = env.reset()
    assert ts.first() and list(ts.observation) == names and all(isinstance(ts.observation[k], np.ndarray) for k in names)
    assert abs(ts.observation['walker/world_zaxis'][2] - 1) < 1e-6
    rng = np.random.default_rng(0)
    for _ in range(20):
        action = rng.uniform(-1, 1, 59)
        ts = env.step(action)
        assert ts.reward == 1 and ts.discount == 1
        assert np.isclose(action, env.task.prev_action).all()
    noise = rng.normal(scale=0.1, size=59)
    seen = []

    def corruptor(action, random_state):
        seen.append(random_state)
        return action + noise
    env2 = fly_envs.template_task(action_corruptor=corruptor, random_state=np.random.RandomState(3))
    plain = fly_envs.template_task()
    env2.reset(); plain.reset()
    for _ in range(5):
        clean = rng.uniform(-1, 1, 59)
        env2.step(clean); plain.step(clean.astype(np.float32) + noise)      # (the corruptor sees the float32 action the kernel would get)
        assert np.isclose(clean + noise, env2.task.prev_action).all()
    assert isinstance(seen[0], np.random.RandomState)
    assert np.array_equal(env2.batch.get('QPOS'), plain.batch.get('QPOS'))       # the kernel saw the corrupted action
    # time limit 1 s = 500 control steps by default; init_qpos moves the start
    env3 = fly_envs.template_task(init_qpos=[0.5, 0, 0.1278, 1, 0, 0, 0], time_limit=0.01, claw_friction=0.4)
    env3.reset()
    assert env3.batch.get('QPOS')[0, 0] == 0.5
    types = [int(env3.step(np.zeros(59)).step_type) for _ in range(7)]
    assert types == [1, 1, 1, 1, 2, 0, 1]


def _custom_task(n, dense=None, **kw):
    """The README's worked example: reward = forward velocimeter reading, the episode ends (discount 0) when the thorax drops below a
    height, a spring on the coxae."""
    import torch
    from flybody_amd import control_laws, fly_envs
    off = {}

    def reward_fn(env):
        o, _, _ = env.layout['velocimeter']
        return env.torch_views()['obs'][:, o]

    def termination_fn(env):
        return env.state_views()['qpos'][:, 2] < off['floor']              # the root body is the thorax
    env = fly_envs.template_task(n_env=n, reward_fn=reward_fn, termination_fn=termination_fn, time_limit=1.0, **kw)
    names = [str(x) for x in env.model.arrays['names_jnt']]
    env.set_control_law(control_laws.joint_spring(env.model, [x for x in names if x.startswith('coxa_abduct')], 0.5))
    return env, off, torch


def test_custom_reward_and_termination_at_64_environments():
    """reward_fn writes the reward view (0 on FIRST), termination_fn ends episodes through fb_batch_end_episode with discount 0, the ended
    environments come back FIRST at the start pose.  (The test reads the device after every step; step_tensor itself does not.)"""
    env, off, torch = _custom_task(64)
    v = env.reset_all(); torch.cuda.synchronize()
    z0 = float(env.state_views()['qpos'][:, 2][0])
    off['floor'] = z0 - 0.002                                                   # 20 um below the start height (the emulation build sees 0.123 .. 0.136 over such a rollout)
    g = torch.Generator(device='cuda'); g.manual_seed(1)
    ended = firsts = 0
    prev_last = torch.zeros(64, dtype=torch.bool, device='cuda')
    start = env.batch.get('QPOS')[0].copy()
    for k in range(26):
        act = (torch.rand(64, 59, device='cuda', generator=g) - 0.5).contiguous()
        v = env.step_tensor(act)
        st, rew, disc, obs = (v[x].clone() for x in ('step_type', 'reward', 'discount', 'obs'))
        o = env.layout['velocimeter'][0]
        assert torch.equal(rew, torch.where(st == 0, torch.zeros_like(rew), obs[:, o]))
        low = env.state_views()['qpos'][:, 2] < off['floor']
        last = st == 2
        assert bool((last[low & (st != 0)]).all())                              # every MID environment below the height is LAST now
        assert bool((last == (low & (st != 0))).all())                          # ... and nothing else is (the time limit, 1 s, is far)
        assert bool((disc[last] == 0).all()) and bool((disc[~last] == 1).all())
        assert bool(((st == 0) == prev_last).all())                             # LAST -> FIRST, nothing else resets
        if bool(prev_last.any()):
            q = env.batch.get('QPOS')
            assert np.array_equal(q[prev_last.cpu().numpy()], np.tile(start, (int(prev_last.sum()), 1)))
        ended += int(last.sum()); firsts += int((st == 0).sum())
        prev_last = last
    print('custom task, 64 environments x 26 steps: %d episodes ended by termination_fn, %d FIRST steps' % (ended, firsts))
    assert ended > 3 and firsts > 3
    assert env.batch.control_law_active and env.control_law()['qfrc_law'].abs().max() > 0


def test_custom_task_on_the_ticket_path():
    """4096 environments x 3 steps: the substep scheduler steps the batch, end_episode and the auto-reset work as at 64."""
    env, off, torch = _custom_task(4096)
    assert env.batch.substep_scheduler
    env.reset_all(); torch.cuda.synchronize()
    off['floor'] = 1e9                                                          # everything is "too low": every MID environment ends
    act = torch.zeros(4096, 59, device='cuda')
    types = []
    for k in range(3):
        v = env.step_tensor(act); torch.cuda.synchronize()
        types.append(v['step_type'].clone())
        assert bool((v['discount'][v['step_type'] == 2] == 0).all())
    assert bool((types[0] == 2).all()) and bool((types[1] == 0).all()) and bool((types[2] == 2).all())
    assert np.isfinite(env.batch.get('QPOS')).all() and not env.batch.get('WARN_EVER').any()
