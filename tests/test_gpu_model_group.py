"""Per-environment physics models in one batch (fb_batch_create_group, the kernels k_group_step / k_group_reset) on the
MI355X: a grouped batch against one CPU oracle per variant, against plain batches of its variants to the bit (both precisions, both
builds, both schedulers), reassignment at an episode boundary, applied forces on a group, and the fly_envs path.

The four variants of walk_imitation (flybody_amd.randomization.vary_model):
  V0 nominal;  V1 friction x 0.5, gain x 0.8, damping x 1.5;  V2 friction x 2, gain x 1.2, damping x 0.7, gravity + 0.1 |g| (cos 0.7, sin 0.7, 0);
  V3 per-body mass factors default_rng(7).uniform(0.8, 1.2, nbody), the world body's 1.
On the CPU oracle alone (16 environments per variant, 100 control steps of U(-0.5, 0.5) actions, terminal_com_dist inf; sampled after
every control step) they reach at most 11 / 11 / 10 / 11 contacts, 23 constraint rows each and 10 / 48 / 8 / 10 Newton iterations of
the 100 allowed; nothing is non-finite and no episode ends.  The tests assert the oracle's sizes inside the kernel's caps (64 contacts,
192 rows) and no engine warning."""
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

_rel = lambda a, b: np.abs(np.asarray(a).ravel() - np.asarray(b).ravel()).max() / max(np.abs(np.asarray(b)).max(), 1e-300)

# the project's bound for FP64 rollouts against the oracle (tests/test_gpu_parity.py, tests/test_gpu_forces.py)
TOL_ROLLOUT = 1e-6
FIELDS = ('QPOS', 'QVEL', 'OBS', 'REWARD', 'STEP_TYPE', 'SENSORDATA', 'WARN_EVER')
# Bits of WARN_EVER that the grouped path itself could raise (FB_WARN_MODEL_ID, FB_WARN_SCHED_WAIT).  The bit-for-bit tests feed U(-1, 1)
# actions, under which a solver warning is physics (measured: 1 of 4096 environments, a V1 one, reaches opt.iterations within 5 steps, in
# the plain batch of V1 as in the group): those tests compare WARN_EVER with the other side instead of asserting it zero.
OWN_WARN_BITS = 64 | 16
_cache = {}


def variants():
    if 'v' not in _cache:
        from flybody_amd.model_blob import load_npz
        from flybody_amd.randomization import vary_model
        a = dict(load_npz(os.path.join(ROOT, 'flybody_amd', 'assets', 'walk_imitation.npz')))
        g = np.asarray(a['opt_gravity'], float)
        f = np.random.default_rng(7).uniform(0.8, 1.2, len(a['body_mass'])); f[0] = 1
        _cache['v'] = [a, vary_model(a, friction_scale=0.5, gain_scale=0.8, damping_scale=1.5),
                       vary_model(a, friction_scale=2.0, gain_scale=1.2, damping_scale=0.7,
                                  gravity=g + 0.1*np.linalg.norm(g)*np.array([np.cos(0.7), np.sin(0.7), 0.0])),
                       vary_model(a, mass_scale=f)]
    return _cache['v']


def oracle_models(arrays_list=None):
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    if arrays_list is not None:
        return [fbo.OracleModel(pack_model(v)) for v in arrays_list]
    if 'om' not in _cache:
        _cache['om'] = [fbo.OracleModel(pack_model(v)) for v in variants()]
    return _cache['om']


def _reference(short=False):
    from flybody_amd.reference import default_walking_reference
    qp, qv = default_walking_reference()
    return (qp[:8], qv[:8], 2) if short else (qp, qv, 64)


def _batch(model, n, precision=64, short=False, time_limit=10.0):
    from flybody_amd import engine
    B = engine.Batch(model, n, precision=precision)
    qp, qv, fs = _reference(short)
    B.set_reference(qp, qv, future_steps=fs, terminal_com_dist=float('inf'), time_limit=time_limit); B.reset()
    return B


def _group(dense, arrays_list=None):
    from flybody_amd import engine
    return engine.ModelGroup(arrays_list if arrays_list is not None else variants(), dense=dense)


def _rollout(B, steps, seed, first=0):
    import torch
    act = torch.empty(B.n_env, B.model.dim('nact'), device='cuda')
    for k in range(first, first + steps):
        B.random_actions(act.data_ptr(), k, seed=seed, dist=1)
        B.step_ptr(act.data_ptr())
    torch.cuda.synchronize()


def _step(B, act):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(act, np.float32)).cuda()
    B.step_ptr(t.data_ptr(), torch.cuda.current_stream().cuda_stream); torch.cuda.synchronize()


@pytest.mark.parametrize('dense', [False, True])
def test_grouped_rollout_matches_one_oracle_per_variant(dense):
    """64 environments, env_model = e % 4, 100 control steps, both engine builds: every environment against an oracle of ITS variant."""
    from oracle import fbo
    n = 64
    group = _group(dense)
    B = _batch(group, n)
    assert B.n_models == 4 and B.get('ENV_MODEL').ravel().tolist() == [e % 4 for e in range(n)]
    qp, qv, _ = _reference()
    oms = oracle_models()
    ods = []
    for e in range(n):
        od = fbo.OracleData(oms[e % 4]); od.configure_env(qp, qv, terminal_com_dist=float('inf')); od.env_reset(); ods.append(od)
    rngs = [np.random.default_rng(2000 + e) for e in range(n)]
    trace, caps_ok = [], True
    for k in range(100):
        act = np.stack([r.uniform(-0.5, 0.5, 59) for r in rngs]).astype(np.float32)
        _step(B, act)
        fbo.step_batch(ods, act.astype(np.float64))
        caps_ok = caps_ok and all(int(od.scalar('ncon')) < 64 and int(od.scalar('nefc')) < 192 for od in ods)
        if (k + 1) % 10 == 0:
            Q, V = B.get('QPOS'), B.get('QVEL')
            trace.append((k + 1, max(_rel(Q[e], ods[e].field('qpos')) for e in range(n)), max(_rel(V[e], ods[e].field('qvel')) for e in range(n))))
    print('grouped rollout vs oracles, %s build, (step, qpos gap, qvel gap):' % ('12-per-CU' if dense else 'default'), ' '.join('(%d %.1e %.1e)' % t for t in trace))
    Q, V = B.get('QPOS'), B.get('QVEL')
    per_variant = [(max(_rel(Q[e], ods[e].field('qpos')) for e in range(v, n, 4)), max(_rel(V[e], ods[e].field('qvel')) for e in range(v, n, 4))) for v in range(4)]
    print('per variant (qpos, qvel):', ' '.join('V%d (%.1e %.1e)' % (v, *g) for v, g in enumerate(per_variant)))
    assert caps_ok and not B.get('WARN_EVER').any()
    assert B.get('STEP_TYPE').ravel().tolist() == [int(od.scalar('step_type')) for od in ods]
    assert max(t[1] for t in trace) < TOL_ROLLOUT and max(t[2] for t in trace) < TOL_ROLLOUT, trace


@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('precision', [64, 32])
def test_grouped_batch_equals_plain_batches_to_the_bit(precision, dense):
    """64 environments x 4 variants against four plain 64-environment batches (same environment indices, same actions), 30 control
    steps on the short reference, so that auto-resets (k_group_step's reset branch) happen."""
    n = 64
    group = _group(dense)
    G = _batch(group, n, precision, short=True)
    P = [_batch(m, n, precision, short=True) for m in group.models]
    for B in [G] + P:
        _rollout(B, 3, seed=11)
    assert not np.array_equal(P[0].get('QPOS')[0], P[1].get('QPOS')[0])      # (mid-episode: the variants differ)
    for B in [G] + P:
        _rollout(B, 27, seed=11, first=3)
    assert not (G.get('WARN_EVER') & OWN_WARN_BITS).any()
    seen = G.get('STEP_COUNT').ravel()
    assert seen.max() < 30                                                    # episodes ended and restarted on the way
    for f in FIELDS:
        g = G.get(f)
        for v in range(4):
            assert np.array_equal(g[v::4], P[v].get(f)[v::4]), (f, v)
    assert np.isfinite(G.get('QPOS')).all()


@pytest.mark.parametrize('dense', [False, True])
def test_substep_scheduler_bit_equal_to_per_wave_on_a_group(dense, monkeypatch):
    """4096 environments, 4 variants, 5 control steps: tickets (the model bound per ticket) against FB_NO_TICKETS=1 (per launch).  The
    smallest configuration that puts a grouped batch on the ticket path with the real slot counts."""
    out = []
    for tickets in (True, False):
        if tickets: monkeypatch.delenv('FB_NO_TICKETS', raising=False)
        else: monkeypatch.setenv('FB_NO_TICKETS', '1')
        group = _group(dense)
        B = _batch(group, 4096)
        assert B.substep_scheduler == tickets and B.n_models == 4
        _rollout(B, 5, seed=7)
        assert not (B.get('WARN_EVER') & OWN_WARN_BITS).any()
        out.append([B.get(f).copy() for f in FIELDS])
        del B, group
    assert np.isfinite(out[0][0]).all()
    for u, v in zip(*out):
        assert np.array_equal(u, v)


def test_reassignment_before_a_reset():
    """ENV_MODEL of 8 environments changed, those reset, 10 steps: they equal plain batches of the NEW variant to the bit."""
    n = 64
    group = _group(False)
    G = _batch(group, n)
    _rollout(G, 3, seed=3)                                                    # some history under the old assignment
    ids = np.arange(5, 5 + 8*7, 7)
    em = G.get('ENV_MODEL').copy()
    new = (em[ids, 0] + 1 + np.arange(8) % 3) % 4
    assert (new != em[ids, 0]).all()
    em[ids, 0] = new
    G.set('ENV_MODEL', em)
    G.reset(ids)
    P = [_batch(m, n) for m in group.models]
    for B in [G] + P:
        _rollout(B, 10, seed=5)
    assert not (G.get('WARN_EVER') & OWN_WARN_BITS).any()
    for f in FIELDS:
        g = G.get(f)
        for e, v in zip(ids, new):
            assert np.array_equal(g[e], P[v].get(f)[e]), (f, e, v)
    e, v = int(ids[0]), int(new[0])
    assert not np.array_equal(G.get('QPOS')[e], P[int((v + 1) % 4)].get('QPOS')[e])


def test_reassignment_while_last_takes_effect_at_the_first_observation():
    """A short time limit ends every episode; while the step type is LAST the id of every environment is changed through the device
    pointer (V0 -> V2, V2 -> V0; tilted gravity shows in the accelerometer of a FIRST observation).  The auto-reset of the next step
    runs under the new model: the FIRST observation and the steps behind it match a FRESH oracle of the new variant."""
    import torch
    from flybody_amd import fly_envs
    from oracle import fbo
    n = 16
    two = [variants()[0], variants()[2]]
    group = _group(False, two)
    B = _batch(group, n, time_limit=0.011)
    oms = [oracle_models()[0], oracle_models()[2]]
    qp, qv, _ = _reference()
    rng = np.random.default_rng(12)
    k = 0
    while not (B.get('STEP_TYPE') == 2).all():
        _step(B, rng.uniform(-0.5, 0.5, (n, 59))); k += 1
        assert k < 20
    assert k >= 3
    old = B.get('ENV_MODEL').ravel().copy()
    view = B.device_view('ENV_MODEL').view(n)
    view.copy_(1 - view); torch.cuda.synchronize()
    new = B.get('ENV_MODEL').ravel()
    assert (new == 1 - old).all()
    ods = []
    for e in range(n):
        od = fbo.OracleData(oms[new[e]]); od.configure_env(qp, qv, terminal_com_dist=float('inf'), time_limit=0.011); od.env_reset(); ods.append(od)
    wrong = fbo.OracleData(oms[old[0]]); wrong.configure_env(qp, qv, terminal_com_dist=float('inf'), time_limit=0.011); wrong.env_reset()
    _step(B, rng.uniform(-0.5, 0.5, (n, 59)))                                 # the auto-reset
    assert (B.get('STEP_TYPE') == 0).all()
    S, O = B.get('SENSORDATA'), B.get('OBS')
    lay = fly_envs.observation_layout(group, 64)[0]['accelerometer']
    gap_first = max(_rel(S[e], ods[e].field('sensordata')) for e in range(n))
    gap_wrong = _rel(S[0], wrong.field('sensordata'))
    print('FIRST observation after reassignment: sensordata gap to the new variant\'s oracle %.2e, to the old variant\'s %.2e' % (gap_first, gap_wrong))
    assert gap_first < TOL_ROLLOUT and gap_wrong > 1e-3
    for e in range(n):
        assert np.allclose(O[e], ods[e].field('obs'), rtol=1e-5, atol=1e-4)
    assert not np.allclose(O[0][lay[0]:lay[0] + 3], wrong.field('obs')[lay[0]:lay[0] + 3], rtol=1e-3, atol=1e-4)
    for _ in range(3):
        act = rng.uniform(-0.5, 0.5, (n, 59)).astype(np.float32)
        _step(B, act); fbo.step_batch(ods, act.astype(np.float64))
    Q, V = B.get('QPOS'), B.get('QVEL')
    eq, ev = max(_rel(Q[e], ods[e].field('qpos')) for e in range(n)), max(_rel(V[e], ods[e].field('qvel')) for e in range(n))
    print('3 steps into the new episode: qpos %.2e qvel %.2e' % (eq, ev))
    assert eq < TOL_ROLLOUT and ev < TOL_ROLLOUT
    assert B.get('STEP_TYPE').ravel().tolist() == [int(od.scalar('step_type')) for od in ods]
    assert not B.get('WARN_EVER').any()


def test_forces_on_a_group_gravity_identity():
    """The gravity identity of tests/test_gpu_forces.py on a two-variant group (V0, V3: other masses): xfrc_applied[b, :3] =
    body_mass_k[b] D on every body of an environment of variant k, against oracles of the variants at gravity g + D."""
    from oracle import fbo
    n, steps = 32, 50
    two = [variants()[0], variants()[3]]
    g = np.linalg.norm(two[0]['opt_gravity'])
    delta = 0.1*g*np.array([np.cos(0.7), np.sin(0.7), 0.0])
    tilted = []
    for v in two:
        t = dict(v); t['opt_gravity'] = np.asarray(v['opt_gravity'], float) + delta; tilted.append(t)
    oms = oracle_models(tilted)
    group = _group(False, two)
    B = _batch(group, n)
    nb = len(two[0]['body_mass'])
    xf = np.zeros((n, nb, 6))
    for e in range(n):
        xf[e, :, :3] = np.asarray(two[e % 2]['body_mass'])[:, None]*delta[None]
    B.set('XFRC_APPLIED', xf.reshape(n, -1))
    assert B.forces_active
    B.reset()
    qp, qv, _ = _reference()
    ods = []
    for e in range(n):
        od = fbo.OracleData(oms[e % 2]); od.configure_env(qp, qv, terminal_com_dist=float('inf')); od.env_reset(); ods.append(od)
    rngs = [np.random.default_rng(2000 + e) for e in range(n)]
    caps_ok = True
    for k in range(steps):
        act = np.stack([r.uniform(-0.5, 0.5, 59) for r in rngs]).astype(np.float32)
        _step(B, act); fbo.step_batch(ods, act.astype(np.float64))
        caps_ok = caps_ok and all(int(od.scalar('ncon')) < 64 and int(od.scalar('nefc')) < 192 for od in ods)
    Q, V = B.get('QPOS'), B.get('QVEL')
    eq, ev = max(_rel(Q[e], ods[e].field('qpos')) for e in range(n)), max(_rel(V[e], ods[e].field('qvel')) for e in range(n))
    print('forces on a group, gravity identity, %d steps: qpos %.2e qvel %.2e' % (steps, eq, ev))
    assert caps_ok and not B.get('WARN_EVER').any()
    assert eq < TOL_ROLLOUT and ev < TOL_ROLLOUT, (eq, ev)


def _resample_run(seed, steps):
    import torch
    from flybody_amd import fly_envs
    env = fly_envs.BatchedFlyEnv(n_env=256, models=variants(), resample_on_reset=True, time_limit=0.02, seed=seed, dense=False)
    v = env.reset_all()
    ids = [env.env_model().cpu().numpy().copy()]
    types = []
    act = torch.empty(256, env.model.dim('nact'), device='cuda')
    for k in range(steps):
        env.batch.random_actions(act.data_ptr(), k, seed=1, dist=1, stream=torch.cuda.current_stream().cuda_stream)
        v = env.step_tensor(act)
        torch.cuda.synchronize()
        types.append(v['step_type'].cpu().numpy().copy()); ids.append(env.env_model().cpu().numpy().copy())
    warn = env.batch.get('WARN_EVER').ravel()
    return np.array(ids), np.array(types), warn, env.batch.n_models


def test_fly_envs_resample_on_reset():
    """The public path: BatchedFlyEnv(models=[4 variants], resample_on_reset=True) over episodes that end (time limit 0.02 s = 11
    steps): ids change only where the step type was LAST, stay in range, are reproducible from the seed, and never trip the clamp."""
    from flybody_amd import engine
    ids, types, warn, nm = _resample_run(seed=3, steps=28)
    assert nm == 4 and ids[0].tolist() == [e % 4 for e in range(256)]
    assert ids.min() >= 0 and ids.max() < 4
    changed = ids[1:] != ids[:-1]
    assert changed.any() and not (changed & (types != 2)).any()              # only where the step just returned LAST
    last = types == 2
    assert last.sum() >= 2*256                                               # every environment ended at least two episodes
    assert 0.5 < changed.sum()/last.sum() < 0.95                             # a uniform draw from 4 keeps the id one time in four
    assert not (warn & engine.WARN_BITS['MODEL_ID']).any()
    ids2, types2, _, _ = _resample_run(seed=3, steps=28)
    assert np.array_equal(ids, ids2) and np.array_equal(types, types2)
    ids3, _, _, _ = _resample_run(seed=4, steps=28)
    assert not np.array_equal(ids, ids3)
