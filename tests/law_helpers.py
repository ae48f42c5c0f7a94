"""Shared by the template_task / control-law tests of the emulation build and of the GPU: the oracle twins and the rollouts against them.
The oracle knows no template task and no control law, so parity is reached through identities."""
import os

import numpy as np

from conftest import ROOT

rel = lambda a, b: np.abs(np.asarray(a).ravel() - np.asarray(b).ravel()).max() / max(np.abs(np.asarray(b)).max(), 1e-300)

# the reference's tests/test_core.py:9-18
CORE_OBS_NAMES = ['accelerometer', 'actuator_activation', 'appendages_pos', 'force', 'gyro', 'joints_pos', 'joints_vel', 'touch', 'velocimeter', 'world_zaxis']
# the reference's test_ctrl_callback (tests/test_core.py:72-100)
CALLBACK_DOFS = [*range(6, 9), *range(42, 53), *range(75, 90)]


def walk_arrays():
    from flybody_amd.model_blob import load_npz
    return dict(load_npz(os.path.join(ROOT, 'flybody_amd', 'assets', 'walk_imitation.npz')))


def template_arrays(**kw):
    from flybody_amd import model_zoo
    return model_zoo.get_model(model_zoo.task_config('template_task', **kw), allow_compile=False)


def template_batch(M, n, time_limit=0.1, precision=64, init_qpos=None):
    """A batch of the template task as fly_envs.template_task sets it up: the "reference" is the start pose, twice."""
    from flybody_amd import engine
    B = engine.Batch(M, n, precision=precision)
    root = np.asarray(M.arrays['qpos0'][:7] if init_qpos is None else init_qpos, float)
    B.set_reference(np.tile(root, (2, 1)), np.zeros((2, 6)), future_steps=0, terminal_com_dist=float('inf'), time_limit=time_limit)
    return B


def stepper(B, on_gpu):
    """step(actions float32 [n, nact]) for a batch on the GPU or on the emulation build."""
    if on_gpu:
        import torch

        def step(act):
            t = torch.from_numpy(np.ascontiguousarray(act)).cuda(); B.step_ptr(t.data_ptr(), torch.cuda.current_stream().cuda_stream); torch.cuda.synchronize()
    else:
        def step(act):
            a = np.ascontiguousarray(act); B.step_ptr(a.ctypes.data)
    return step


def actions(n, steps, nact=59):
    """The existing rollout tests' actions: U(-0.5, 0.5), one generator per environment seeded 2000 + e.  [steps, n, nact] float32."""
    rngs = [np.random.default_rng(2000 + e) for e in range(n)]
    return np.stack([np.stack([r.uniform(-0.5, 0.5, nact) for r in rngs]) for _ in range(steps)]).astype(np.float32)


def template_twin_rollout(lib_path, n, steps, on_gpu, time_limit=0.1, options=None):
    """n template_task environments against their oracle twin: walk_imitation with terminal_com_dist = inf, the same time limit and the
    default reference (whose row 0 is qpos0[:7], the template's start pose).  Asserts of the ORACLE run that its only episode ends are
    the time limit's (a twin that terminates for a reason the template does not have would hide a difference) and that its systems stay
    far from the caps.  Also steps a walk_imitation batch of the same engine library side by side and asserts that the template's state
    equals it to the bit after every step: the template's physics IS the walking task's.
    options: model options (opt_*) set on both sides, e.g. opt_noslip_iterations = 0.
    Returns gaps = dict(qpos, qvel: the largest relative gap to the oracle over EVERY control step, where: the (step, environment) of
    the largest qvel gap, obs), the step types [steps, n] of both sides, rewards, discounts."""
    from flybody_amd import engine
    from flybody_amd.engine import observation_layout
    from flybody_amd.model_blob import pack_model
    from flybody_amd.reference import default_walking_reference
    from oracle import fbo
    wa, ta = walk_arrays(), dict(template_arrays())
    for k, v in (options or {}).items():
        wa[k] = np.array(v, dtype=np.asarray(wa[k]).dtype); ta[k] = wa[k]
    qp, qv = default_walking_reference()
    assert np.array_equal(qp[0], wa['qpos0'][:7])
    M = engine.Model(ta, lib_path=lib_path)
    B = template_batch(M, n, time_limit); B.reset()
    W = engine.Batch(engine.Model(wa, lib_path=lib_path), n, precision=64)
    W.set_reference(qp, qv, terminal_com_dist=float('inf'), time_limit=time_limit); W.reset()
    om = fbo.OracleModel(pack_model(wa))
    ods = []
    for _ in range(n):
        od = fbo.OracleData(om); od.configure_env(qp, qv, terminal_com_dist=float('inf'), time_limit=time_limit); od.env_reset(); ods.append(od)
    lt, nobs = observation_layout(M, 0)
    Mw = engine.Model(wa, lib_path=lib_path)
    lw, _ = observation_layout(Mw, 64)
    assert B.nobs == nobs and [k for k in lt if lt[k][1] > 0] == CORE_OBS_NAMES

    def obs_gap():
        O = B.get('OBS'); g = 0.0
        for e in range(n):
            oo = ods[e].field('obs')
            for k in CORE_OBS_NAMES:
                a, b = O[e, lt[k][0]:lt[k][0] + lt[k][1]], oo[lw[k][0]:lw[k][0] + lw[k][1]]
                g = max(g, float(np.max(np.abs(a - b)/(1e-4 + 1e-5*np.abs(b)))))      # (in units of the smoke test's allclose(rtol 1e-5, atol 1e-4))
        return g
    gaps = dict(qpos=0.0, qvel=0.0, obs=obs_gap(), where=None)
    step, wstep = stepper(B, on_gpu), stepper(W, on_gpu)
    acts = actions(n, steps)
    te, to, rew, disc = [], [], [], []
    max_ncon = max_nefc = 0
    for k in range(steps):
        step(acts[k]); wstep(acts[k]); fbo.step_batch(ods, acts[k].astype(np.float64))
        Q, V = B.get('QPOS'), B.get('QVEL')
        assert np.array_equal(Q, W.get('QPOS')) and np.array_equal(V, W.get('QVEL')), 'template_task left walk_imitation\'s physics at step %d' % (k + 1)
        gq, gv = max(rel(Q[e], ods[e].field('qpos')) for e in range(n)), max(rel(V[e], ods[e].field('qvel')) for e in range(n))
        if gv > gaps['qvel']:
            gaps['where'] = (k + 1, int(np.argmax([rel(V[e], ods[e].field('qvel')) for e in range(n)])))
        gaps['qpos'] = max(gaps['qpos'], gq); gaps['qvel'] = max(gaps['qvel'], gv)
        gaps['obs'] = max(gaps['obs'], obs_gap())
        te.append(B.get('STEP_TYPE').ravel().copy()); to.append(np.array([int(od.scalar('step_type')) for od in ods]))
        rew.append(B.get('REWARD').ravel().copy()); disc.append(B.get('DISCOUNT').ravel().copy())
        assert not any(int(od.scalar('should_terminate')) and not (od.scalar('time') >= time_limit - 1e-9) for od in ods)
        max_ncon = max(max_ncon, max(int(od.scalar('ncon')) for od in ods)); max_nefc = max(max_nefc, max(int(od.scalar('nefc')) for od in ods))
    te, to = np.array(te), np.array(to)
    # the oracle's only episode ends are the time limit's: LAST at control steps 50 and 101 (1-based), FIRST right after
    per = int(round(time_limit/2e-3))
    expect = np.ones(steps, int)
    for k in range(steps):
        c = (k + 1) % (per + 1)
        expect[k] = 2 if c == per else (0 if c == 0 else 1)
    assert (to == expect[:, None]).all(), 'the oracle twin ended an episode for a reason the template does not have'
    assert max_ncon < 32 and max_nefc < 96, (max_ncon, max_nefc)
    assert not B.get('WARN_EVER').any()
    return gaps, te, to, np.array(rew), np.array(disc)


def stiffness_pair(k_extra=None):
    """(engine arrays, oracle arrays, law rows) of identity (c): the oracle's jnt_stiffness is 1.5 x the shipped one, plus a spring on two
    hinges that have none; the engine runs the shipped model with pos_gain = 0.5 jnt_stiffness, pos_ref = qpos_spring and the same two."""
    a = walk_arrays()
    nv = len(a['dof_jntid'])
    jid = np.asarray(a['dof_jntid']); hinge = np.asarray(a['jnt_type'])[jid] == 3
    ks = np.asarray(a['jnt_stiffness'], float)
    free = [j for j in range(len(ks)) if a['jnt_type'][j] == 3 and ks[j] == 0]
    assert len(free) >= 2 and (ks > 0).sum() > 10
    extra = [free[0], free[len(free)//2]]
    k_extra = float(np.median(ks[ks > 0])) if k_extra is None else k_extra
    okk = 1.5*ks; okk[extra] = k_extra
    oa = dict(a); oa['jnt_stiffness'] = okk
    pos_gain = np.where(hinge, 0.5*ks[jid], 0.0)
    for j in extra:
        pos_gain[a['jnt_dofadr'][j]] = k_extra
    pos_ref = np.where(hinge, np.asarray(a['qpos_spring'])[np.asarray(a['jnt_qposadr'])[jid]], 0.0)
    assert pos_gain[:6].max() == 0 and len(pos_gain) == nv
    return a, oa, dict(pos_gain=pos_gain, pos_ref=pos_ref)


def motor_pair(g=0.2):
    """Identity (d): act_gain = g on every dof against an oracle whose actuators are (1 + g) times as strong: gain and bias parameters
    (randomization.vary_model's gain_scale) and the force range x (1 + g).  Every actuator is covered, the force clamp included: the
    adhesion actuators (body transmission) reach the dofs through qfrc_actuator as well -- their moment arms are the contact normals'
    Jacobians -- so the law scales them with the motors."""
    from flybody_amd.randomization import vary_model
    a = walk_arrays()
    oa = vary_model(a, gain_scale=1.0 + g)
    oa['actuator_forcerange'] = np.array(oa['actuator_forcerange'], float)*(1.0 + g)
    return a, oa, dict(act_gain=np.full(len(a['dof_jntid']), g))


def law_rollout(lib_path, pair, n, steps, on_gpu, with_law=True):
    """n walk_imitation environments with the law of `pair` (stiffness_pair / motor_pair) against the oracle on the pair's oracle model.
    Returns the largest relative qpos / qvel gap over the steps; with_law False: the same engine without the law (the check can fail)."""
    from flybody_amd import engine
    from flybody_amd.model_blob import pack_model
    from flybody_amd.reference import default_walking_reference
    from oracle import fbo
    a, oa, law = pair
    qp, qv = default_walking_reference()
    M = engine.Model(a, lib_path=lib_path)
    B = engine.Batch(M, n, precision=64)
    B.set_reference(qp, qv, terminal_com_dist=float('inf'))
    if with_law:
        B.set_control_law(**law)
    B.reset()
    om = fbo.OracleModel(pack_model(oa))
    ods = []
    for _ in range(n):
        od = fbo.OracleData(om); od.configure_env(qp, qv, terminal_com_dist=float('inf')); od.env_reset(); ods.append(od)
    step = stepper(B, on_gpu)
    acts = actions(n, steps)
    eq = ev = 0.0
    for k in range(steps):
        step(acts[k]); fbo.step_batch(ods, acts[k].astype(np.float64))
        assert all(int(od.scalar('ncon')) < 64 and int(od.scalar('nefc')) < 192 for od in ods)
        if (k + 1) % 10 == 0 or k == steps - 1:
            Q, V = B.get('QPOS'), B.get('QVEL')
            eq = max(eq, max(rel(Q[e], ods[e].field('qpos')) for e in range(n)))
            ev = max(ev, max(rel(V[e], ods[e].field('qvel')) for e in range(n)))
    if with_law:
        assert not B.get('WARN_EVER').any()
        assert B.get('STEP_TYPE').ravel().tolist() == [int(od.scalar('step_type')) for od in ods]
    return eq, ev
