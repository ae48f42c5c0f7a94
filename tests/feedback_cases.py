"""The assertions on fb_batch_rollout_feedback (csrc/fb_rollout.hpp: k_closedloop_rollout), stated once for the emulation build
(tests/test_rollout_feedback_emulation.py) and the MI355X (tests/test_gpu_rollout_feedback.py).  Test helper, not a test.

A `Ctx` carries what differs between the two: how a tensor reaches the batch's memory and comes back, how the device is synchronised,
and how a batch of the four walking frames of tests/test_rollout_emulation.py (two in the air, two settled in contact) is made.
Shapes: 4 - 8 rollouts, T = 3 intervals of 1 or 2 substeps."""
import types

import numpy as np

PARITY = 1e-6                     # tests/test_gpu_parity.py's contract: max |difference| over max |reference| of a vector
STATE_FIELDS = ('QPOS', 'QVEL', 'ACT', 'QACC', 'WARN_EVER', 'SIZE_STATS')       # (what a later control step reads)
T = 3


class Ctx:
    def __init__(self, a, frames, make_batch, dev, np_, sync=lambda: None):
        self.a, self.frames, self.make_batch, self.dev, self.np_, self.sync = a, frames, make_batch, dev, np_, sync
        self.shim = types.SimpleNamespace(arrays=a)       # what lqr.state_difference / derivatives.integrate_pos need of a model
        self.nq, self.nv, self.nu = len(a['qpos0']), len(a['dof_bodyid']), len(a['actuator_ctrlrange'])
        self.na = int((np.asarray(a['actuator_actadr']) >= 0).sum())
        self.nx, self.ndx = self.nq + self.nv + self.na, 2*self.nv + self.na
        self.lo, self.hi = np.asarray(a['actuator_ctrlrange'], float).T
        self.limited = np.asarray(a['actuator_ctrllimited']).astype(bool)
        self.x0 = np.array([np.r_[f[0], f[1], f[2]] for f in frames])            # the sources' states [4, nx]


def rel_err(got, ref):
    got, ref = np.asarray(got, float).ravel(), np.asarray(ref, float).ravel()
    return float(np.abs(got - ref).max()/max(np.abs(ref).max(), 1e-300))


def nominals(c, envs, seed, spread=0.01):
    """x_nom [n_nom, T, nx], u_nom [n_nom, T, nu]: nominal m stays near the state of environment envs[m] -- a tangent step of size `spread`
    away, rotation of the root included -- and differs for every t and every m; u_nom mid-range."""
    from flybody_amd import derivatives
    from test_deriv_emulation import mid_ctrl
    rng = np.random.default_rng(seed)
    x = np.empty((len(envs), T, c.nx)); u = np.empty((len(envs), T, c.nu))
    for m, e in enumerate(envs):
        for t in range(T):
            q, v, act = c.frames[e][:3]
            x[m, t] = np.r_[derivatives.integrate_pos(c.shim, q, spread*rng.normal(size=c.nv)), v + spread*rng.normal(size=c.nv),
                            act + spread*rng.normal(size=c.na)]
            u[m, t] = mid_ctrl(c.a, rng)
    return x, u


def dense_gains(c, n_nom, seed, scale=1.0):
    """K [n_nom, T, nu, ndx], k [n_nom, T, nu]: dense, every row scaled by its actuator's range so that a tangent distance of a few
    hundredths moves the input by a fraction of the range -- a few inputs saturate, most do not.  The velocity columns are a hundred
    times smaller: joint velocities leave their nominal by whole units within an interval."""
    rng = np.random.default_rng(seed)
    width = (c.hi - c.lo)[:, None]
    K = scale*width*rng.normal(size=(n_nom, T, c.nu, c.ndx))
    K[..., c.nv:2*c.nv] *= 0.01
    k = 0.05*width[:, 0]*rng.normal(size=(n_nom, T, c.nu))
    return K, k


def formula(c, res_state, ids, noms, x_nom, u_nom, K, k, alpha):
    """u [n, T, nu] of the feedback law in numpy FP64 from the RECORDED states: x_0 = the source's state, x_t = state[t - 1]."""
    from flybody_amd import lqr
    n = len(ids)
    u = np.empty((n, T, c.nu))
    for r in range(n):
        for t in range(T):
            x = c.x0[ids[r]] if t == 0 else res_state[r, t - 1]
            dx = lqr.state_difference(c.shim, x, x_nom[noms[r], t])
            v = u_nom[noms[r], t] + ((1.0 if alpha is None else alpha[r])*(0 if k is None else k[noms[r], t]) + (0 if K is None else K[noms[r], t] @ dx))
            u[r, t] = np.where(c.limited, np.clip(v, c.lo, c.hi), v)
    return u


def run(c, batch, x_nom, u_nom, K=None, k=None, alpha=None, **kw):
    d = lambda x: None if x is None else c.dev(np.ascontiguousarray(x, np.float64))
    return batch.rollout_feedback(d(x_nom), d(u_nom), d(K), d(k), d(alpha), **kw)


def same_physics(c, a, b):
    assert np.array_equal(c.np_(a.state), c.np_(b.state)) and np.array_equal(c.np_(a.status), c.np_(b.status))
    if a.sensordata is not None and b.sensordata is not None:
        assert np.array_equal(c.np_(a.sensordata), c.np_(b.sensordata))


# ------------------------------------------------------------------ 1
def degenerate_cases_are_the_open_loop_bits(c, batch):
    x_nom, u_nom = nominals(c, [0, 1, 2, 3], seed=31)
    open_ = batch.rollout(ctrl=c.dev(u_nom), n_substeps=2, sensors=True)
    assert c.np_(open_.status).tolist() == [0]*4
    zero = run(c, batch, x_nom, u_nom, np.zeros((4, T, c.nu, c.ndx)), np.zeros((4, T, c.nu)), n_substeps=2, sensors=True)
    null = run(c, batch, x_nom, u_nom, n_substeps=2, sensors=True)
    k = 0.1*np.random.default_rng(32).normal(size=(4, T, c.nu))
    off = run(c, batch, x_nom, u_nom, None, k, np.zeros(4), n_substeps=2, sensors=True)
    on = run(c, batch, x_nom, u_nom, None, k, None, n_substeps=2, sensors=True)
    for r in (zero, null, off):
        same_physics(c, r, open_)
        assert np.array_equal(c.np_(r.ctrl), u_nom)
    assert not np.array_equal(c.np_(on.state), c.np_(open_.state))              # (the same k with alpha = 1 does move the rollouts)


# ------------------------------------------------------------------ 2, 3
def closed_loop_is_open_loop_on_its_own_inputs_and_the_inputs_are_the_formula(c, batch, tag):
    ids, noms = [0, 1, 2, 3, 2, 3], [0, 1, 2, 3, 2, 3]
    x_nom, u_nom = nominals(c, [0, 1, 2, 3], seed=41)
    K, k = dense_gains(c, 4, seed=42, scale=1.5)
    alpha = np.array([1.0, 0.5, 1.0, 0.25, 0.0, 2.0])
    worst = 0.0
    for nsub in (1, 2):
        res = run(c, batch, x_nom, u_nom, K, k, alpha, nom_ids=noms, env_ids=ids, n_substeps=nsub, sensors=True)
        u = c.np_(res.ctrl)
        sat = ((u == c.lo) | (u == c.hi)) & c.limited
        assert sat.any() and sat.mean() < 0.5 and np.isfinite(c.np_(res.state)).all(), (sat.sum(), sat.size)
        assert sat[2:4].any(), 'no input of a frame in contact saturates'
        # 2: the recorded inputs through the open-loop kernel, from the same environments: the same bits
        open_ = batch.rollout(ctrl=res.ctrl, env_ids=ids, n_substeps=nsub, sensors=True)
        same_physics(c, res, open_)
        # 3: the inputs against numpy, vector by vector
        ref = formula(c, c.np_(res.state), ids, noms, x_nom, u_nom, K, k, alpha)
        err = max(rel_err(u[r, t], ref[r, t]) for r in range(len(ids)) for t in range(T))
        print(f'{tag}: n_substeps {nsub}: inputs against the formula in numpy {err:.1e}  bound {PARITY:.0e}  saturated {int(sat.sum())} of {sat.size}')
        worst = max(worst, err)
    assert worst <= PARITY, worst


# ------------------------------------------------------------------ 4
def exact_inputs_give_exact_bits(c, batch):
    ids, noms = [0, 2, 2, 1, 0], [0, 1, 1, 0, 1]
    x_nom, u_nom = nominals(c, [0, 2], seed=51)
    rng = np.random.default_rng(52)
    K = np.zeros((2, T, c.nu, c.ndx)); k = np.zeros((2, T, c.nu))
    hinge = np.r_[np.arange(6, c.nv), c.nv + np.arange(c.nv), 2*c.nv + np.arange(c.na)]    # plain subtractions: everything but the free joint's dq
    for m in range(2):
        for t in range(T):
            for i in range(c.nu):
                if (i + m + t) % 2:
                    K[m, t, i, rng.choice(hinge)] = rng.choice([-1.0, 1.0])*2.0**rng.integers(-3, 3)
                else:
                    k[m, t, i] = 0.05*(c.hi[i] - c.lo[i])*rng.normal()
    alpha = np.array([1.0, 0.5, 2.0, 0.25, 4.0])
    res = run(c, batch, x_nom, u_nom, K, k, alpha, nom_ids=noms, env_ids=ids, n_substeps=1)
    u, x = c.np_(res.ctrl), c.np_(res.state)
    for r in range(5):
        for t in range(T):
            xs = c.x0[ids[r]] if t == 0 else x[r, t - 1]
            xn = x_nom[noms[r], t]
            # plain differences of the raw coordinates: hinge dof d has qpos address d + 1 behind the free joint's 7
            dx = np.r_[np.zeros(6), xs[7:c.nq] - xn[7:c.nq], xs[c.nq:] - xn[c.nq:]]
            s = np.array([sum(K[noms[r], t, i, j]*dx[j] for j in np.flatnonzero(K[noms[r], t, i])) for i in range(c.nu)])
            v = u_nom[noms[r], t] + (alpha[r]*k[noms[r], t] + s)
            ref = np.where(c.limited, np.clip(v, c.lo, c.hi), v)
            assert np.array_equal(u[r, t], ref), (r, t, np.abs(u[r, t] - ref).max())
    assert not np.array_equal(u[1], u[2])


# ------------------------------------------------------------------ 5
def time_and_nominal_indexing(c, batch, tag):
    ids, noms = [0, 2, 2, 1, 0], [0, 1, 1, 0, 1]
    x_nom, u_nom = nominals(c, [0, 2], seed=61)
    K, k = dense_gains(c, 2, seed=62, scale=0.3)
    assert all(not np.array_equal(a[m, s], a[n, t]) for a in (x_nom, u_nom, K) for m in range(2) for n in range(2) for s in range(T) for t in range(T)
               if (m, s) < (n, t))
    alpha = np.array([1.0, 0.5, 0.5, 1.0, 1.0])
    res = run(c, batch, x_nom, u_nom, K, k, alpha, nom_ids=noms, env_ids=ids, n_substeps=2, sensors=True)
    x, u = c.np_(res.state), c.np_(res.ctrl)
    assert np.array_equal(x[1], x[2]) and np.array_equal(u[1], u[2])            # same source, nominal and alpha
    assert not np.array_equal(u[0, 0], u[4, 0]) and not np.array_equal(x[0], x[4])          # same source, another nominal
    alpha2 = alpha.copy(); alpha2[2] = 0.25
    other = c.np_(run(c, batch, x_nom, u_nom, K, k, alpha2, nom_ids=noms, env_ids=ids, n_substeps=2).ctrl)
    assert not np.array_equal(other[2, 0], u[2, 0]) and np.array_equal(other[[0, 1, 3, 4]], u[[0, 1, 3, 4]])     # another alpha
    ref = formula(c, x, ids, noms, x_nom, u_nom, K, k, alpha)
    err = max(rel_err(u[r, t], ref[r, t]) for r in range(5) for t in range(T))
    print(f'{tag}: indexing: inputs against the formula in numpy {err:.1e}  bound {PARITY:.0e}')
    assert err <= PARITY, err


# ------------------------------------------------------------------ 6
def quaternion_columns_are_live(c, batch, tag):
    from flybody_amd import derivatives, lqr
    delta = np.array([0.3, -0.2, 0.45])                 # the rotation vector x_nom (-) x_0 of the root: x_0 (-) x_nom is -delta
    x_nom = np.repeat(c.x0[[1, 2]][:, None], T, axis=1)                          # (frame 1: the strongly rotated root in the air; 2: in contact)
    dq = np.zeros(c.nv); dq[3:6] = delta
    for m, e in enumerate((1, 2)):
        x_nom[m, 0, :c.nq] = derivatives.integrate_pos(c.shim, c.x0[e, :c.nq], dq)
    assert np.abs(lqr.state_difference(c.shim, c.x0[[1, 2]], x_nom[:, 0])[:, 3:6] + delta).max() < 1e-14
    assert np.abs(np.delete(lqr.state_difference(c.shim, c.x0[[1, 2]], x_nom[:, 0]), [3, 4, 5], axis=1)).max() == 0
    _, u_nom = nominals(c, [1, 2], seed=71)
    K = np.zeros((2, T, c.nu, c.ndx))
    w = c.hi - c.lo
    for i, (col, g) in enumerate(((3, 0.5), (4, -0.25), (5, 0.125), (4, 1.0))):
        K[:, :, i, col] = g*2.0**np.floor(np.log2(w[i]))                          # a power of two near the actuator's range
    res = run(c, batch, x_nom, u_nom, K, env_ids=[1, 2], n_substeps=1)
    u = c.np_(res.ctrl)
    ref = formula(c, c.np_(res.state), [1, 2], [0, 1], x_nom, u_nom, K, None, None)
    moved = np.abs(u[:, 0, :4] - u_nom[:, 0, :4])
    assert (moved > 0.02*w[:4]).all() and np.array_equal(u[:, 0, 4:], u_nom[:, 0, 4:]), moved
    err = max(rel_err(u[r, t], ref[r, t]) for r in range(2) for t in range(T))
    e4 = rel_err(u[:, 0, :4] - u_nom[:, 0, :4], ref[:, 0, :4] - u_nom[:, 0, :4])
    print(f'{tag}: quaternion columns: inputs against the formula {err:.1e}, the feedback term alone {e4:.1e}  bound {PARITY:.0e}')
    assert err <= PARITY and e4 <= PARITY, (err, e4)


# ------------------------------------------------------------------ 7
def rows_and_calls(c, batch):
    ids, noms = [0, 2, 2, 1, 0, 3, 3], [0, 1, 1, 0, 1, 1, 0]
    x_nom, u_nom = nominals(c, [0, 2], seed=81)
    K, k = dense_gains(c, 2, seed=82, scale=0.3)
    kw = dict(nom_ids=noms, env_ids=ids, n_substeps=2)
    full = run(c, batch, x_nom, u_nom, K, k, sensors=True, **kw)
    assert batch.rollouts_run() == 7 and c.np_(full.status).tolist() == [0]*7
    for pool in (1, 3, 0, 0):
        other = run(c, batch, x_nom, u_nom, K, k, sensors=True, pool_rows=pool, **kw)
        assert batch.rollouts_run() == 7
        same_physics(c, other, full)
        assert np.array_equal(c.np_(other.ctrl), c.np_(full.ctrl)), pool
    bare = run(c, batch, x_nom, u_nom, K, k, **kw)
    assert bare.sensordata is None and np.array_equal(c.np_(bare.state), c.np_(full.state)) and np.array_equal(c.np_(bare.ctrl), c.np_(full.ctrl))


# ------------------------------------------------------------------ 8
def sources_are_untouched(c):
    from test_rollout_emulation import ctrl_rows, twin_ctrl_loop
    batch, twin = c.make_batch(), c.make_batch()
    x_nom, u_nom = nominals(c, [0, 1, 2, 3], seed=91)
    K, k = dense_gains(c, 4, seed=92, scale=0.3)
    before = {f: batch.get(f) for f in STATE_FIELDS + ('CTRL', 'WARN')}
    res = run(c, batch, x_nom, u_nom, K, k, n_substeps=2, sensors=True)
    assert batch.rollouts_run() == 4 and np.isfinite(c.np_(res.state)).all()
    for f, x in before.items():
        assert np.array_equal(x, batch.get(f)), f
    ctrl = ctrl_rows(c.a, 4, 3, seed=93)
    mine = twin_ctrl_loop(batch, ctrl, 2, fields=STATE_FIELDS, sync=c.sync)
    rec = twin_ctrl_loop(twin, ctrl, 2, fields=STATE_FIELDS, sync=c.sync)
    for t in range(3):
        for f in STATE_FIELDS:
            assert np.array_equal(mine[t][f], rec[t][f]), (t, f)


# ------------------------------------------------------------------ 9 (the device only: tests/test_gpu_rollout_feedback.py)
def first_order_case(c, model, set_frames):
    """Environment 0 is the nominal state (the fly in the air), environments 1 .. 4 are it plus a tangent step of 1e-4 on a hinge angle, a
    hinge velocity, a root rotation and an activation.  Returns the batch, the steps delta [4, ndx], A, B of one substep at the nominal,
    and gains K whose columns at the four coordinates make |B K delta| comparable to |A delta| (the other columns multiply zeros)."""
    from flybody_amd import derivatives, engine
    q, v, act, ctrl = c.frames[0]
    cols = [20, c.nv + 35, 4, 2*c.nv + 11]
    delta = np.zeros((4, c.ndx)); delta[np.arange(4), cols] = 1e-4
    frames = [(q, v, act, ctrl)] + [(derivatives.integrate_pos(c.shim, q, d[:c.nv]), v + d[c.nv:2*c.nv], act + d[2*c.nv:], ctrl) for d in delta]
    batch = engine.Batch(model, 5, precision=64)
    set_frames(batch, frames)
    fd = batch.transition_fd(env_ids=[0], n_substeps=1)
    A, B = c.np_(fd.A)[0], c.np_(fd.B)[0]
    assert c.np_(fd.status).tolist() == [0]
    rng = np.random.default_rng(7)
    K = 1e-3*rng.normal(size=(c.nu, c.ndx))
    for i, j in enumerate(cols):
        col = rng.normal(size=c.nu)*(c.hi - c.lo)
        K[:, j] = col*np.abs(A @ delta[i]).max()/np.abs(B @ col*1e-4).max()
    return batch, np.r_[q, v, act], ctrl, delta, A, B, K


def first_order_consistency_with_transition_fd(c, model, set_frames, tag):
    """state' (-) x_nom' against (A + B K) delta.  The tolerance is measured in the same run on code this kernel does not touch: the same
    residual of the OPEN-LOOP kernel against A delta (K = 0), times ten -- the feedback term adds second-order terms of the same size."""
    from flybody_amd import lqr
    batch, xbar, ubar, delta, A, B, K = first_order_case(c, model, set_frames)
    u_dev = np.abs(K @ delta.T).max(axis=1)
    assert (u_dev < 0.25*np.minimum(ubar - c.lo, c.hi - ubar)).all()            # precondition: no input saturates
    ratio = [np.abs(B @ K @ d).max()/np.abs(A @ d).max() for d in delta]
    assert all(0.5 <= r <= 2 for r in ratio), ratio                             # precondition: the feedback term is as large as the free one
    open_ = c.np_(batch.rollout(ctrl=c.dev(np.tile(ubar, (5, 1, 1))), n_substeps=1).state)[:, 0]
    base = [rel_err(lqr.state_difference(c.shim, open_[1 + i], open_[0]), A @ delta[i]) for i in range(4)]
    res = run(c, batch, xbar[None, None], ubar[None, None], K[None, None], nom_ids=[0]*5, n_substeps=1)
    assert c.np_(res.status).tolist() == [0]*5
    x = c.np_(res.state)[:, 0]
    assert np.allclose(x[0], open_[0], rtol=0, atol=1e-12)                      # the nominal itself: dx = 0 but for the root's quaternion against itself, which is rounding
    got = [rel_err(lqr.state_difference(c.shim, x[1 + i], x[0]), (A + B @ K) @ delta[i]) for i in range(4)]
    for i, name in enumerate(('hinge angle', 'hinge velocity', 'root rotation', 'activation')):
        print(f'{tag}: first order, {name}: K = 0 against A delta {base[i]:.1e}, closed loop against (A + B K) delta {got[i]:.1e}  '
              f'(|B K delta| / |A delta| = {ratio[i]:.2f})')
    assert all(g <= 10*b for g, b in zip(got, base)), (got, base)


# ------------------------------------------------------------------ 10
def refusals(c, model, lib_path=None):
    """Every refusal names its reason (include/flybody_engine.h)."""
    import ctypes as C
    import pytest
    from flybody_amd import engine
    B = engine.Batch(model, 2, precision=64)
    L = B.L
    nx, nu, ndx = c.nx, c.nu, c.ndx
    z = lambda *s: c.dev(np.zeros(s))
    X, U, out, uo = z(3, 2, nx), z(3, 2, nu), z(3, 2, nx), z(3, 2, nu)
    noms3 = np.zeros(3, np.int32)

    def fbk(n_nom=1, nom_ids=noms3, x=X, u=U):
        return engine._Feedback(n_nom, None if nom_ids is None else nom_ids.ctypes.data, None if x is None else x.data_ptr(),
                                None if u is None else u.data_ptr(), None, None, None)

    def cfg(n_roll=1, horizon=2, n_substeps=1, ids=None, pool=0):
        return engine._RolloutConfig(n_roll, horizon, n_substeps, None if ids is None else ids.ctypes.data, pool)

    def raw(b, cf, f, state=out):
        engine._check(L, L.fb_batch_rollout_feedback(b, None if cf is None else C.byref(cf), None if f is None else C.byref(f),
                                                     None if state is None else C.c_void_p(state.data_ptr()), None, C.c_void_p(uo.data_ptr()), None, None))
    raw(B.h, cfg(), fbk()); c.sync()                      # (the arguments the refusals below vary are accepted as they stand)
    for match, args in (('null batch', (None, cfg(), fbk())), ('null config', (B.h, None, fbk())), ('null feedback', (B.h, cfg(), None)),
                        ('x_nom is NULL', (B.h, cfg(), fbk(x=None))), ('u_nom is NULL', (B.h, cfg(), fbk(u=None))),
                        ('n_nom must be >= 1', (B.h, cfg(), fbk(n_nom=0))),
                        ('nom_ids is NULL and n_nom', (B.h, cfg(n_roll=2), fbk(n_nom=3, nom_ids=None))),
                        ('n_roll must be >= 1', (B.h, cfg(n_roll=0), fbk())), ('horizon must be >= 1', (B.h, cfg(horizon=0), fbk())),
                        ('n_substeps must be >= 0', (B.h, cfg(n_substeps=-1), fbk())),
                        ('environment id out of range', (B.h, cfg(n_roll=3), fbk()))):
        with pytest.raises(engine.EngineError, match='fb_batch_rollout_feedback: .*' + match):
            raw(*args)
    with pytest.raises(engine.EngineError, match='state output is NULL'):
        raw(B.h, cfg(), fbk(), state=None)
    for bad in ([0, 1], [-1, 0], [0, 3]):
        with pytest.raises(engine.EngineError, match='nominal id -?\\d+ out of range'):
            raw(B.h, cfg(n_roll=2), fbk(n_nom=1 if bad[1] == 1 else 3, nom_ids=np.array(bad, np.int32)))
    x2, u2 = z(2, 2, nx), z(2, 2, nu)
    for ids in ([2, 0], [0, -1]):
        with pytest.raises(engine.EngineError, match='environment id -?\\d+ out of range'):
            B.rollout_feedback(x2, u2, env_ids=ids)
    for pool in (-1, 1 << 20):
        with pytest.raises(engine.EngineError, match='pool_rows out of range'):
            B.rollout_feedback(x2, u2, pool_rows=pool)
    kw = {} if lib_path is None else dict(lib_path=lib_path)
    with pytest.raises(engine.EngineError, match='FP64 batch'):
        engine.Batch(model, 2, precision=32).rollout_feedback(x2, u2)
    a2 = dict(c.a); a2['body_mass'] = np.asarray(c.a['body_mass'])*1.1
    with pytest.raises(engine.EngineError, match='group of 2 models'):
        engine.Batch(engine.ModelGroup([c.a, a2], **kw), 2, precision=64).rollout_feedback(x2, u2)
    Bl = engine.Batch(model, 2, precision=64)
    Bl.set_control_law(bias=np.zeros(c.nv))
    with pytest.raises(engine.EngineError, match='knows no control law'):
        Bl.rollout_feedback(x2, u2)
    Bl.clear_control_law()
    Bf = engine.Batch(model, 2, precision=64)
    Bf.set('QFRC_APPLIED', np.zeros((2, c.nv)))
    with pytest.raises(engine.EngineError, match='knows no applied forces'):
        Bf.rollout_feedback(x2, u2)
    Bf.clear_forces()
    # the Python shim's own checks
    for bad in (dict(x_nom=x2.float()), dict(u_nom=u2[:, :, :nu - 1]), dict(K=z(2, 2, ndx, nu)), dict(k=z(2, 1, nu)), dict(alpha=z(3)),
                dict(nom_ids=[0], env_ids=[0, 1]), dict(x_nom=np.zeros((2, 2, nx)))):
        with pytest.raises(ValueError):
            B.rollout_feedback(**{**dict(x_nom=x2, u_nom=u2), **bad})
    # accepted: many rollouts of one nominal and one environment
    B.forward(); c.sync()
    r = B.rollout_feedback(z(1, 1, nx), z(1, 1, nu), nom_ids=[0, 0, 0], env_ids=[1, 1, 1], n_substeps=1)
    assert B.rollouts_run() == 3 and r.state.shape == (3, 1, nx) and r.ctrl.shape == (3, 1, nu)
