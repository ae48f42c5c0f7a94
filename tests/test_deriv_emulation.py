"""fb_batch_transition_fd (csrc/fb_deriv.hpp: MuJoCo's mjd_transitionFD for the engine's step, one (frame, column, side) ticket per wave)
through the kernel-source emulation build, against the finite-difference recipe run on the CPU oracle (tests/fd_reference.py), against
closed forms that do not go through the oracle, and its argument validation.  No GPU needed.

The error of a matrix is taken per column: max |engine - oracle| over the column's largest oracle entry; every column is compared, in
one of two classes.  The oracle's recipe is run twice, with eps and 2 eps:
  * a column the oracle RESOLVES -- its two estimates agree to 1 % of the column's largest entry, and that entry lies above the rounding
    floor of its own quotient -- enters the figures below and is held to TOL;
  * any other column holds, in the oracle itself, rounding noise or a kink (the sensors' derivatives with respect to the root's
    horizontal translation are structurally zero: entries of 4e-6 against an accelerometer reading of 880; the force sensors in contact
    carry the constraint solver's stopping tolerance of 1e-8, divided by 2 eps) and must agree with the oracle to ten times the
    oracle's own eps-vs-2 eps difference in that column plus the floor,
        floor = 64 ulp(largest nominal output of the matrix's rows) / divisor.

Measured on the emulation build (eps = 1e-6; gap = largest column error, beside it the oracle's own eps-vs-2 eps figure):
    walk_imitation, in the air,  centred: A 2.7e-9 (6.7e-9)   B 3.5e-10 (3.5e-10)  C 4.8e-4 (4.2e-4)   D 0
    walk_imitation, in contact,  centred: A 1.1e-7 (3.3e-8)   B 1.9e-9 (2.8e-9)    C 9.3e-3 (6.1e-3)   D 0     (nefc 14)
    walk_imitation, in the air,  forward: A 6.6e-9 (3.9e-7)   B 6.9e-10 (3.5e-10)  C 4.2e-4 (4.4e-4)   D 0
    walk_imitation, in contact,  forward: A 2.7e-7 (4.1e-5)   B 3.7e-9 (2.8e-9)    C 1.1e-2 (7.6e-3)   D 0
    flight_imitation (nefc 5):            A 5.0e-6 (5.4e-4)   B 9.0e-9 (1.3e-8)
    walk_on_ball (nefc 19):               A 5.0e-8 (3.9e-8)   B 8.2e-10 (3.5e-10)
    n_substeps = 2, in contact:           A 5.3e-6 (4.6e-6)   B 1.3e-7 (1.4e-7)         A_2 vs A(x1) A(x0): 7.8e-9 of max |A_2|
    closed forms: activation block 7.2e-11, d act'/d ctrl 4.5e-11, hinge rows 1.2e-10
D is exactly zero on both sides: after one substep no sensor has seen the control (ctrl enters act_dot only).
At eps = 1e-6 the oracle's own eps-vs-2 eps figure is evaluation noise over eps, not truncation, and the gap to the engine is noise of
the same kind: two implementations of one transition differ by ~1e-13 of the state in contact, which 2 eps turns into 5e-8.  The gap
is therefore of the size of the oracle's figure, not well below it.  What was done to tell it from a systematic difference (warm start,
neighbour list, stale caches):
  * with eps = 1e-4 the gap of flight_imitation's A falls from 5.0e-6 to 6.2e-8, a factor 80 of the ideal 100 (test_gap_is_rounding_noise);
  * on a walking frame in contact (nefc 14; the third frame of tests/test_gpu_deriv.py) it falls from 1.4e-5 to 4.0e-7, a factor 35, on
    this build, and from 2.3e-6 to 4.7e-7, a factor 5, on the MI355X -- where the oracle's own figure at eps = 1e-4 is 2.9e-3, truncation.
    The part that does not fall with 1 / eps is not the solver's stopping rule (opt_tolerance 1e-14 instead of 1e-8 changes no digit of
    the gap) and not noslip (with noslip off the gap is 5.6e-4 and 1.6e-5: the same factor 35); it is not explained further;
  * the warm start, the neighbour list and the caches are covered directly: pool_rows 1, 3 and the full pool and two calls give the same
    bits, and the closed forms below hold to 1e-10 without the oracle.
TOL is ten times the largest measured gap of each matrix."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, random_state

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fd_reference as fr  # noqa: E402

TOL = dict(A=5.4e-5, B=1.4e-6, C=1.2e-1, D=0.0)            # 10 x the largest measured column error of each matrix (module comment)
TOL_CLOSED = 1e-9                                           # activation block and d act'/d ctrl against their closed forms
TOL_HINGE = 1e-8                                            # hinge rows: d q'/dx = [I 0 0] + h d v'/dx, absolute
TOL_CHAIN = 1.2e-7                                          # A_2 against A(x1) A(x0), relative to max |A_2|: 10 x the oracle's own 1.2e-8 in contact
ULPS = 64
RESOLVED = 1e-2                                             # a column is resolved when the oracle's two step sizes agree to 1 % of its largest entry


@pytest.fixture(scope='module')
def emu_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    return g.build_emu()


def _load(name, emu_lib):
    from flybody_amd import engine
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    a = dict(engine.load_npz(os.path.join(engine.ASSETS, name + '.npz')))
    return engine.Model(a, lib_path=emu_lib), fbo.OracleModel(pack_model(a)), a


def mid_ctrl(a, rng, lo=0.3, hi=0.7):
    r = np.asarray(a['actuator_ctrlrange'], float)
    return r[:, 0] + (r[:, 1] - r[:, 0])*rng.uniform(lo, hi, len(r))


def settle(om, a, q, v, ctrl, steps=300):
    """The oracle's state after `steps` substeps: (qpos, qvel, act)."""
    from oracle import fbo
    od = fbo.OracleData(om)
    od.field('qpos')[:] = q; od.field('qvel')[:] = v; od.field('ctrl')[:] = ctrl
    od.call('step1')
    for _ in range(steps):
        od.call('step')
    na = int((np.asarray(a['actuator_actadr']) >= 0).sum())
    return od.field('qpos').copy(), od.field('qvel').copy(), (od.field('act')[:na].copy() if na else np.zeros(0))


def set_frames(batch, frames):
    """frames: [(qpos, qvel, act, ctrl)] -> the batch's environments, then forward() (which defines the warm start w)."""
    batch.set('QPOS', np.array([f[0] for f in frames])); batch.set('QVEL', np.array([f[1] for f in frames]))
    batch.set('CTRL', np.array([f[3] for f in frames]))
    if batch.model.dim('na'):
        batch.set('ACT', np.array([f[2] for f in frames]))
    batch.forward()


def floors(F, eps, centered, n=1):
    """Rounding floor of the quotients of (x' rows, sensor rows): ULPS ulps of the largest nominal output over the divisor."""
    nom = F.nominal(n)
    h = 2*eps if centered else eps
    fx = ULPS*np.spacing(max(np.abs(np.r_[nom[0], nom[1], nom[2]]).max(), 1e-300))/h
    fs = ULPS*np.spacing(max(np.abs(nom[3]).max(), 1e-300))/h
    return dict(A=fx, B=fx, C=fs, D=fs)


def compare(got, ref, ref2, floor):
    """(gap, sensitivity): the largest column error of `got` against the oracle's `ref`, and of the oracle's own second estimate `ref2`
    (step 2 eps) against it, over the columns the oracle resolves.  The other columns must agree to the oracle's own uncertainty.
    Every column is in one of the two classes."""
    got, ref, ref2 = np.asarray(got), np.asarray(ref), np.asarray(ref2)
    assert got.shape == ref.shape and np.isfinite(got).all()
    scale = np.abs(ref).max(axis=0); unc = np.abs(ref2 - ref).max(axis=0); err = np.abs(got - ref).max(axis=0)
    resolved = (scale > floor) & (unc <= RESOLVED*scale)
    bad = ~resolved & (err > 10*unc + floor)
    assert not bad.any(), ('columns the oracle does not resolve differ by more than its own uncertainty', np.nonzero(bad)[0], err[bad], unc[bad])
    if not resolved.any():
        return 0.0, 0.0
    return float((err[resolved]/scale[resolved]).max()), float((unc[resolved]/scale[resolved]).max())


def check_frame(tag, res, k, F, eps, centered, n=1, names='ABCD'):
    """Matrices of frame k of an engine result against the oracle recipe; the recipe's own eps-vs-2 eps sensitivity is printed beside."""
    ref = dict(zip('ABCD', F.matrices(eps, centered, n)))
    ref2 = dict(zip('ABCD', F.matrices(2*eps, centered, n)))
    assert len(set(F.nefc)) == 1, ('precondition: a perturbed transition changed nefc', sorted(set(F.nefc)))
    fl = floors(F, eps, centered, n)
    for m in names:
        gap, sens = compare(getattr(res, m)[k].numpy(), ref[m], ref2[m], fl[m])
        print(f'{tag} {m}: gap {gap:.2e}  oracle eps vs 2 eps {sens:.2e}  bound {TOL[m]:.1e}  nefc {F.nefc[0]}')
        assert gap <= TOL[m], (tag, m, gap)


# ------------------------------------------------------------------ walk_imitation: two frames, shared by the tests below
@pytest.fixture(scope='module')
def walk(emu_lib):
    from flybody_amd import engine
    model, om, a = _load('walk_imitation', emu_lib)
    rng = np.random.default_rng(11)
    q, v = random_state(a, np.random.default_rng(0), spread=0.0, z=2.0)
    air = (q, v, rng.uniform(-0.1, 0.1, 59), mid_ctrl(a, rng))
    q, v = random_state(a, np.random.default_rng(3), spread=0.05, z=0.13, vel=0.0)
    ctrl = mid_ctrl(a, rng, 0.45, 0.55)
    floor_ = settle(om, a, q, v, ctrl) + (ctrl,)
    batch = engine.Batch(model, 2, precision=64)
    set_frames(batch, [air, floor_])
    F = [fr.Frame(om, a, *air), fr.Frame(om, a, *floor_)]
    return dict(model=model, om=om, a=a, batch=batch, frames=[air, floor_], F=F)


@pytest.fixture(scope='module')
def walk_centred(walk):
    res = walk['batch'].transition_fd(sensors=True)
    return res, walk['batch'].fd_tickets()


def test_walk_centred_matches_the_oracle_recipe(walk, walk_centred):
    res, tickets = walk_centred
    assert tickets == 2*(1 + 2*(275 + 59)) and res.status.tolist() == [0, 0]
    assert walk['F'][1].nominal() and walk['F'][1].nefc[-1] > 0            # the second frame stands on the floor
    for k, tag in enumerate(('air', 'contact')):
        check_frame('walk centred ' + tag, res, k, walk['F'][k], 1e-6, True)


def test_walk_forward_matches_the_oracle_recipe(walk):
    res = walk['batch'].transition_fd(sensors=True, centered=False)
    assert walk['batch'].fd_tickets() == 2*(1 + 275 + 59)
    for k, tag in enumerate(('air', 'contact')):
        check_frame('walk forward ' + tag, res, k, walk['F'][k], 1e-6, False)


def _other_task_state(model, a):
    """A frame (qpos, qvel, act, ctrl) of any task: joints off their defaults and inside their ranges, a rotated root / ball, in the air."""
    rng = np.random.default_rng(5)
    nq, nv = len(a['qpos0']), len(a['dof_bodyid'])
    q = np.array(a['qpos0'], float); v = rng.normal(size=nv)*0.5
    hinge = [j for j in range(len(a['jnt_type'])) if a['jnt_type'][j] == 3]
    qa = np.asarray(a['jnt_qposadr'])[hinge]
    q[qa] += rng.uniform(-0.05, 0.05, len(qa))
    lim = [j for j in hinge if a['jnt_limited'][j]]
    lo, hi = np.asarray(a['jnt_range'])[lim].T
    ql = np.asarray(a['jnt_qposadr'])[lim]
    q[ql] = np.clip(q[ql], lo + 0.05*(hi - lo), hi - 0.05*(hi - lo))          # (flight's qpos0 sits on wing limits)
    for j, t in enumerate(a['jnt_type']):                                      # rotated root / ball
        adr = int(a['jnt_qposadr'][j])
        if t == 0:
            q[adr + 2] = 2.0; quat = np.array([1.0, 0, 0, 0]) + rng.uniform(-0.3, 0.3, 4); q[adr + 3:adr + 7] = quat/np.linalg.norm(quat)
        elif t == 1:
            quat = np.array([1.0, 0, 0, 0]) + rng.uniform(-0.3, 0.3, 4); q[adr:adr + 4] = quat/np.linalg.norm(quat)
    na = model.dim('na')
    assert len(q) == nq
    return (q, v, rng.uniform(-0.1, 0.1, na), mid_ctrl(a, rng))


def _other_task_frame(name, emu_lib):
    from flybody_amd import engine
    model, om, a = _load(name, emu_lib)
    frame = _other_task_state(model, a)
    batch = engine.Batch(model, 1, precision=64)
    set_frames(batch, [frame])
    return model, om, a, batch, frame


@pytest.mark.parametrize('name', ['flight_imitation', 'walk_on_ball'])
def test_other_tasks_match_the_oracle_recipe(emu_lib, name):
    """flight_imitation: na = 0, ellipsoid fluid forces; walk_on_ball: a ball joint and no free joint."""
    model, om, a, batch, frame = _other_task_frame(name, emu_lib)
    assert (name == 'flight_imitation') == (model.dim('na') == 0) and (name == 'walk_on_ball') == (1 in list(a['jnt_type']))
    res = batch.transition_fd()
    assert res.C is None and res.D is None and res.status.tolist() == [0]
    check_frame(name, res, 0, fr.Frame(om, a, *frame), 1e-6, True, names='AB')


def test_gap_is_rounding_noise(emu_lib):
    """The gap to the oracle falls with 1 / eps: it is the rounding of the two transitions over the divisor, nothing systematic."""
    model, om, a, batch, frame = _other_task_frame('flight_imitation', emu_lib)
    F = fr.Frame(om, a, *frame)
    gaps = []
    for eps in (1e-6, 1e-4):
        res = batch.transition_fd(eps=eps)
        ref, ref2 = F.matrices(eps), F.matrices(2*eps)
        gaps.append(compare(res.A[0].numpy(), ref[0], ref2[0], floors(F, eps, True)['A'])[0])
    print('flight A gap at eps 1e-6, 1e-4:', gaps)
    assert gaps[1] < 0.05*gaps[0]


# ------------------------------------------------------------------ closed forms (no oracle)
def test_activation_block_and_hinge_rows_have_their_closed_forms(walk, walk_centred):
    res, _ = walk_centred
    a = walk['a']
    nv, na = 108, 59
    h = float(a['opt_timestep'])
    tau = np.asarray(a['actuator_dynprm'], float)[np.argsort(np.asarray(a['actuator_actadr']))]      # (by activation address)
    assert set(np.asarray(a['actuator_dyntype']).tolist()) == {2} and np.array_equal(np.asarray(a['actuator_actadr']), np.arange(59))
    hinge = [int(a['jnt_dofadr'][j]) for j in range(len(a['jnt_type'])) if a['jnt_type'][j] == 3]
    for k in range(2):
        A, B = res.A[k].numpy(), res.B[k].numpy()
        e1 = np.abs(A[2*nv:, 2*nv:] - np.diag(1 - h/tau)).max(); e2 = np.abs(A[2*nv:, :2*nv]).max()
        e3 = np.abs(B[2*nv:] - np.diag(h/tau)).max()
        e4 = max(np.abs(A[r] - np.eye(2*nv + na)[r] - h*A[nv + r]).max() for r in hinge)
        e5 = max(np.abs(B[r] - h*B[nv + r]).max() for r in hinge)
        print(f'frame {k}: act block {e1:.1e} {e2:.1e}, d act/d ctrl {e3:.1e}, hinge rows {e4:.1e} {e5:.1e}')
        assert e1 < TOL_CLOSED and e2 < TOL_CLOSED and e3 < TOL_CLOSED
        assert e4 < TOL_HINGE and e5 < TOL_HINGE


# ------------------------------------------------------------------ two substeps
def test_two_substeps_match_the_recipe_and_the_chain_rule(walk):
    from flybody_amd import engine
    a, om = walk['a'], walk['om']
    x0 = walk['frames'][1]
    F0 = walk['F'][1]
    q1, v1, act1, _ = F0.nominal()
    x1 = (q1, v1, act1, x0[3])
    batch = engine.Batch(walk['model'], 2, precision=64)
    set_frames(batch, [x0, x1])
    two = batch.transition_fd(env_ids=[0], n_substeps=2)
    check_frame('walk 2 substeps contact', two, 0, F0, 1e-6, True, n=2, names='AB')
    one = batch.transition_fd(want_B=False)
    A2 = two.A[0].numpy()
    prod = one.A[1].numpy() @ one.A[0].numpy()
    e = np.abs(A2 - prod).max()/np.abs(A2).max()
    print(f'A_2 vs A(x1) A(x0): {e:.2e} of max |A_2| (bound {TOL_CHAIN:.1e})')
    assert e < TOL_CHAIN


# ------------------------------------------------------------------ ctrl at a range limit
def test_ctrl_at_a_range_limit_gives_one_sided_columns(walk):
    from flybody_amd import engine
    a, om = walk['a'], walk['om']
    q, v, act, ctrl = walk['frames'][1]
    ctrl = ctrl.copy()
    r = np.asarray(a['actuator_ctrlrange'], float)
    assert np.asarray(a['actuator_ctrllimited'])[[4, 9, 17]].all()
    ctrl[4] = r[4, 1]; ctrl[9] = r[9, 0]; ctrl[17] = r[17, 1] - 0.5e-6             # upper bound, lower bound, closer than eps to the upper
    batch = engine.Batch(walk['model'], 1, precision=64)
    set_frames(batch, [(q, v, act, ctrl)])
    F = fr.Frame(om, a, q, v, act, ctrl)
    assert [F.ctrl_sides(i, 1e-6) for i in (4, 9, 17, 5)] == [(False, True), (True, False), (False, True), (True, True)]
    for centered in (True, False):
        res = batch.transition_fd(want_A=False, centered=centered)
        # centred: three columns lose a side; forward: the two columns at / near the upper bound nudge backwards
        assert batch.fd_tickets() == (1 + 2*59 - 3 if centered else 1 + 59)
        ref = F.matrices(1e-6, centered, cols=range(275, 275 + 59))[1]
        ref2 = F.matrices(2e-6, centered, cols=range(275, 275 + 59))[1]
        gap = compare(res.B[0].numpy(), ref, ref2, floors(F, 1e-6, centered)['B'])[0]
        print(f'ctrl at limits, centred {centered}: B gap {gap:.2e}')
        assert gap <= TOL['B']
        assert (np.abs(res.B[0].numpy()[:, [4, 9, 17]]).max(axis=0) > 0.01).all()          # h / tau = 0.02: not the zero column of a clamped nudge
    # neither side fits (a control outside its range): the column is zero
    ctrl[4] = r[4, 1] + 0.1
    set_frames(batch, [(q, v, act, ctrl)])
    res = batch.transition_fd(want_A=False)
    assert not res.B[0].numpy()[:, 4].any() and res.B[0].numpy()[:, 5].any()


# ------------------------------------------------------------------ row reuse, determinism
def test_results_do_not_depend_on_the_pool_or_the_call(emu_lib, walk):
    model, om, a, batch, frame = _other_task_frame('walk_on_ball', emu_lib)
    from flybody_amd import engine
    b2 = engine.Batch(model, 2, precision=64)
    f2 = (frame[0], frame[1]*0.5, frame[2], frame[3])
    set_frames(b2, [frame, f2])
    full = b2.transition_fd(sensors=True)
    small = b2.transition_fd(sensors=True, pool_rows=3)
    again = b2.transition_fd(sensors=True)
    one = b2.transition_fd(sensors=True, pool_rows=1)
    for m in 'ABCD':
        x = getattr(full, m).numpy()
        assert m == 'D' or not np.array_equal(x[0], x[1])          # (D = 0: after one substep no sensor has seen the control yet)
        for other in (small, again, one):
            assert np.array_equal(x, getattr(other, m).numpy()), m
    # walk_imitation in contact, the control columns
    wb = walk['batch']
    x = wb.transition_fd(want_A=False, sensors=True)
    y = wb.transition_fd(want_A=False, sensors=True, pool_rows=3)
    assert np.array_equal(x.B.numpy(), y.B.numpy()) and np.array_equal(x.D.numpy(), y.D.numpy())


# ------------------------------------------------------------------ non-disturbance
def test_linearising_between_steps_leaves_the_environments_alone(emu_lib, reference_traj):
    from flybody_amd import engine
    model, _, a = _load('walk_imitation', emu_lib)
    qp, qv = reference_traj
    rng = np.random.default_rng(2)
    acts = [rng.uniform(-0.5, 0.5, (8, 59)).astype(np.float32) for _ in range(3)]
    fields = ('QPOS', 'QVEL', 'ACT', 'QACC', 'OBS', 'WARN', 'SIZE_STATS', 'STEP_TICKS')

    def run(linearise):
        b = engine.Batch(model, 8, precision=64)
        b.set_reference(qp, qv, terminal_com_dist=float('inf'))
        b.reset()
        out = []
        for k, act in enumerate(acts):
            b.step_ptr(act.ctypes.data)
            if linearise and k == 0:
                before = {f: b.get(f) for f in fields}
                r = b.transition_fd(env_ids=[1, 6, 3], want_A=False, sensors=True)
                assert np.isfinite(r.B.numpy()).all() and r.B.numpy().any()
                for f in fields:
                    assert np.array_equal(before[f], b.get(f)), f
            out.append({f: b.get(f) for f in fields})
        return out
    plain, lin = run(False), run(True)
    for k in range(len(acts)):
        for f in fields:
            assert np.array_equal(plain[k][f], lin[k][f]), (k, f)


# ------------------------------------------------------------------ validation
def test_argument_validation(emu_lib, walk):
    import ctypes as C
    from flybody_amd import engine
    model, a = walk['model'], walk['a']
    B = engine.Batch(model, 2, precision=64)
    L = B.L
    out = np.zeros(275*275*2)

    def raw(b, cfg, A=out.ctypes.data):
        engine._check(L, L.fb_batch_transition_fd(b, None if cfg is None else C.byref(cfg), A, None, None, None, None, None))

    def cfg(eps=1e-6, centered=1, n_substeps=1, n_frames=1, ids=None, pool=0):
        return engine._FDConfig(eps, centered, n_substeps, n_frames, None if ids is None else ids.ctypes.data, pool)
    with pytest.raises(engine.EngineError, match='null batch'):
        raw(None, cfg())
    with pytest.raises(engine.EngineError, match='null config'):
        raw(B.h, None)
    with pytest.raises(engine.EngineError, match='all four outputs are NULL'):
        raw(B.h, cfg(), None)
    with pytest.raises(engine.EngineError, match='all four outputs are NULL'):
        B.transition_fd(want_A=False, want_B=False)
    for bad in (0.0, -1e-6, float('nan'), float('inf')):
        with pytest.raises(engine.EngineError, match='eps must be finite and > 0'):
            B.transition_fd(eps=bad)
    with pytest.raises(engine.EngineError, match='n_substeps must be >= 1'):
        B.transition_fd(n_substeps=0)
    with pytest.raises(engine.EngineError, match='n_frames must be >= 1'):
        raw(B.h, cfg(n_frames=0))
    with pytest.raises(engine.EngineError, match='centered must be 0 or 1'):
        raw(B.h, cfg(centered=2))
    for ids in ([2], [-1], [0, 5]):
        with pytest.raises(engine.EngineError, match='environment id -?\\d+ out of range'):
            B.transition_fd(env_ids=ids)
    with pytest.raises(engine.EngineError, match='environment id out of range'):
        raw(B.h, cfg(n_frames=3))
    for pool in (-1, 9, 1 << 20):
        with pytest.raises(engine.EngineError, match='pool_rows out of range'):
            B.transition_fd(pool_rows=pool)
    with pytest.raises(engine.EngineError, match='FP64 batch'):
        engine.Batch(model, 2, precision=32).transition_fd()
    a2 = dict(a); a2['body_mass'] = np.asarray(a['body_mass'])*1.1
    with pytest.raises(engine.EngineError, match='group of 2 models'):
        engine.Batch(engine.ModelGroup([a, a2], lib_path=emu_lib), 2, precision=64).transition_fd()
    Bl = engine.Batch(model, 2, precision=64)
    Bl.set_control_law(bias=np.zeros(108))
    with pytest.raises(engine.EngineError, match='knows no control law'):
        Bl.transition_fd()
    Bl.clear_control_law()
    Bf = engine.Batch(model, 2, precision=64)
    Bf.set('QFRC_APPLIED', np.zeros((2, 108)))
    with pytest.raises(engine.EngineError, match='knows no applied forces'):
        Bf.transition_fd()
    Bf.clear_forces()
    # NULL A with B given: only the nu control columns run (and the nominal); NULL B: only the state columns
    set_frames(Bf, walk['frames'])
    r = Bf.transition_fd(want_A=False, env_ids=[0])
    assert r.A is None and r.B.shape == (1, 275, 59) and Bf.fd_tickets() == 1 + 2*59
    r = Bf.transition_fd(want_A=False, env_ids=[0], centered=False)
    assert Bf.fd_tickets() == 1 + 59
    fl = engine.Model.from_asset('flight_imitation', lib_path=emu_lib)
    Bq = engine.Batch(fl, 1, precision=64)
    Bq.forward()
    r = Bq.transition_fd(want_B=False, centered=False)
    assert r.B is None and r.A.shape == (1, 84, 84) and Bq.fd_tickets() == 1 + 84


# ------------------------------------------------------------------ Python surface
def test_python_surface(emu_lib):
    from flybody_amd import derivatives
    from flybody_amd.inverse_dynamics import differentiate_pos
    model, om, a, batch, frame = _other_task_frame('walk_on_ball', emu_lib)
    q, v, act, ctrl = frame
    res = derivatives.transition_fd(model, q, v, act, ctrl, sensors=True)
    ref = batch.transition_fd(sensors=True)
    for m in 'ABCD':
        assert np.array_equal(getattr(res, m), getattr(ref, m)[0].numpy()), m
    assert res.status == 0 and res.A.shape == (2*105 + 59, 2*105 + 59)
    many = derivatives.transition_fd(model, np.array([q, q]), np.array([v, 0.5*v]), np.array([act, act]), np.array([ctrl, ctrl]), batch_size=1)
    assert np.array_equal(many.A[0], res.A) and many.C is None and not np.array_equal(many.A[0], many.A[1]) and many.status.tolist() == [0, 0]
    with pytest.raises(ValueError):
        derivatives.transition_fd(model, q, v[:-1])
    for name in ('walk_imitation', 'flight_imitation', 'walk_on_ball'):
        m = _load(name, emu_lib)[0]
        names = derivatives.tangent_names(m)
        ndx, nu = 2*m.dim('nv') + m.dim('na'), m.dim('nu')
        assert len(names) == ndx + nu and len(set(names)) == len(names) and all(names)
        assert names[ndx].startswith('ctrl:') and names[m.dim('nv')].startswith('dv:') and names[0].startswith('dq:')
    # integrate_pos inverts differentiate_pos (free joint on walk_imitation, the ball joint here), and is the recipe's own integration
    rng = np.random.default_rng(1)
    for name in ('walk_imitation', 'walk_on_ball'):
        m, _, aa = _load(name, emu_lib)
        nv = m.dim('nv')
        q0 = _other_task_frame(name, emu_lib)[4][0]
        dq = rng.normal(size=nv)*0.3
        q1 = derivatives.integrate_pos(m, q0, dq)
        assert np.abs(differentiate_pos(m, q0, q1, 1.0) - dq).max() < 1e-13
        assert np.abs(q1 - fr.integrate_pos(aa, q0, dq)).max() < 1e-15
        both = derivatives.integrate_pos(m, np.array([q0, q0]), np.array([dq, -dq]))
        assert np.array_equal(both[0], q1) and np.abs(differentiate_pos(m, q0, both[1], 1.0) + dq).max() < 1e-13
