"""States, field table and assertions of tests/test_smooth_stages.py: the smooth stages of the step kernel (fb_smooth.hpp: d_kinematics,
d_com_pos, d_crb, d_com_vel, d_passive with the ellipsoid wing model, d_rne_bias, actuation, sensors) against the FP64 oracle, on every
model, in FP64 and in FP32.

THE STATES are chosen on the CPU with the oracle alone; each carries a property that test_smooth_stages.py::test_states_have_their_properties
asserts on the oracle's own evaluation, so a state that loses its property fails there instead of leaving another test green and empty.

  flight_imitation   roll0 ... roll4   oracle rollouts under U(-1, 1) actions, snapshots after 12 / 23 / 34 / 45 control steps of four environments
                                       and 29 of a fifth run, ctrl from the oracle: max|qvel| > 1e3 and max|qfrc_fluid| > 1 in at least
                                       three of the first four
                     still             the pose of roll0 at zero velocity: qfrc_fluid exactly 0 (the fmax(FB_MINV, .) guards divide 0 by
                                       the guard), QFRC_PASSIVE is springs only
                     +x -x +y -y +z -z the pose of roll0, root translating along one world axis at 50 cm/s, every other velocity zero: the
                                       sign of fabs(v) v in the box drag, projected areas with two components gone, cosa at its limits
  walk_imitation,    rand0 ... rand2   conftest.random_state / the tethered counterpart with non-zero CTRL and ACT
  walk_on_ball       adhesion          rand0 with the six adhesion actuators at 1 -- CTRL and ACT: these actuators are filtered
                                       (dyntype 2), a forward evaluation takes their force from ACT and only act_dot from CTRL;
                                       the oracle's qfrc_actuator differs from rand0's with both at 0 ("adhesion0")
  walk_on_ball       spin              rand1 with the ball's own dofs at (8, -6, 5) rad/s, |w| = 11.2: the second tree's CVEL is not small
  every model        quat*1.3, quat*1e-3   the free root's quaternion (walk_on_ball: the ball's, its fly is welded to the world) scaled:
                                       the stages normalise it
                     ctrl+5, ctrl-5    CTRL (and ACT where the model has activations) at +5 / -5 times the control range: some force-limited
                                       actuator sits at its force clamp
                     qvel*300
                     limits            the limited hinges 2 rad beyond their ranges, sign at random (LIMITS below: which), the abdomen left
                                       alone: one row per driven joint, 35 / 134 / 136 rows (the free models are lifted to z = 1 first)
                     folded            the same with the abdomen driven as well (FOLDED below), 86 / 155 / 150 rows: its contact list holds
                                       sphere-cylinder pairs whose MPR normal is discontinuous in the pose (EXCEPTIONS below)
                     far               the root at (50, -30, z): xpos - com cancels (walk_on_ball has no root position: no such state)
  and the first state once more as the last environment: equal to the bit in every field.  The environment counts (21, 14, 14) are no multiple
  of four, the environments a workgroup of the 12-per-CU build holds.

THE COMPARISON.  Relative differences max|x - y| / max|y| per field and environment (the project's _rel).  CVEL is compared as
[angular, velocity of the body's frame origin], the two halves on their own scales: the kernel expresses every body's spatial velocity
about ONE point, FB_SUBTREE_COM (the CoM of the whole model), the oracle and MuJoCo about subtree_com[body_rootid[b]] -- on walk_on_ball
(roots 1 and 68) the raw linear parts differ by tenths of their magnitude (2.4 relative on the spin state) while lin + ang x (xpos - ref)
agrees to 2e-15.
Where an oracle field is identically zero the kernel's must be zero too."""
import os

import numpy as np

from conftest import ROOT, random_state
from test_delassus_entry_lanes import _state
from test_solver_handover import TOL, _rel

ASSETS = os.path.join(ROOT, 'flybody_amd', 'assets')
TASKS = ('flight_imitation', 'walk_on_ball', 'walk_imitation')
VARIANTS = tuple(sorted(f[:-4] for f in os.listdir(os.path.join(ASSETS, 'variants')) if f.endswith('.npz')))

# fb_batch_get field -> oracle field
SMOOTH = (('XPOS', 'xpos'), ('XQUAT', 'xquat'), ('GEOM_XPOS', 'geom_xpos'), ('GEOM_XMAT', 'geom_xmat'), ('SITE_XPOS', 'site_xpos'),
          ('SUBTREE_COM', 'subtree_com'), ('CVEL', 'cvel'), ('QM', 'qM'), ('QFRC_BIAS', 'qfrc_bias'), ('QFRC_PASSIVE', 'qfrc_passive'),
          ('QFRC_ACTUATOR', 'qfrc_actuator'), ('QACC_SMOOTH', 'qacc_smooth'))
SOLVER = (('QACC', 'qacc'), ('QFRC_CONSTRAINT', 'qfrc_constraint'), ('EFC_FORCE', 'efc_force'), ('SENSORDATA', 'sensordata'))
EXTRA = ('qfrc_fluid', 'actuator_force', 'xmat')                   # oracle fields the property assertions read

# FP64: tests/test_gpu_parity.py's figures.  FP32, smooth fields: 64 units of single precision in the last place -- at most 10 bodies on the
# longest chain of these models times about 6 dependent roundings per link (joint quaternion, rotation, translation), linear growth;
# not taken from the code under test (the oracle moves by <= 2.3e-7 when the state is rounded to single precision).  FP32 QACC: TOL[32].
TOL_SMOOTH = {64: 1e-9, 32: 64*2.0**-24}
TOL_SOLVER = {64: 1e-6, 32: TOL[32]}
# The bounds that are not the common ones, each from the oracle's own spread under one-ulp perturbations (ulp_spread: no code under test in it):
# (model or None for every model, state, fields, precisions, bound as a function of (common bound, spread))
#   * 'far', FP32, smooth fields: 64 max(2^-24, spread) -- xpos - com and lin + ang x (xpos - com) cancel there;
#   * walk_on_ball 'qvel*300', FP32, QFRC_BIAS alone: the same rule -- the one smooth field that exceeded 64 x 2^-24 (1.2e-5, in emulation
#     already): its velocity products cancel, the oracle's own spread is 1.2e-5.  Every other field of 'qvel*300' keeps the common bound;
#   * 'folded', both precisions, the solver-dependent fields: max(common, 2 spread).  With the abdomen folded 2 rad beyond its ranges the
#     sphere of segment 7 sits 0.004 ... 0.04 deep in the cylinders of segments 2, 3 and 4, and the MPR normal of such a pair is not a
#     continuous function of the pose: in the ORACLE, 16 copies of the state with qpos / qvel moved by one unit of DOUBLE precision in the
#     last place return normals 4e-4 ... 1e-2 apart for exactly those pairs (every other contact: < 1e-9) and QACC 6e-4 ... 1.1e-2 apart.
#     A kernel whose FP64 roundings differ from the oracle's lands on either side: the emulation differs from the oracle by 2e-3 ... 1e-2 on
#     those normals on the walking models and by 2e-12 on flight_imitation, the MI355X by 2.0e-3 on the flight state -- the very figure by
#     which the oracle's own copies differ on that contact.  The smooth fields of 'folded' keep the common bounds.
_smooth_rule = lambda common, spread: 64*max(2.0**-24, spread)
EXCEPTIONS = ((None, 'far', tuple(f for f, _ in SMOOTH), (32,), _smooth_rule),
              ('walk_on_ball', 'qvel*300', ('QFRC_BIAS',), (32,), _smooth_rule),
              (None, 'folded', tuple(f for f, _ in SOLVER), (64, 32), lambda common, spread: max(common, 2*spread)))
# seeds of rand0 ... rand2.  walk_imitation skips 2: that state holds a capsule 5.4e-4 deep in a cylinder, and over 17 copies of it one
# single-precision ulp apart the FP32 kernel's MPR normal of that contact ranges over 0.15 (emulation and MI355X; the oracle's and the FP64
# kernel's over 6e-8), FP32 QACC 5e-4 ... 9.8e-2 from the oracle's -- the ill-conditioned FP32 portal refinement of tests/pgs_cases.py, in
# front of the solver and outside the stages this file is for (test_smooth_stages.py's docstring has the figures)
RAND_SEEDS = {'walk_on_ball': (0, 1, 2), 'walk_imitation': (0, 1, 3)}
# 'limits' and 'folded': (seed, share of the limited hinges that are driven).  'limits' leaves the abdomen in range, 'folded' drives it as
# well (EXCEPTIONS above).  walk_on_ball drives three quarters of the hinges: with all of them the legs fill the contact list (64 contacts,
# 192 rows).
LIMITS = {'flight_imitation': (7, 1.0), 'walk_imitation': (7, 1.0), 'walk_on_ball': (11, 0.75)}
FOLDED = {'flight_imitation': (7, 1.0), 'walk_imitation': (8, 1.0), 'walk_on_ball': (13, 0.75)}     # (walk_imitation with seed 7: 64 contacts, the cap)
SPREAD_PATTERNS = 16


def load(name):
    from flybody_amd.model_blob import load_npz
    return load_npz(os.path.join(ASSETS, name + '.npz') if name in TASKS else os.path.join(ASSETS, 'variants', name + '.npz'))


def task_of(name):
    return next(t for t in TASKS if name.startswith(t))


def _free_root(a):
    return int(a['jnt_type'][0]) == 0


def _quat_adr(a):
    """qpos address of the quaternion the 'quat*' states scale: the free root's, or the ball joint's"""
    return 3 if _free_root(a) else int(a['jnt_qposadr'][np.nonzero(a['jnt_type'] == 1)[0][0]])


def _adhesion(a):
    return np.nonzero(a['actuator_trntype'] == 5)[0]            # mjTRN_BODY


def _st(name, q, v, ctrl, act):
    return dict(name=name, q=np.array(q, float), v=np.array(v, float), ctrl=np.array(ctrl, float), act=np.array(act, float))


def flight_rollout_states(a, snapshots=(12, 23, 34, 45)):
    """Oracle rollouts set up as tests/test_gpu_parity.py::flight_rollout_vs_oracle: environment e is read after snapshots[e] control
    steps of its own U(-1, 1) actions"""
    from flybody_amd.mjcf_compile import qrot
    from flybody_amd.model_blob import pack_model
    from flybody_amd.reference import constant_speed_trajectory
    from flybody_amd.wbpg import build_tables
    from oracle import fbo
    om = fbo.OracleModel(pack_model(a))
    tabs = build_tables()
    cq, cv = constant_speed_trajectory(200, 20.0, init_pos=(0, 0, 1), body_rot_angle_y=-47.5, control_timestep=2e-4)
    root = cq.copy()
    for i in range(len(root)):
        root[i, :3] = cq[i, :3] + qrot(cq[i, 3:], -a['com_offset'])
    ods = []
    for e in range(len(snapshots)):
        od = fbo.OracleData(om); od.set_wbpg(tabs, seed=5); od.set_env_id(e)
        od.configure_env(root, cv, future_steps=5, terminal_com_dist=2.0, time_limit=0.6); od.env_reset(); ods.append(od)
    rng = np.random.default_rng(1)
    out = [None]*len(snapshots)
    for k in range(1, max(snapshots) + 1):
        fbo.step_batch(ods, rng.uniform(-1, 1, (len(ods), 12)))
        for e, s in enumerate(snapshots):
            if s == k: out[e] = _st('roll%d' % e, ods[e].field('qpos'), ods[e].field('qvel'), ods[e].field('ctrl'), np.zeros(0))
    return out


def states(a, name):
    """the states of one task model, in the order of the module docstring"""
    task = task_of(name)
    nu, na, nv = len(a['actuator_trntype']), int((a['actuator_actadr'] >= 0).sum()), len(a['dof_bodyid'])
    if task == 'flight_imitation':
        S = flight_rollout_states(a)
        S.append(dict(flight_rollout_states(a, snapshots=(29,))[0], name='roll4'))
        base = S[0]
        S.append(_st('still', base['q'], np.zeros(nv), base['ctrl'], base['act']))
        for k, ax in enumerate('xyz'):
            for sg in (+1, -1):
                v = np.zeros(nv); v[k] = 50.0*sg
                S.append(_st('+-'[sg < 0] + ax, base['q'], v, base['ctrl'], base['act']))
        fast = S[1]
    else:
        S = []
        for seed in RAND_SEEDS[task]:
            rng = np.random.default_rng(100 + seed)
            q, v = _state(a, True, 200 + seed, 0.2, False) if task == 'walk_on_ball' else random_state(a, rng)
            S.append(_st('rand%d' % len(S), q, 2.5*v if task == 'walk_on_ball' else v, rng.uniform(-0.3, 0.3, nu), rng.uniform(-0.2, 0.2, na)))
        base = S[0]
        for val in (1.0, 0.0):
            c, t = base['ctrl'].copy(), base['act'].copy()
            ad = _adhesion(a); c[ad] = val; t[a['actuator_actadr'][ad]] = val
            S.append(_st('adhesion' if val else 'adhesion0', base['q'], base['v'], c, t))
        if task == 'walk_on_ball':
            d = int(a['jnt_dofadr'][np.nonzero(a['jnt_type'] == 1)[0][0]])
            v = S[1]['v'].copy(); v[d:d + 3] = (8.0, -6.0, 5.0)
            S.append(_st('spin', S[1]['q'], v, S[1]['ctrl'], S[1]['act']))
        fast = S[1]
    qa = _quat_adr(a)
    for s in (1.3, 1e-3):
        q = base['q'].copy(); q[qa:qa + 4] *= s
        S.append(_st('quat*%g' % s, q, base['v'], base['ctrl'], base['act']))
    lo, hi = a['actuator_ctrlrange'][:, 0], a['actuator_ctrlrange'][:, 1]
    for sg in (+1, -1):
        c = 5.0*(hi if sg > 0 else lo)
        t = np.array([c[i] for i in range(nu) if a['actuator_actadr'][i] >= 0])
        S.append(_st('ctrl%+d' % (5*sg), base['q'], base['v'], c, t))
    S.append(_st('qvel*300', fast['q'], 300.0*fast['v'], fast['ctrl'], fast['act']))
    for tag, (seed, share) in (('limits', LIMITS[task]), ('folded', FOLDED[task])):
        q = base['q'].copy(); rng = np.random.default_rng(seed)
        for j in np.nonzero((a['jnt_type'] == 3) & (a['jnt_limited'] != 0))[0]:
            if tag == 'limits' and 'abdomen' in str(a['names_jnt'][j]): continue
            up, driven = rng.random(2) < (0.5, share)
            if driven: q[a['jnt_qposadr'][j]] = a['jnt_range'][j, 1] + 2.0 if up else a['jnt_range'][j, 0] - 2.0
        if _free_root(a): q[2] = 1.0
        S.append(_st(tag, q, base['v'], base['ctrl'], base['act']))
    if _free_root(a):
        q = base['q'].copy(); q[0], q[1] = 50.0, -30.0
        S.append(_st('far', q, base['v'], base['ctrl'], base['act']))
    S.append(dict(base, name=base['name'] + ' again'))
    return S


def variant_state(a, name):
    """one state of a variant blob, twice (the copy must come out equal to the bit): a flight rollout snapshot, or a random state with
    controls and activations"""
    task = task_of(name)
    if task == 'flight_imitation': S = flight_rollout_states(a, snapshots=(17,))
    else:
        rng = np.random.default_rng(11)
        q, v = _state(a, True, 211, 0.2, False) if task == 'walk_on_ball' else random_state(a, rng)
        S = [_st('rand', q, v, rng.uniform(-0.3, 0.3, len(a['actuator_trntype'])), rng.uniform(-0.2, 0.2, int((a['actuator_actadr'] >= 0).sum())))]
    return S + [dict(S[0], name=S[0]['name'] + ' again')]


def rounded(S, precision):
    """the states as the engine holds them: rounded to single precision for the FP32 build"""
    if precision == 64: return S
    r = lambda x: x.astype(np.float32).astype(float)
    return [dict(s, q=r(s['q']), v=r(s['v']), ctrl=r(s['ctrl']), act=r(s['act'])) for s in S]


def _evaluate(model, s):
    from oracle import fbo
    od = fbo.OracleData(model)
    od.field('qpos')[:] = s['q']; od.field('qvel')[:] = s['v']; od.field('ctrl')[:] = s['ctrl']
    if len(s['act']): od.field('act')[:] = s['act']
    od.call('forward')
    res = dict(s, nefc=int(od.scalar('nefc')), ncon=int(od.scalar('ncon')))
    for _, of in SMOOTH + SOLVER: res[of] = od.field(of).copy()
    for of in EXTRA: res[of] = od.field(of).copy()
    return res


def oracle_forward(a, S, precision):
    """FP64 oracle forward evaluations of the states (FP32: of the states rounded to single precision)"""
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    model = fbo.OracleModel(pack_model(a))
    return [_evaluate(model, s) for s in rounded(S, precision)]


def _origin_velocity(cvel, xpos, ref):
    """[angular, velocity of the body's frame origin] from spatial velocities about ref[b]: (ang, lin + ang x (xpos - ref))"""
    c = np.asarray(cvel, float).reshape(-1, 6); x = np.asarray(xpos, float).reshape(-1, 3)
    return c[:, :3], c[:, 3:] + np.cross(c[:, :3], x - ref)


def oracle_field(a, r, of):
    """an oracle field in the form it is compared in"""
    if of == 'subtree_com': return r[of][:3]
    if of == 'cvel': return _origin_velocity(r['cvel'], r['xpos'], r['subtree_com'].reshape(-1, 3)[a['body_rootid']])
    if of == 'efc_force': return r[of][:r['nefc']]
    return r[of]


def kernel_field(got, e, f, nefc):
    if f == 'CVEL': return _origin_velocity(got['CVEL'][e], got['XPOS'][e], got['SUBTREE_COM'][e][None, :])
    if f == 'EFC_FORCE': return got[f][e][:nefc]
    return got[f][e]


def forward(a, lib, ref, precision):
    """the kernel's forward evaluation of the states behind ref (an oracle_forward result): every compared field, [environment][...]"""
    from flybody_amd import engine
    M = engine.Model(a, lib_path=lib)
    B = engine.Batch(M, len(ref), precision=precision)
    B.set('QPOS', np.array([r['q'] for r in ref])); B.set('QVEL', np.array([r['v'] for r in ref])); B.set('CTRL', np.array([r['ctrl'] for r in ref]))
    if len(ref[0]['act']): B.set('ACT', np.array([r['act'] for r in ref]))
    B.forward(); B.synchronize()
    out = {f: B.get(f).copy() for f in ('NCON', 'NEFC', 'WARN_EVER') + tuple(f for f, _ in SMOOTH + SOLVER)}
    del B, M
    return out


def _difference(x, y):
    """(relative difference, the oracle's value is identically zero); CVEL: the larger of its two halves' differences"""
    if isinstance(y, tuple):
        d = [_difference(p, q) for p, q in zip(x, y)]
        return max(v for v, _ in d), all(z for _, z in d)
    if np.abs(y).max() == 0: return float(np.abs(x).max()), True
    return _rel(x, y), False


def ulp_spread(a, s, fields=SMOOTH, ulp=32, patterns=SPREAD_PATTERNS):
    """How far the ORACLE's fields range over `patterns` evaluations in which every input and every non-zero real model constant is moved
    by one unit in the last place, random signs -- of single precision (the state rounded to it first) or of double precision:
    {oracle field: widest range of an entry / largest magnitude of the field}.  The conditioning of a state, measured without the code
    under test."""
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    s = rounded([s], ulp)[0]
    base = _evaluate(fbo.OracleModel(pack_model(a)), s)
    rng = np.random.default_rng(5)
    dt = np.float32 if ulp == 32 else np.float64

    def nudge(x):
        x = np.asarray(x, dt)                    # (a zero stays zero: zeros switch model features off)
        return np.where(x == 0, x, np.nextafter(x, np.where(rng.random(x.shape) < 0.5, -np.inf, np.inf).astype(dt))).astype(float)

    def oracle_field(a, r, of):                  # (the rows of the unperturbed evaluation: equal lengths over the patterns)
        return r[of][:base['nefc']] if of == 'efc_force' else globals()['oracle_field'](a, r, of)
    halves = lambda x: x if isinstance(x, tuple) else (x,)
    seen = {of: [halves(oracle_field(a, base, of))] for _, of in fields}
    for _ in range(patterns):
        ap = {k: (nudge(v) if np.asarray(v).dtype.kind == 'f' and np.ndim(v) > 0 else v) for k, v in a.items()}
        r = _evaluate(fbo.OracleModel(pack_model(ap)), dict(s, q=nudge(s['q']), v=nudge(s['v']), ctrl=nudge(s['ctrl']), act=nudge(s['act'])))
        for _, of in fields: seen[of].append(halves(oracle_field(a, r, of)))
    # the spread of a field: the widest range any of its entries covers over the evaluations, relative to the field's largest magnitude
    spread = {}
    for _, of in fields:
        spread[of] = 0.0
        for h in range(len(seen[of][0])):
            x = np.array([np.ravel(v[h]) for v in seen[of]])
            if np.abs(x[0]).max() > 0: spread[of] = max(spread[of], float((x.max(0) - x.min(0)).max()/np.abs(x[0]).max()))
    return spread


def check_forward(a, name, got, ref, precision, tag, spread=None):
    """Every field of every environment of model `name` against the oracle; the figures are printed before they are asserted.  spread:
    spreads(...) of the model and precision.  Returns {field: worst relative difference over the entries held to the common bound}."""
    rules = {k: r for k, r in exceptions(name, precision).items() if spread and k in spread}
    ncon, nefc = got['NCON'].ravel().tolist(), got['NEFC'].ravel().tolist()
    rows = [(e, r['name'], (ncon[e], nefc[e]), (r['ncon'], r['nefc'])) for e, r in enumerate(ref) if (ncon[e], nefc[e]) != (r['ncon'], r['nefc'])]
    print('%s FP%d: (contacts, rows) that differ from the oracle (environment, state, kernel, oracle) %s' % (tag, precision, rows))
    if precision == 64: assert not rows, (tag, rows)
    worst, zero, bound = {}, [], {}
    for e, r in enumerate(ref):
        for f, of in SMOOTH + SOLVER:
            if f == 'EFC_FORCE' and (r['nefc'] == 0 or nefc[e] != r['nefc']): continue
            x, y = kernel_field(got, e, f, r['nefc']), oracle_field(a, r, of)
            assert all(np.isfinite(p).all() for p in (x if isinstance(x, tuple) else (x,))), (tag, r['name'], f)
            d, z = _difference(x, y)
            if z: zero.append((r['name'], f, d)); continue
            worst[(r['name'], f)] = d
            smooth = (f, of) in SMOOTH
            bound[(r['name'], f)] = (TOL_SMOOTH if smooth else TOL_SOLVER)[precision]
            if (r['name'], f) in rules: bound[(r['name'], f)] = rules[(r['name'], f)](bound[(r['name'], f)], spread[(r['name'], f)])
    summary = {}
    for f, _ in SMOOTH + SOLVER:
        common = [k for k in worst if k[1] == f and k not in rules]
        if not common: continue                   # (identically zero in every state: a model without contacts)
        k = max(common, key=worst.get)
        summary[f] = worst[k]
        print('%s FP%d: %-15s largest relative difference to the oracle %.2e (state %s)' % (tag, precision, f, worst[k], k[0]))
    for k in rules:
        if k in worst: print('%s FP%d: state %s %-15s %.2e, bound %.2e from the oracle\'s spread %.2e' % (tag, precision, k[0], k[1], worst[k], bound[k], spread[k]))
    assert all(d == 0 for _, _, d in zero), (tag, [z for z in zero if z[2] != 0])
    asserted = [f for f, _ in SMOOTH + SOLVER] if precision == 64 else [f for f, _ in SMOOTH] + ['QACC']      # (FP32 forces and sensors are printed)
    bad = {k: (v, bound[k]) for k, v in worst.items() if k[1] in asserted and not v < bound[k]}
    assert not bad, (tag, bad)
    # the first state again as the last environment: equal to the bit
    for f in got:
        assert np.array_equal(got[f][0], got[f][-1]), (tag, f)
    assert not got['WARN_EVER'].any(), (tag, got['WARN_EVER'].ravel().tolist())
    return summary


def check_properties(a, name, ref):
    """the properties of the module docstring, on the oracle's evaluation of the states"""
    task = task_of(name)
    by = {r['name']: r for r in ref}
    nv = len(a['dof_bodyid'])
    assert len(ref) % 4 != 0 and by[ref[0]['name'] + ' again'] is ref[-1], (name, len(ref))
    J = np.nonzero((a['jnt_type'] == 3) & (a['jnt_limited'] != 0))[0]
    qj = by['limits']['q'][a['jnt_qposadr'][J]]
    hinge_limited = int(((qj > a['jnt_range'][J, 1] + 1.9) | (qj < a['jnt_range'][J, 0] - 1.9)).sum())       # hinges 2 rad beyond their range
    if task == 'flight_imitation':
        roll = [by['roll%d' % e] for e in range(4)]
        print(name, 'rollout states: (max|qvel|, max|qfrc_fluid|)', [(float(np.abs(r['v']).max()), float(np.abs(r['qfrc_fluid']).max())) for r in roll])
        assert sum(np.abs(r['v']).max() > 1e3 and np.abs(r['qfrc_fluid']).max() > 1 for r in roll) >= 3
        assert len({tuple(np.round(r['q'][7:], 6)) for r in roll}) == 4                  # four wing-beat phases
        assert not by['still']['qfrc_fluid'].any() and by['still']['qfrc_passive'].any()
        for k, ax in enumerate('xyz'):
            p, n = by['+' + ax], by['-' + ax]
            assert np.count_nonzero(p['v']) == 1 and p['v'][k] == -n['v'][k] == 50.0
            assert p['qfrc_fluid'][k]*n['qfrc_fluid'][k] < 0 and p['qfrc_fluid'][k] < 0, (ax, p['qfrc_fluid'][k], n['qfrc_fluid'][k])      # drag opposes the motion
    else:
        for k in range(3):
            r = by['rand%d' % k]
            assert r['ctrl'].all() and r['act'].all() and np.abs(r['qfrc_actuator']).max() > 0
        d = _rel(by['adhesion']['qfrc_actuator'], by['adhesion0']['qfrc_actuator'])
        print(name, 'adhesion at 1 against 0: qfrc_actuator changes by', d, 'contacts', by['adhesion']['ncon'])
        assert d > 1e-3 and by['adhesion']['ncon'] > 0
        if task == 'walk_on_ball':
            root = a['body_rootid']
            assert sorted(set(root.tolist())) == [0, 1, 68]
            dof = int(a['jnt_dofadr'][np.nonzero(a['jnt_type'] == 1)[0][0]])
            assert np.linalg.norm(by['spin']['v'][dof:dof + 3]) >= 10
            assert np.abs(by['spin']['cvel'].reshape(-1, 6)[68]).max() >= 5
            # the two reference points are apart: raw linear parts about the model's CoM and about the trees' differ
            sc = by['spin']['subtree_com'].reshape(-1, 3)
            assert np.linalg.norm(sc[1] - sc[0]) > 1e-2 and np.linalg.norm(sc[68] - sc[0]) > 1e-2
    qa = _quat_adr(a)
    for s in (1.3, 1e-3):
        assert abs(np.linalg.norm(by['quat*%g' % s]['q'][qa:qa + 4]) - s) < 1e-6*s
        assert _rel(by['quat*%g' % s]['xpos'], ref[0]['xpos']) < 1e-6                   # the oracle normalises it as well
    lim = a['actuator_forcelimited'] != 0
    for tag in ('ctrl+5', 'ctrl-5'):
        f = by[tag]['actuator_force']
        at = lim & ((f == a['actuator_forcerange'][:, 0]) | (f == a['actuator_forcerange'][:, 1]))
        print(name, tag, 'actuators at a force clamp:', int(at.sum()), 'of', int(lim.sum()), 'limited')
        assert at.any()
    assert np.abs(by['qvel*300']['v']).max() > 300
    print(name, 'limits: rows', by['limits']['nefc'], 'contacts', by['limits']['ncon'], 'hinges beyond their range', hinge_limited, 'of', len(J))
    assert by['limits']['nefc'] >= hinge_limited > 20 and by['limits']['nefc'] < 192 and by['limits']['ncon'] < 64
    A = np.array([j for j in J if 'abdomen' in str(a['names_jnt'][j])])
    ql, qf = by['limits']['q'][a['jnt_qposadr'][A]], by['folded']['q'][a['jnt_qposadr'][A]]
    assert np.array_equal(ql, ref[0]['q'][a['jnt_qposadr'][A]])                                   # 'limits': the abdomen where the first state has it ...
    beyond = (qf > a['jnt_range'][A, 1] + 1.9) | (qf < a['jnt_range'][A, 0] - 1.9)
    print(name, 'folded: rows', by['folded']['nefc'], 'contacts', by['folded']['ncon'], 'abdomen hinges beyond their range', int(beyond.sum()), 'of', len(A))
    assert beyond.sum() >= 8 and by['folded']['nefc'] < 192 and by['folded']['ncon'] < 64          # ... 'folded': beyond it, below the caps
    if _free_root(a): assert by['far']['q'][:2].tolist() == [50.0, -30.0]
    else: assert 'far' not in by
    assert len(by['qvel*300']['v']) == nv


def exceptions(name, precision):
    """{(state, field): rule} of EXCEPTIONS for one model and precision"""
    task = task_of(name)
    return {(st, f): rule for model, st, fields, precisions, rule in EXCEPTIONS if model in (None, task) and precision in precisions for f in fields}


def spreads(a, name, S, precision):
    """{(state, field): the oracle's one-ulp spread} for the exceptions of one model and precision (FP32: units of single precision at the
    rounded state, FP64: of double precision)"""
    by = {s['name']: s for s in S}
    want = {}
    for (st, f) in exceptions(name, precision):
        if st in by: want.setdefault(st, []).append((f, dict(SMOOTH + SOLVER)[f]))
    out = {}
    for st, fields in want.items():
        sp = ulp_spread(a, by[st], tuple(fields), precision)
        out.update({(st, f): sp[of] for f, of in fields})
    return out
