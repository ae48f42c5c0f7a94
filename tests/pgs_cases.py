"""States, references and assertions of tests/test_pgs_solver.py: block PGS (fb_constraint.hpp: d_pgs, opt_solver = 0) against the FP64 oracle.

THE STATES are forward evaluations chosen on the CPU with the oracle alone, so that the row counts sit on BOTH SIDES of every threshold
of d_constraint_a's dispatch (LdsCfg, fb_types.hpp):

  library / precision   d_pgs<LDS, S>, slot   d_pgs<LDS, S>, wide placement   d_pgs<global, S>   d_pgs<global, !S>
  default, FP64         <= 43 rows            44 ... 64                       never              >= 65
  12-per-CU, FP64       <= 23                 24 ... 54                       55 ... 64          >= 65
  default, FP32         <= 46                 47 ... 64                       never              >= 65

  * WALK_STATES / BALL_STATES of tests/test_delassus_entry_lanes.py: 0, 1, 3, 10, 11, 15, 16, 17, 33, 40, 65 / 66 rows;
  * WALK_EXTRA (same generator): 23 | 24, 43 | 44, 46 | 47, 54 | 55, 56, 60, 63, 64 | 65 rows; the 56-row state runs out of sweeps on the
    lane == row loop;
  * PRESSED (conftest.random_state at a fixed height): more than 64 rows, where a lane owns rows k, k + 64, k + 128 -- two registers up
    to 128 rows, three up to the cap of 192 -- and a friction block (three consecutive rows) may start at row 62 / 63 or 126 / 127: its
    forces, residuals and block constants then come from two registers (r3_get / r3_set, res_axpy3<false>).  The 158-row state needs all
    opt_iterations sweeps, the 153-row one stops after ~20; the 192-row state is the row cap (64 contacts).

test_pgs_solver.py::test_states_reach_every_branch asserts every one of these properties on the oracle's own evaluation: a state that
loses its property fails there instead of leaving another test green and empty.

A STATE THAT WAS REPLACED, and why.  The first 44-row state was (78, 0.05).  FP64 agrees with the oracle there on the GPU (5.7e-9 on the
forces), FP32 does not: QACC 7.0e-2, on both libraries.  The cause lies in front of the solver: Newton (the model's default) shows the same
7.0e-2 on that state, and the contact list differs -- the FP32 narrow phase returns the normal of one convex pair (a capsule 2.2e-4 deep
in a cylinder, MPR) 0.12 away from the oracle's.  On the GPU that normal moves by 1e-5 ... 0.19 over 16 copies of the state whose qpos is
perturbed by one unit of single precision in the last place (with the one-lane form of the narrow phase as well); in FP64, on the GPU and
in the oracle, it moves by 2e-12 and 2e-8.  The single-precision emulation (exact division and square root) happens to land within 5e-5.
So that state measures the conditioning of the FP32 portal refinement (precision policy), not the solver, and (147, 0.05)
-- 44 rows as well, found by the same search -- stands in its place."""
import numpy as np

from conftest import random_state
from test_delassus_entry_lanes import BALL_STATES, SIZES, WALK_STATES, _state
from test_solver_handover import FIELDS, TOL, _rel

# (seed, joint spread) of _state(arrays, False, seed, spread, False); FP64 and FP32-rounded row counts in the comment
WALK_EXTRA = [(45, 0.05), (19, 0.0), (92, 0.1), (147, 0.05), (270, 0.05), (91, 0.05), (7, 0.0), (184, 0.05), (119, 0.1), (73, 0.0), (57, 0.0),
              (42, 0.05), (55, 0.1)]                                     # 23 24 43 44 46 47 54 55 56 60 63 64 65 rows
# (seed, height) of conftest.random_state: rows, first rows of the friction blocks that straddle a register boundary
PRESSED = [(7, 0.13), (3, 0.13), (3, 0.12), (1, 0.11), (1, 0.10), (20, 0.10), (1, 0.05)]       # 79 (63), 90 (62), 114 (62), 129 (63, 126), 153 (63, 126), 158 (127), 192 (63, 126)
REQUIRED_ROWS = (23, 24, 43, 44, 46, 47, 54, 55, 64, 65)                 # both sides of every threshold of the table above
ROW_CAP = 192


def pgs_arrays(arrays, noslip=None):
    """The model with opt_solver = 0 (mjtSolver numbering: 0 = PGS); noslip = 0 leaves the raw PGS forces (no d_noslip behind the sweeps)."""
    a = dict(arrays); a['opt_solver'] = np.array(0, np.int32)
    if noslip is not None: a['opt_noslip_iterations'] = np.array(noslip)
    return a


def states(arrays, name):
    if name == 'ball': return [_state(arrays, True, *s) for s in BALL_STATES]
    return ([_state(arrays, False, *s) for s in WALK_STATES] + [_state(arrays, False, seed, spread, False) for seed, spread in WALK_EXTRA]
            + [random_state(arrays, np.random.default_rng(seed), z=z) for seed, z in PRESSED])


def oracle_forward(model, qv, precision):
    """FP64 oracle forward evaluations (the FP32 cases start from the state rounded to single precision, as the engine holds it)."""
    from oracle import fbo
    res = []
    for q, v in qv:
        if precision == 32: q = q.astype(np.float32).astype(float); v = v.astype(np.float32).astype(float)
        od = fbo.OracleData(model); od.field('qpos')[:] = q; od.field('qvel')[:] = v; od.call('forward')
        con = od.contacts()
        res.append(dict(q=q, v=v, nefc=int(od.scalar('nefc')), ncon=int(od.scalar('ncon')), niter=int(od.scalar('solver_niter')),
                        blocks=[int(c[10]) for c in con if int(c[9]) == 3 and int(c[10]) >= 0],      # first rows of the friction blocks
                        **{of: od.field(of).copy() for _, of in FIELDS}))
    return res


def placements(model):
    """(rows of the LDS matrix slot, rows of the wide LDS placement) of the library behind an engine.Model, per precision (LdsCfg)."""
    return {p: (model.dim('lds_ar_rows_f%d' % p), model.dim('lds_wide_rows_f%d' % p)) for p in (64, 32)}


def assert_columns(nefc, ar_rows, wide_rows):
    """every column of the dispatch table that exists for these thresholds holds a state, on both sides of each threshold"""
    assert {ar_rows, ar_rows + 1, wide_rows, wide_rows + 1, 64, 65} <= set(nefc), (ar_rows, wide_rows, sorted(nefc))
    assert any(64 < n <= 128 for n in nefc) and any(128 < n < ROW_CAP for n in nefc) and ROW_CAP in nefc, sorted(nefc)


def check_forward(got, ref, precision, tag, max_it):
    """NEFC, EFC_FORCE[:nefc], QFRC_CONSTRAINT, QACC, the sweep counts and the warning bits of every environment against the oracle;
    the figures are printed before they are asserted"""
    from flybody_amd.engine import WARN_BITS
    nefc = got['NEFC'].ravel().tolist(); niter = got['SOLVER_NITER'].ravel().tolist(); warn = got['WARN_EVER'].ravel().tolist()
    print('%s FP%d: (rows, sweeps of the kernel, sweeps of the oracle) %s' % (tag, precision, [(r['nefc'], k, r['niter']) for r, k in zip(ref, niter)]))
    if precision == 64: assert nefc == [r['nefc'] for r in ref]
    else: print('%s FP32: row counts that differ from the oracle (environment, kernel, oracle) %s' % (tag, [(e, n, r['nefc']) for e, (n, r) in enumerate(zip(nefc, ref)) if n != r['nefc']]))
    worst = {}
    for e, r in enumerate(ref):
        n = r['nefc']
        for f, of in FIELDS:
            if f == 'EFC_FORCE' and (n == 0 or nefc[e] != n): continue
            x, y = (got[f][e][:n], r[of][:n]) if f == 'EFC_FORCE' else (got[f][e], r[of])
            assert np.isfinite(x).all(), (tag, e, n, f)
            if np.abs(y).max() == 0: assert np.abs(x).max() == 0, (tag, e, f); continue
            worst[(e, n, f)] = _rel(x, y)
    for f, _ in FIELDS:
        k = max((k for k in worst if k[2] == f), key=worst.get)
        print('%s FP%d: largest relative difference of %s to the oracle %.2e at (environment, rows, field) %s' % (tag, precision, f, worst[k], k))
    asserted = [f for f, _ in FIELDS] if precision == 64 else ['QACC']          # (FP32 forces are printed, as in the Newton tests)
    bad = {k: v for k, v in worst.items() if k[2] in asserted and not v < TOL[precision]}
    assert not bad, (tag, bad)
    for e, r in enumerate(ref):
        assert (niter[e] >= 1) == (nefc[e] > 0) and niter[e] <= max_it, (tag, e, nefc[e], niter[e])
        assert bool(warn[e] & WARN_BITS['SOLVER_MAXITER']) == (niter[e] == max_it), (tag, e, nefc[e], niter[e], warn[e])
        assert not warn[e] & (WARN_BITS['SOLVER_FALLBACK'] | WARN_BITS['CCD_MAXITER']), (tag, e, warn[e])
        if r['nefc'] != ROW_CAP: assert not warn[e] & (WARN_BITS['CONTACT_CAP'] | WARN_BITS['EFC_CAP']), (tag, e, nefc[e], warn[e])
    return worst


# ------------------------------------------------------------------ rollouts
ROLL_STEPS, ROLL_ENVS = 20, 8
ROLL_CASES = {'short': dict(frames=8, kw=dict(future_steps=2)), 'full': dict(frames=None, kw={})}


def roll_actions():
    """even environments under U(-1, 1), odd ones under the bench's clipped N(0, 1): any leading slice of the batch holds both"""
    rng = np.random.default_rng(41)
    u = rng.uniform(-1, 1, (ROLL_STEPS, ROLL_ENVS, 59)); g = np.clip(rng.normal(size=(ROLL_STEPS, ROLL_ENVS, 59)), -1.0, 1.0)
    return np.where((np.arange(ROLL_ENVS) % 2 == 0)[None, :, None], u, g).astype(np.float32)


def oracle_rollout(model, reference, case):
    from oracle import fbo
    qp, qv = reference
    c = ROLL_CASES[case]; T = c['frames'] or len(qp)
    acts = roll_actions()
    ods = []
    for _ in range(ROLL_ENVS):
        od = fbo.OracleData(model); od.configure_env(qp[:T], qv[:T], terminal_com_dist=float('inf'), **c['kw']); od.env_reset(); ods.append(od)
    types = []
    for k in range(ROLL_STEPS):
        fbo.step_batch(ods, acts[k].astype(np.float64)); types.append([int(od.scalar('step_type')) for od in ods])
    return dict(acts=acts, types=np.array(types), qpos=np.array([od.field('qpos').copy() for od in ods]), qvel=np.array([od.field('qvel').copy() for od in ods]))


def check_rollout(B, n, reference, case, ref, step, tag):
    """n environments of the batch B through the oracle's control steps, environment e against oracle environment e % ROLL_ENVS;
    step(k) runs control step k and waits for it"""
    qp, qv = reference
    c = ROLL_CASES[case]; T = c['frames'] or len(qp)
    own = np.arange(n) % ROLL_ENVS
    B.set_reference(qp[:T], qv[:T], terminal_com_dist=float('inf'), **c['kw']); B.reset()
    rows = sweeps = 0
    for k in range(ROLL_STEPS):
        step(k)
        assert B.get('STEP_TYPE').ravel().tolist() == ref['types'][k][own].tolist(), (tag, k, B.get('STEP_TYPE').ravel().tolist(), ref['types'][k].tolist())
        rows = max(rows, int(B.get('NEFC').max())); sweeps = max(sweeps, int(B.get('SOLVER_NITER').max()))
    if case == 'short': assert (ref['types'][:, own] == 2).any() and (ref['types'][:, own] == 0).any()       # episodes ended and restarted inside the rollout
    Q, V = B.get('QPOS'), B.get('QVEL')
    eq = max(_rel(Q[e], ref['qpos'][own[e]]) for e in range(n)); ev = max(_rel(V[e], ref['qvel'][own[e]]) for e in range(n))
    print('%s, %s reference: qpos %.2e qvel %.2e relative to the oracle after %d control steps of %d environments; up to %d rows, %d sweeps'
          % (tag, case, eq, ev, ROLL_STEPS, n, rows, sweeps))
    assert rows > 0 and sweeps > 1, (tag, rows, sweeps)           # the warm start was used: some substep solved a system in more than one sweep
    assert eq < 1e-6 and ev < 1e-6, (tag, eq, ev)
