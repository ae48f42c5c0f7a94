"""The assertions on fb_batch_lqr_backward (csrc/fb_riccati.hpp), shared by tests/test_lqr_backward_emulation.py (the
kernel-source emulation build, no GPU) and tests/test_gpu_lqr_backward.py (the MI355X, both engine builds).

Inputs are synthetic, well conditioned and seeded: A = 0.9 x a random orthogonal matrix + 0.05 x normal noise, B normal, Q = G'G/ndx + 0.1 I,
R = H'H/nu + I, q and r normal, all different for every (nominal, interval).  REFERENCE AND BOUND: the recursion is computed twice on the
CPU, by lqr.backward_pass in FP64 and by the same formulas in np.longdouble with a hand-written Cholesky solve; e_ref is the largest
relative difference (max |delta| / max |ref|, per array) between the two -- numpy's own rounding on the problem.  The kernel's error
against the longdouble reference must be <= 10 x e_ref, with a floor of 64 eps, per array (K, k, P, p, dV).  The factor 10 is for another
summation order (k in blocks of 4 on the matrix core against BLAS's), the project's own margin in DESIGN.md 21's first-order test.
"""
import ctypes as C
import functools

import numpy as np
import pytest

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
ARRAYS = ('K', 'k', 'P', 'p', 'dV')
SHAPES = [(5, 2, 3, 2), (16, 16, 2, 1), (17, 1, 2, 3), (33, 5, 2, 2), (64, 64, 1, 1), (275, 59, 2, 2)]          # (ndx, nu, T, n_nom)


class Ctx:
    """batch: an engine.Batch of the build under test; dev: numpy -> tensor where it computes; np_: back; sync: wait for the device."""

    def __init__(self, batch, make_batch, dev, np_, sync=lambda: None, tag=''):
        self.batch, self.make_batch, self.dev, self.np_, self.sync, self.tag = batch, make_batch, dev, np_, sync, tag


# ------------------------------------------------------------------ inputs
def problem(ndx, nu, T, n, seed):
    rng = np.random.default_rng(seed)
    A = np.empty((n, T, ndx, ndx))
    for m in range(n):
        for t in range(T):
            A[m, t] = 0.9*np.linalg.qr(rng.standard_normal((ndx, ndx)))[0] + 0.05*rng.standard_normal((ndx, ndx))
    B = rng.standard_normal((n, T, ndx, nu))
    G = rng.standard_normal((ndx, ndx)); H = rng.standard_normal((nu, nu))
    Q = G.T @ G/ndx + 0.1*np.eye(ndx); R = H.T @ H/nu + np.eye(nu)
    return dict(A=A, B=B, Q=Q, R=R, q=rng.standard_normal((n, T + 1, ndx)), r=rng.standard_normal((n, T, nu)))


# ------------------------------------------------------------------ the longdouble reference
def _chol_ld(M):
    n = len(M); L = np.zeros((n, n), LD)
    for j in range(n):
        d = M[j, j] - L[j, :j] @ L[j, :j]
        if not (d > 0 and np.isfinite(d)):
            return None
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j] @ L[j, :j])/L[j, j]
    return L


def _solve_ld(L, b):
    n = len(L); y = np.array(b, LD)
    for i in range(n):
        y[i] = (y[i] - L[i, :i] @ y[:i])/L[i, i]
    for i in range(n - 1, -1, -1):
        y[i] = (y[i] - L[i + 1:, i] @ y[i + 1:])/L[i, i]
    return y


def backward_ld(A, B, Q, R, Qf=None, q=None, r=None, mu=None):
    """The formulas of include/flybody_engine.h in np.longdouble: dict of K, k, P, p, dV, status."""
    n, T, ndx, nu = B.shape
    A, B, Q, R = (np.asarray(x, LD) for x in (A, B, Q, R))
    Qf = Q if Qf is None else np.asarray(Qf, LD)
    q = np.zeros((n, T + 1, ndx), LD) if q is None else np.asarray(q, LD)
    r = np.zeros((n, T, nu), LD) if r is None else np.asarray(r, LD)
    mu = np.zeros(n, LD) if mu is None else np.asarray(mu, LD)
    K = np.zeros((n, T, nu, ndx), LD); k = np.zeros((n, T, nu), LD); P = np.zeros((n, T + 1, ndx, ndx), LD); p = np.zeros((n, T + 1, ndx), LD)
    dV = np.zeros((n, 2), LD); status = np.zeros(n, np.int32)
    for m in range(n):
        P[m, T] = Qf; p[m, T] = q[m, T]
        for t in range(T - 1, -1, -1):
            At, Bt, Pn, pn = A[m, t], B[m, t], P[m, t + 1], p[m, t + 1]
            W = Pn @ At; Y = Pn @ Bt
            Qxx = Q + At.T @ W; Qux = Bt.T @ W; Quu = R + Bt.T @ Y
            Qx = q[m, t] + At.T @ pn; Qu = r[m, t] + Bt.T @ pn
            L = _chol_ld(Quu + mu[m]*np.eye(nu, dtype=LD))
            if L is None:
                status[m] = 1 + t; dV[m] = 0
                K[m, :t + 1] = 0; k[m, :t + 1] = 0; P[m, :t + 1] = 0; p[m, :t + 1] = 0
                break
            Kt = -_solve_ld(L, Qux); kt = -_solve_ld(L, Qu)
            Pt = Qxx + Kt.T @ Quu @ Kt + Kt.T @ Qux + Qux.T @ Kt
            K[m, t] = Kt; k[m, t] = kt; P[m, t] = (Pt + Pt.T)/2
            p[m, t] = Qx + Kt.T @ (Quu @ kt + Qu) + Qux.T @ kt
            dV[m, 0] += 2*(kt @ Qu); dV[m, 1] += kt @ Quu @ kt
    return dict(K=K, k=k, P=P, p=p, dV=dV, status=status)


@functools.lru_cache(maxsize=None)
def reference(ndx, nu, T, n, seed, with_mu):
    """(problem, mu, numpy FP64 result, longdouble result, e_ref per array): computed once per process and shared, never modified."""
    from flybody_amd import lqr
    pr = problem(ndx, nu, T, n, seed)
    mu = 0.1*(1.0 + np.arange(n)) if with_mu else None
    f64 = dict(zip(ARRAYS + ('status',), lqr.backward_pass(pr['A'], pr['B'], pr['Q'], pr['R'], None, pr['q'], pr['r'], mu)))
    ld = backward_ld(pr['A'], pr['B'], pr['Q'], pr['R'], None, pr['q'], pr['r'], mu)
    assert not f64['status'].any() and not ld['status'].any()                    # numpy's own recursion meets no non-positive pivot here
    return pr, mu, f64, ld, {a: rel(f64[a], ld[a]) for a in ARRAYS}


def rel(x, ref):
    den = float(np.abs(ref).max())
    return float(np.abs(np.asarray(x, LD) - ref).max())/den if den > 0 else float(np.abs(x).max())


def run(c, pr, mu=None, q=True, r=True, want_P=True, batch=None, **kw):
    d = lambda x: None if x is None else c.dev(x)
    res = (batch or c.batch).lqr_backward(d(pr['A']), d(pr['B']), d(pr['Q']), d(pr['R']), d(pr.get('Qf')), d(pr['q']) if q else None,
                                          d(pr['r']) if r else None, d(mu), want_P=want_P, **kw)
    c.sync()
    return res


def as_numpy(c, res):
    return {f: None if getattr(res, f) is None else c.np_(getattr(res, f)) for f in res._fields}


def assert_within_bound(c, got, ld, e_ref, what, arrays=ARRAYS):
    errs = {a: rel(got[a], ld[a]) for a in arrays}
    print(f'{what} [{c.tag}]: ' + '  '.join(f'{a} {errs[a]:.1e} (numpy {e_ref[a]:.1e})' for a in arrays))
    for a in arrays:
        assert np.isfinite(got[a]).all(), a
        assert errs[a] <= max(10*e_ref[a], 64*EPS), (what, a, errs[a], e_ref[a])
    return errs


# ------------------------------------------------------------------ 1: the tile map and every edge, exact
GEMM_SHAPES = [(16, 16, 4), (17, 5, 3), (33, 16, 17), (275, 59, 275)]                # (m, n, k)


def gemm_is_exact_on_small_integers(c):
    """C = op(X) op(Y) + D bit for bit against numpy, for the four op combinations, on integer entries in -3 .. 3 (every partial sum is an
    integer below 2^53: any summation order gives the same bits, a wrong lane map does not).  X and Y are random, hence asymmetric."""
    rng = np.random.default_rng(5)
    for m, n, k in GEMM_SHAPES:
        for tx in (False, True):
            for ty in (False, True):
                X = rng.integers(-3, 4, (k, m) if tx else (m, k)).astype(np.float64)
                Y = rng.integers(-3, 4, (n, k) if ty else (k, n)).astype(np.float64)
                D = rng.integers(-3, 4, (m, n)).astype(np.float64)
                want = (X.T if tx else X) @ (Y.T if ty else Y)
                got = c.batch.riccati_gemm(c.dev(X), c.dev(Y), c.dev(D), trans_x=tx, trans_y=ty)
                got0 = c.batch.riccati_gemm(c.dev(X), c.dev(Y), None, trans_x=tx, trans_y=ty)
                c.sync()
                assert np.array_equal(c.np_(got), want + D), (m, n, k, tx, ty)
                assert np.array_equal(c.np_(got0), want), (m, n, k, tx, ty)


# ------------------------------------------------------------------ 2: shapes
def shape_matches_the_reference(c, i):
    """Full outputs at one of SHAPES against the longdouble reference.  Shapes with an even index run with mu NULL (the short form of
    P_t), those with an odd index with mu = 0.1 (1 + m) (the general form)."""
    ndx, nu, T, n = SHAPES[i]
    pr, mu, f64, ld, e_ref = reference(ndx, nu, T, n, 100 + i, i % 2 == 1)
    got = as_numpy(c, run(c, pr, mu))
    assert got['K'].shape == (n, T, nu, ndx) and got['k'].shape == (n, T, nu) and got['P'].shape == (n, T + 1, ndx, ndx)
    assert got['p'].shape == (n, T + 1, ndx) and got['dV'].shape == (n, 2) and got['status'].tolist() == [0]*n
    assert_within_bound(c, got, ld, e_ref, f'shape {SHAPES[i]}')
    flat = got['K'].reshape(n*T, -1); fk = got['k'].reshape(n*T, -1)               # gains differ across (m, t): the indexing is live
    for a in range(n*T):
        for b in range(a):
            assert not np.allclose(flat[a], flat[b], rtol=1e-3) and not np.allclose(fk[a], fk[b], rtol=1e-3)


# ------------------------------------------------------------------ 3: special cases
def plain_tvlqr(c):
    """q = r = mu = NULL: the recursion of lqr.tvlqr (existing code), at the same bound; k, p and dV are exactly zero."""
    from flybody_amd import lqr
    pr = problem(33, 5, 3, 2, 7)
    K, P = lqr.tvlqr(pr['A'], pr['B'], pr['Q'], pr['R'])
    ld = backward_ld(pr['A'], pr['B'], pr['Q'], pr['R'])
    e_ref = dict(K=rel(K, ld['K']), P=rel(P, ld['P']))
    got = as_numpy(c, run(c, pr, q=False, r=False))
    assert_within_bound(c, got, ld, e_ref, 'against tvlqr', ('K', 'P'))
    assert not got['k'].any() and not got['p'].any() and not got['dV'].any() and not got['status'].any()
    res = run(c, pr, q=False, r=False, want_P=False)
    assert res.P is None and res.p is None and np.array_equal(c.np_(res.K), got['K'])
    # lqr.tvlqr(batch=...) is this call, returned as numpy
    Kb, Pb = lqr.tvlqr(pr['A'], pr['B'], pr['Q'], pr['R'], batch=c.batch)
    assert np.array_equal(Kb, got['K']) and np.array_equal(Pb, got['P'])


def regularisation_shrinks_the_gain(c):
    """mu = [0, 0.5, 10] on three copies of one problem: |K| falls monotonically, and all three match the reference."""
    from flybody_amd import lqr
    one = problem(17, 5, 3, 1, 11)
    pr = {a: (np.repeat(v, 3, axis=0) if a in ('A', 'B', 'q', 'r') else v) for a, v in one.items()}
    mu = np.array([0.0, 0.5, 10.0])
    f64 = dict(zip(ARRAYS, lqr.backward_pass(pr['A'], pr['B'], pr['Q'], pr['R'], None, pr['q'], pr['r'], mu)))
    ld = backward_ld(pr['A'], pr['B'], pr['Q'], pr['R'], None, pr['q'], pr['r'], mu)
    got = as_numpy(c, run(c, pr, mu))
    assert_within_bound(c, got, ld, {a: rel(f64[a], ld[a]) for a in ARRAYS}, 'mu 0 / 0.5 / 10')
    norms = [float(np.linalg.norm(got['K'][m])) for m in range(3)]
    assert norms[0] > norms[1] > norms[2] > 0, norms


def _cost_change(pr, K, k, alpha, m):
    """J of the linear model simulated in numpy under du = alpha k + K dx from dx_0 = 0 (where J = 0 for alpha = 0)."""
    T = K.shape[1]; dx = np.zeros(K.shape[-1]); J = 0.0
    for t in range(T):
        du = alpha*k[m, t] + K[m, t] @ dx
        J += dx @ pr['Q'] @ dx + du @ pr['R'] @ du + 2*pr['q'][m, t] @ dx + 2*pr['r'][m, t] @ du
        dx = pr['A'][m, t] @ dx + pr['B'][m, t] @ du
    return J + dx @ pr['Q'] @ dx + 2*pr['q'][m, T] @ dx


def dV_predicts_the_line_search(c):
    """q, r non-zero, mu = 0: the change of J equals alpha dV[0] + alpha^2 dV[1] for alpha 1, 0.5, 0.25 to 1e-9 relative, and that is
    minimal at alpha = 1."""
    pr = problem(17, 5, 4, 2, 13)
    got = as_numpy(c, run(c, pr))
    for m in range(2):
        d0, d1 = got['dV'][m]
        assert d0 < 0 < d1
        for alpha in (1.0, 0.5, 0.25):
            J = _cost_change(pr, got['K'], got['k'], alpha, m)
            assert abs(J - (alpha*d0 + alpha*alpha*d1)) <= 1e-9*abs(J), (m, alpha, J, d0, d1)
        assert abs(-d0/(2*d1) - 1.0) <= 1e-9                                      # the parabola's minimum
        assert _cost_change(pr, got['K'], got['k'], 1.0, m) < min(_cost_change(pr, got['K'], got['k'], a, m) for a in (0.9, 1.1))


# ------------------------------------------------------------------ 4: stationary mode
def stationary_mode_is_lqr(c):
    """A stabilisable pair at (17, 5), horizon 200: P_0 matches lqr.lqr (existing code) to its tol -- lqr stops at a Riccati residual of
    tol |P|, which for a contraction of rate rho lies within tol/(1 - rho) of the fixed point: 10 tol covers rho <= 0.9, and the
    closed loop here has rho^2 below 0.75 --, P_0 against P_1 is below 1e-10 relative, the outputs have a time axis of 1."""
    from flybody_amd import lqr
    one = problem(17, 5, 1, 1, 17)
    A, B = one['A'][0, 0], one['B'][0, 0]
    tol = 1e-10
    K, P = lqr.lqr(A, B, one['Q'], one['R'], tol=tol)
    assert np.abs(np.linalg.eigvals(A + B @ K)).max()**2 < 0.75
    pr = dict(A=np.ascontiguousarray(one['A'][:, 0]), B=np.ascontiguousarray(one['B'][:, 0]), Q=one['Q'], R=one['R'], q=None, r=None)
    got = as_numpy(c, run(c, pr, q=False, r=False, stationary=True, horizon=200))
    assert got['K'].shape == (1, 1, 5, 17) and got['k'].shape == (1, 1, 5) and got['P'].shape == (1, 2, 17, 17) and got['p'].shape == (1, 2, 17)
    e = [rel(got['P'][0, 0], P), rel(got['P'][0, 0], got['P'][0, 1]), rel(got['K'][0, 0], K)]
    print(f'stationary [{c.tag}]: P_0 against lqr.lqr {e[0]:.1e}, against P_1 {e[1]:.1e}, K against lqr.lqr {e[2]:.1e}')
    assert e[0] <= 10*tol and e[1] < 1e-10 and e[2] <= 10*tol and got['status'].tolist() == [0]
    Kb, Pb = lqr.lqr(A, B, one['Q'], one['R'], tol=tol, batch=c.batch)
    assert rel(Pb, P) <= 10*tol and rel(Kb, K) <= 10*tol


# ------------------------------------------------------------------ 5: failure is data
def failure_is_data(c):
    """One indefinite R for the call; nominals 0 and 2 have a B large enough that R + B'PB is positive definite all the way, nominal 1 has
    a tiny B at t = 1 of T = 3, where Quu is R to rounding: status [0, 2, 0], nominal 1 zero from t = 1 down and finite everywhere, the
    others bit-equal to a call without it."""
    from flybody_amd import lqr
    pr = problem(6, 3, 3, 3, 19)
    pr['B'] *= 10.0; pr['B'][1, 1] *= 1e-3
    pr['R'] = np.diag([1.0, 1.0, -0.5])
    ref = dict(zip(ARRAYS + ('status',), lqr.backward_pass(pr['A'], pr['B'], pr['Q'], pr['R'], None, pr['q'], pr['r'])))
    assert ref['status'].tolist() == [0, 2, 0]                                   # the numpy reference fails there and nowhere else
    got = as_numpy(c, run(c, pr))
    assert got['status'].tolist() == [0, 2, 0]
    for a in ARRAYS:
        assert np.isfinite(got[a]).all(), a
    assert not got['K'][1, :2].any() and not got['k'][1, :2].any() and not got['P'][1, :2].any() and not got['p'][1, :2].any() and not got['dV'][1].any()
    for a in ('K', 'k'):
        assert rel(got[a][1, 2], ref[a][1, 2]) < 1e-12                           # the interval before the failure is a result
    assert rel(got['P'][1, 2:], ref['P'][1, 2:]) < 1e-12
    for a in ARRAYS:
        assert rel(got[a][[0, 2]], ref[a][[0, 2]]) < 1e-11, a
    sub = {a: (np.ascontiguousarray(v[[0, 2]]) if a in ('A', 'B', 'q', 'r') else v) for a, v in pr.items()}
    two = as_numpy(c, run(c, sub))
    for a in ARRAYS + ('status',):
        assert np.array_equal(two[a], got[a][[0, 2]]), a
    # a pivot that is not finite is the same verdict, and writes no NaN
    bad = {a: v.copy() for a, v in pr.items()}; bad['B'][0, 2, 0, 0] = np.inf
    got = as_numpy(c, run(c, bad))
    assert got['status'].tolist() == [3, 2, 0]
    for a in ARRAYS:
        assert np.isfinite(got[a]).all() and not got[a][0, :3].any(), a          # (P_T = Qf and p_T = q_T lie behind the failing interval)
    assert np.array_equal(got['K'][2], two['K'][1])


# ------------------------------------------------------------------ 6, 7: determinism and the hand-over
def determinism_and_regrowth(c):
    """Two calls give the same bits; a call with larger shapes in between (the workspace grows) does not change them; n_nom = 1 alone is
    nominal 0 of a batch of 3."""
    batch = c.make_batch()
    pr = problem(33, 5, 2, 3, 23)
    a = as_numpy(c, run(c, pr, batch=batch))
    b = as_numpy(c, run(c, pr, batch=batch))
    run(c, problem(40, 7, 3, 4, 29), batch=batch)
    d = as_numpy(c, run(c, pr, batch=batch))
    one = {k: (np.ascontiguousarray(v[:1]) if k in ('A', 'B', 'q', 'r') else v) for k, v in pr.items()}
    e = as_numpy(c, run(c, one, batch=batch))
    for f in ARRAYS + ('status',):
        assert np.array_equal(a[f], b[f]) and np.array_equal(a[f], d[f]) and np.array_equal(a[f][:1], e[f]), f


def hand_over_without_a_copy(c):
    """K is returned as Kt.transpose(2, 3): the transposition rollout_feedback applies gives back the tensor the kernel wrote."""
    res = run(c, problem(5, 2, 3, 2, 31))
    Kt = res.K.transpose(2, 3)
    assert res.K.shape == (2, 3, 2, 5) and Kt.is_contiguous() and not res.K.is_contiguous()
    assert Kt.contiguous().data_ptr() == res.K.data_ptr() == Kt.data_ptr()


# ------------------------------------------------------------------ 8: refusals
class _Cfg(C.Structure):
    _fields_ = [('n_nom', C.c_int32), ('horizon', C.c_int32), ('ndx', C.c_int32), ('nu', C.c_int32), ('stationary', C.c_int32)]


def refusals(c):
    import torch
    b = c.batch; L = b.L
    pr = problem(5, 2, 2, 1, 37)
    t = {a: c.dev(pr[a]) for a in ('A', 'B', 'Q', 'R')}
    Kt = c.dev(np.zeros((1, 2, 5, 2)))
    st = torch.zeros(1, dtype=torch.int32, device=Kt.device)
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    good = dict(b=b.h, cfg=_Cfg(1, 2, 5, 2, 0), A=ptr(t['A']), B=ptr(t['B']), Q=ptr(t['Q']), R=ptr(t['R']), Kt=ptr(Kt), status=ptr(st))

    def call(**kw):
        a = dict(good); a.update(kw)
        cfg = a['cfg']
        rc = L.fb_batch_lqr_backward(a['b'], None if cfg is None else C.byref(cfg), a['A'], a['B'], a['Q'], a['R'], None, None, None, None, a['Kt'], None, None,
                                     None, None, a['status'], None)
        return rc, L.fb_last_error().decode()
    assert call()[0] == 0
    c.sync()
    cases = [(dict(b=None), 'null batch'), (dict(cfg=None), 'null config'), (dict(A=None), 'A is NULL'), (dict(B=None), 'B is NULL'),
             (dict(Q=None), 'Q is NULL'), (dict(R=None), 'R is NULL'), (dict(Kt=None), 'Kt'), (dict(status=None), 'status'),
             (dict(cfg=_Cfg(0, 2, 5, 2, 0)), 'n_nom'), (dict(cfg=_Cfg(1, 0, 5, 2, 0)), 'horizon'), (dict(cfg=_Cfg(1, 2, 0, 2, 0)), 'ndx must'),
             (dict(cfg=_Cfg(1, 2, 5, 0, 0)), 'nu must'), (dict(cfg=_Cfg(1, 2, 1025, 2, 0)), 'ndx 1025 exceeds'),
             (dict(cfg=_Cfg(1, 2, 5, 65, 0)), 'nu 65 exceeds'), (dict(cfg=_Cfg(1, 2, 5, 2, 2)), 'stationary'), (dict(cfg=_Cfg(1, 2, 5, 2, -1)), 'stationary')]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc != 0 and word in msg and 'fb_batch_lqr_backward' in msg, (kw, msg)
    # the shim: dtype, shape, device, contiguity
    A, B, Q, R = t['A'], t['B'], t['Q'], t['R']
    bad = [dict(A=A.float()), dict(B=B[:, :, :4]), dict(B=B[:, :1].contiguous()), dict(Q=Q[:4, :4].contiguous()), dict(R=torch.empty((2, 2), dtype=torch.float64, device='meta')),
           dict(A=A.transpose(2, 3)), dict(A=pr['A']), dict(q=c.dev(np.zeros((1, 2, 5)))), dict(r=c.dev(np.zeros((1, 3, 2)))), dict(mu=c.dev(np.zeros(2))),
           dict(horizon=3), dict(stationary=True), dict(Qf=Q[:4].contiguous())]
    for kw in bad:
        a = dict(A=A, B=B, Q=Q, R=R); a.update(kw)
        with pytest.raises(ValueError):
            b.lqr_backward(**a)
    with pytest.raises(ValueError):
        b.riccati_gemm(A[0, 0], B[0, 0][:4].contiguous())
