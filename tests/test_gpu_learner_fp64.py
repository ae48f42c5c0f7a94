"""The learner's loss, layer-epilogue, Gaussian-head and optimizer kernels (include/flybody_learner.h; float32 on the GPU) against
FLOAT64 restatements of the same operations (tests/learner_fp64.py), at the smallest shapes that reach every guard, tail and branch of
each kernel plus the workload's own shape.

TOLERANCES.  A float32-against-float32 comparison cannot see a formula that is wrong in float32 on both sides, and a fixed tolerance
wide enough for the worst input hides everything on the others.  So every compared quantity is evaluated three times: by the kernel,
in float64, and by the float64 text run in float32 on the CPU (cancellation-free forms where they matter).  With err = max |. - float64|
(relative where noted), the bound on the kernel is

        err_kernel <= FACTOR * err_ref + ULPS ulp(scale of the quantity)             FACTOR = 4, ULPS = 4 unless listed below

-- never a multiple of the kernel's own error.  4 x covers the summation order of atomics / wave reductions and a different libm.
GEMM-like outputs keep the project's rtol = 2e-5, atol = 2e-5.  Two conditions were fixed before any GPU run: the per-dimension
batch-mean stddev KL within 1e-3 relative at delta = 3e-4 and 1e-4 (B = 256), and d zs from fbl_gauss_head_bwd_std within 1e-5 relative
for pre-activations in [-16, 4].

Factors other than the default (measured on an MI355X; the table is repeated in DESIGN.md section 5):

    quantity                          kernel error   err_ref    measured   FACTOR   cause
    fbl_td_loss d_logits              5.77e-9        9.31e-10   6.2 x      8        (N, B, K) = (20, 256, 51), geometric support, logits of scale
        30.  Both errors are ONE float32 rounding: that of z = r + gamma d v on a row where r = -2436 and gamma d v cancel and z lands where
        the atoms are ~1 apart (an error of ulp(2436) / 2 in z moves 1e-4 of the mass to the neighbouring atom).  The kernel rounds
        fma(gamma d, v, r) once, the CPU rounds the product and the sum: float64 with z rounded the kernel's way gives 5.75e-9, rounded the
        CPU's way 9.15e-10 -- neither is the more careful, the input decides which lands closer.  Every other d_logits case is below 4 x.

What the first GPU run of these tests found besides the two conditions (fixed in the kernel and in dmpo/losses.py; the figures are the
kernel's error before -> after, in units of err_ref):
    d_log_temperature, Q = 150 + N(0, 1), T = 0.05       4357 x -> 3.2 x    lse(q / T) and sum w q / T were batch-averaged separately (|q / T| ~ 3000)
      and with every dual at -18 (T = 2.5e-8)            2.9e7 x -> 8.2 x   (below the 4-ulp floor)
    d_online_mean / d_online_std, same inputs            17.8 x / 14.4 x -> 1.0 x / 0.7 x    q / T - max / T: 2e-4 on every weight
    d_online_std, os == ts, alpha_stddev = 1000          120 x -> below 4 x   alpha (1 / os - ts^2 / os^3) cancels; now -alpha r (2 + r) / os
    loss_kl_std, kl_stddev_rel at delta = 3e-4 / 1e-4    7-11 x with 0.5 expm1(2 d) - d, d = log ts - log os (the two logarithms carry
      1e-7 each against d = 3e-4; and 0.5 expm1(2 d) - d = d^2 + ... still cancels) -> below 4 x with (r - log1p r) + r^2 / 2, r = (ts - os) / os
"""
import math

import numpy as np
import pytest
import torch

import learner_fp64 as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
EPS32 = R.EPS32
DEV = 'cuda'

# quantity -> (FACTOR, ULPS) where the default (4, 4) does not hold (the table in the module's docstring)
_FACTORS = {'td d_logits': (8.0, 4.0)}


class Checker:
    """Collects every comparison of a test, prints the figures, and fails at the end with all the misses."""

    def __init__(self, what):
        self.what = what; self.miss = []

    @staticmethod
    def err(a, ref, rel):
        a = a.detach().double().cpu().reshape(ref.shape); e = (a - ref.double()).abs()
        if rel:
            e = e/ref.double().abs().clamp_min(1e-300)
        return float(e.max()) if e.numel() else 0.0

    def check(self, name, got, ref64, ref32, rel=False, scale=None, key=None):
        factor, ulps = _FACTORS.get(key or name, (4.0, 4.0))
        e, eref = self.err(got, ref64, rel), self.err(ref32, ref64, rel)
        if scale is None:
            scale = 1.0 if rel else (float(ref64.abs().max()) if ref64.numel() else 0.0)
        bound = factor*eref + ulps*EPS32*float(scale)
        ok = e <= bound
        print('%s %-28s kernel %.3e  err_ref %.3e  bound %.3e  (%.1f x err_ref)%s' % (self.what, name, e, eref, bound, e/max(eref, 1e-300) if eref else float('inf'),
                                                                                   '' if ok else '   <-- MISS'))
        if not ok:
            self.miss.append((name, e, eref, bound))

    def limit(self, name, value, bound):
        ok = value <= bound
        print('%s %-28s %.3e  (fixed bound %.3e)%s' % (self.what, name, value, bound, '' if ok else '   <-- MISS'))
        if not ok:
            self.miss.append((name, value, None, bound))

    def close(self, name, got, ref64, rtol=2e-5, atol=2e-5):
        a = got.detach().double().cpu(); ok = torch.allclose(a, ref64, rtol=rtol, atol=atol)
        print('%s %-28s max |err| %.3e (rtol %.0e, atol %.0e)%s' % (self.what, name, float((a - ref64).abs().max()), rtol, atol, '' if ok else '   <-- MISS'))
        if not ok:
            self.miss.append((name, float((a - ref64).abs().max()), None, atol))

    def done(self):
        assert not self.miss, '%s: %s' % (self.what, self.miss)


def _gpu(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


# ====================================================================================================== MPO loss
EPS = dict(epsilon=0.1, epsilon_penalty=0.1, epsilon_mean=0.0025, epsilon_stddev=1e-7)
DUALS_SMALL = dict(log_temperature=1.5, log_alpha_mean=2.0, log_alpha_stddev=30.0, log_penalty_temperature=1.5)
DUALS_REF = dict(log_temperature=10.0, log_alpha_mean=10.0, log_alpha_stddev=1000.0, log_penalty_temperature=10.0)


def _mpo_inputs(N, B, D, delta=1e-1, q_kind='n3', seed=0):
    g = torch.Generator().manual_seed(1000*seed + 7*N + 3*B + D)
    rn = lambda *s: torch.randn(*s, generator=g)
    tm = rn(B, D)*0.3; ts = torch.rand(B, D, generator=g)*0.5 + 0.2
    om = tm + math.sqrt(2*EPS['epsilon_mean'])*ts*rn(B, D)                    # mean KL (tm - om)^2 / (2 ts^2) ~ epsilon_mean per dimension
    os_ = ts.clone() if delta == 0 else (ts*(1 + delta*rn(B, D))).abs()
    acts = tm[None] + ts[None]*rn(N, B, D)
    if q_kind == 'n3':
        q = rn(N, B)*3
    else:                                                                       # 'q150': q / T - max cancels; one row with equal samples
        q = 150 + rn(N, B); q[:, B//2] = 150.25
    return om, os_, tm, ts, acts, q


def _mpo_duals(D, init, seed=0):
    g = torch.Generator().manual_seed(seed)
    if init == 'below':                                                         # every dual below the projection's floor
        return dict(log_temperature=torch.tensor([-19.5]), log_alpha_mean=-18.5 - 5*torch.rand(D, generator=g),
                    log_alpha_stddev=-18.001 - 30*torch.rand(D, generator=g), log_penalty_temperature=torch.tensor([-1000.0]))
    jit = lambda n: 0.25*torch.randn(n, generator=g)
    d = {k: torch.full((1 if 'temperature' in k else D,), float(v)) for k, v in init.items()}
    return {k: v + (jit(v.numel()) if float(v[0]) < 100 else 0) for k, v in d.items()}


def _mpo_kernel(inp, duals, penal):
    from flybody_amd.dmpo import MPOLoss, fused
    from flybody_amd.dmpo.losses import PenalizationCostRealActions
    om, os_, tm, ts, acts, q = _gpu(*inp)
    D = om.shape[1]
    cost = PenalizationCostRealActions(penal[2], penal[3], DEV) if isinstance(penal, tuple) else None
    if cost is not None:                                           # (scale, offset, minimum, maximum): the references read the first two
        assert torch.equal(cost.scale.cpu(), penal[0]) and torch.equal(cost.offset.cpu(), penal[1])
    m = MPOLoss(D, action_penalization=penal is not None, penalization_cost=cost, **EPS).to(DEV)
    with torch.no_grad():
        for k, v in duals.items():
            getattr(m, k).copy_(v)
    st, g_om, g_os, gd = fused.mpo_loss_grad(m, om, os_, tm, ts, acts, q)
    torch.cuda.synchronize()
    out = dict(stats=st[:18].clone(), d_online_mean=g_om, d_online_std=g_os)
    for k in duals:
        out[k] = getattr(m, k).detach().clone(); out['d_' + k] = gd[getattr(m, k)].clone()
    return out


def _penal(D, kind):
    if kind == 'off':
        return None
    if kind == 'norm':
        return 'norm'
    lo = -np.abs(np.random.default_rng(0).normal(size=D)).astype(np.float32) - 0.2; hi = (-lo*1.3).astype(np.float32)     # unequal ranges
    return (torch.from_numpy(hi - lo), torch.from_numpy(lo), lo, hi)


def _mpo_compare(ck, inp, duals, penal):
    """Every output of fbl_mpo_loss against the references; returns (kernel, float64, float32) result dicts."""
    got = _mpo_kernel(inp, duals, penal)
    r64 = R.mpo_loss(*inp, duals, EPS, penal, F64); r32 = R.mpo_loss(*inp, duals, EPS, penal, F32)
    s64 = r64['stats']
    # the loss is a sum of six parts, loss_alpha a sum over D of alpha (eps - KL) terms of either sign: their scale is the sum of magnitudes
    am = R.softplus(r64['log_alpha_mean']) + R.FEPS; as_ = R.softplus(r64['log_alpha_stddev']) + R.FEPS
    alpha_terms = float((am*(EPS['epsilon_mean'] + r64['kl_mean'])).sum() + (as_*(EPS['epsilon_stddev'] + r64['kl_std'])).sum())
    parts = float(s64[1:5].abs().sum() + s64[6].abs()) + alpha_terms
    for i, name in enumerate(R.STAT_NAMES):
        if name == 'penalty_kl_q_rel' and penal is None:
            continue
        # (and the non-parametric KLs are sums over the samples of w log(N w), terms of either sign)
        scale = {'loss': parts, 'loss_alpha': alpha_terms, 'kl_q_rel': float(r64['kl_q_terms']), 'penalty_kl_q_rel': float(r64['kl_p_terms'])}.get(name)
        ck.check(name, got['stats'][i], s64[i], r32['stats'][i], scale=scale)
    for k in ('d_online_mean', 'd_online_std', 'd_log_temperature', 'd_log_alpha_mean', 'd_log_alpha_stddev') + (('d_log_penalty_temperature',) if penal is not None else ()):
        ck.check(k, got[k], r64[k], r32[k])
    for k in duals:
        if k == 'log_penalty_temperature' and penal is None:
            continue
        assert torch.equal(got[k].cpu(), duals[k].clamp(min=R.MIN_LOG)), k            # the projection is written back, exactly
    return got, r64, r32


@pytest.mark.parametrize('penal', ['off', 'ranges', 'norm'])
@pytest.mark.parametrize('N,B,D', [(1, 1, 1), (32, 37, 64), (3, 9, 5), (20, 8, 3), (20, 256, 59)])
def test_mpo_loss_shapes(N, B, D, penal):
    """N at 1 / MAXN, D at 1 / a full wave, B off the 8 rows of a workgroup, N < D and D < N; penalization off, with unequal real-action
    ranges, and with the kernel's default scale 2 / offset -1 (penalization_cost=None)."""
    ck = Checker('mpo %s %s' % ((N, B, D), penal))
    _mpo_compare(ck, _mpo_inputs(N, B, D), _mpo_duals(D, DUALS_SMALL), _penal(D, penal))
    ck.done()


@pytest.mark.parametrize('init', ['small', 'reference'])
@pytest.mark.parametrize('delta', [1e-1, 1e-3, 3e-4, 1e-4, 0.0])
def test_mpo_loss_at_the_stddev_constraint(delta, init):
    """The operating point epsilon_stddev = 1e-7 holds the policy at: online stddev within delta of the target's.  CONDITION 1: at delta = 3e-4
    and 1e-4 the per-dimension batch-mean stddev KL (recovered from d_log_alpha_stddev = sigmoid (eps - KL), sigmoid == 1 at these duals) is
    within 1e-3 relative of float64, and d_log_alpha_stddev within 1e-3 epsilon_stddev.  (log(os/ts) + ts^2 / (2 os^2) - 1/2 in float32 missed
    this by a factor of 70-600; 0.5 expm1(2 d) - d reaches 3e-5 / 9e-5.)"""
    N, B, D = 20, 256, 59
    ck = Checker('mpo delta=%g %s' % (delta, init))
    inp = _mpo_inputs(N, B, D, delta=delta, seed=1)
    duals = _mpo_duals(D, DUALS_SMALL if init == 'small' else DUALS_REF, seed=1)
    got, r64, r32 = _mpo_compare(ck, inp, duals, _penal(D, 'ranges'))
    kl64 = r64['kl_std']
    # float64 may use the textbook expression: it agrees with the cancellation-free one
    assert torch.allclose(R.naive_normal_kl_std(inp[3], inp[1], F64), kl64, rtol=1e-6, atol=1e-16)
    km = r64['kl_mean']; assert 0.5*EPS['epsilon_mean'] < float(km.mean()) < 2*EPS['epsilon_mean']      # the mean KL sits at its constraint
    if delta == 0.0:
        assert float(kl64.abs().max()) == 0.0 and torch.equal(got['d_log_alpha_stddev'].cpu(), torch.full((D,), EPS['epsilon_stddev']))
    else:
        if delta in (3e-4, 1e-4):
            assert 1e-9 <= float(kl64.min()) and float(kl64.max()) <= 1e-6, (float(kl64.min()), float(kl64.max()))      # the regime the constraint lives in
        assert float(torch.sigmoid(r64['log_alpha_stddev'].float()).min()) == 1.0
        kl_k = EPS['epsilon_stddev'] - got['d_log_alpha_stddev'].double().cpu()
        rel = float(((kl_k - kl64).abs()/kl64).max())
        print('mpo delta=%g: per-dimension mean stddev KL %.2e .. %.2e, kernel relative error %.3e' % (delta, float(kl64.min()), float(kl64.max()), rel))
        if delta in (3e-4, 1e-4):
            ck.limit('CONDITION 1: kl_std relative', rel, 1e-3)
            ck.limit('CONDITION 1: d_log_alpha_stddev', float((got['d_log_alpha_stddev'].double().cpu() - r64['d_log_alpha_stddev']).abs().max()), 1e-3*EPS['epsilon_stddev'])
            s64 = r64['stats']
            for i in (4, 10):                                       # loss_kl_std, kl_stddev_rel follow
                ck.limit('CONDITION 1: ' + R.STAT_NAMES[i], abs(float(got['stats'][i]) - float(s64[i]))/abs(float(s64[i])), 1e-3)
    ck.done()


def test_mpo_loss_q_offset_and_equal_samples():
    """Q values 150 + N(0, 1) under a small temperature (q / T ~ 3000: q / T - max cancels) and one state whose samples all have the same Q
    (uniform weights, zero non-parametric KL)."""
    N, B, D = 20, 256, 59
    ck = Checker('mpo q150')
    inp = _mpo_inputs(N, B, D, q_kind='q150', seed=2)
    duals = _mpo_duals(D, dict(DUALS_SMALL, log_temperature=-3.0, log_penalty_temperature=-3.0), seed=2)
    got, r64, r32 = _mpo_compare(ck, inp, duals, _penal(D, 'ranges'))
    q = inp[5]; assert float(q[:, B//2].std()) == 0.0 and float(r64['stats'][15]) < 0.1 and float((q/float(r64['stats'][15])).min()) > 1000
    ck.done()


def test_mpo_loss_projects_every_dual():
    """Every log_* below -18: all four are written back as exactly -18 and the loss is the loss at -18."""
    N, B, D = 20, 37, 59
    ck = Checker('mpo duals below -18')
    duals = _mpo_duals(D, 'below')
    assert all(float(v.max()) < R.MIN_LOG for v in duals.values())
    got, r64, r32 = _mpo_compare(ck, _mpo_inputs(N, B, D, seed=3), duals, _penal(D, 'ranges'))
    for k in duals:
        assert torch.equal(got[k].cpu(), torch.full_like(duals[k], R.MIN_LOG)), k
    ck.done()


# ====================================================================================================== categorical TD loss
def _support(kind, K):
    if kind == 'uniform':
        return torch.linspace(-150, 150, K)
    if kind == 'geometric':                                                    # steps growing by 1.25 from atom to atom
        return (torch.cumsum(1.25**torch.arange(K, dtype=F64), 0) - 40.0).float()
    return torch.sort(torch.randn(K, generator=torch.Generator().manual_seed(K), dtype=F64)*40).values.float()


N_TARGET_KINDS = 6


def _td_targets(B, support, shift, g):
    """(reward, discount) per row by kind: 0 exactly on an atom (discount 0), 1 exactly vmin, 2 exactly vmax, 3 above the support,
    4 below it, 5 somewhere inside an interval with a real discount."""
    K = support.shape[0]; kind = (torch.arange(B) + shift) % N_TARGET_KINDS
    span = float(support[-1] - support[0])
    j = torch.randint(0, K, (B,), generator=g)
    r = torch.zeros(B); d = torch.zeros(B)
    r = torch.where(kind == 0, support[j], r)
    r = torch.where(kind == 1, support[0].expand(B), r); r = torch.where(kind == 2, support[-1].expand(B), r)
    r = torch.where(kind == 3, support[-1] + 0.4*span + 1.0, r); r = torch.where(kind == 4, support[0] - 0.4*span - 1.0, r)
    r = torch.where(kind == 5, torch.randn(B, generator=g)*0.05*span, r); d = torch.where(kind == 5, torch.rand(B, generator=g), d)
    return r, d, kind, j


@pytest.mark.parametrize('support', ['uniform', 'geometric', 'random'])
@pytest.mark.parametrize('N,B,K', [(1, 1, 2), (3, 7, 64), (4, 4, 51), (5, 37, 8), (20, 256, 51)])
def test_td_loss(N, B, K, support):
    """fbl_td_loss at the smallest N, B, K; waves without a head / one head per wave / two heads in one wave; a full wave of atoms; B off the
    4 rows of a workgroup -- on uniform and NON-uniform supports (the projection's per-atom 1 / (v[k+1] - v[k]) and 1 / (v[k] - v[k-1])), with
    targets exactly on an atom, exactly on either end, outside the support on both sides and inside an interval, logits of scale 2 and of scale
    30 (most p underflow, log p stays finite), with and without the biases."""
    from flybody_amd.dmpo import fused
    vals = _support(support, K)
    assert bool((vals[1:] > vals[:-1]).all())
    g = torch.Generator().manual_seed(100*N + B + K)
    seen = set(); end_atom = one_hot = underflow = 0
    for shift in range(0, N_TARGET_KINDS, min(B, N_TARGET_KINDS)):
        r, d, kind, j = _td_targets(B, vals, shift, g); seen |= set(kind.tolist())
        for scale in (2.0, 30.0):
            for with_bias in (False, True):
                ck = Checker('td %s %s shift %d scale %g bias %d' % ((N, B, K), support, shift, scale, with_bias))
                qt = torch.randn(N, B, K, generator=g)*scale; q1 = torch.randn(B, K, generator=g)*scale
                bt = torch.randn(K, generator=g) if with_bias else None; b1 = torch.randn(K, generator=g) if with_bias else None
                a64 = R.td_loss(qt, bt, q1, b1, vals, r, d, 0.99, F64); a32 = R.td_loss(qt, bt, q1, b1, vals, r, d, 0.99, F32)
                loss, sq, dlog, dbias = fused.td_loss_grad(*_gpu(q1, b1, qt, bt, vals, r, d), 0.99)
                torch.cuda.synchronize()
                ck.check('loss', loss, a64['loss'], a32['loss'])
                ck.check('sampled_q', sq, a64['sampled_q'], a32['sampled_q'], scale=float(vals.abs().max()))
                ck.check('d_logits', dlog, a64['d_logits'], a32['d_logits'], key='td d_logits')
                ck.check('d_bias', dbias, a64['d_bias'], a32['d_bias'], scale=float(a64['d_logits'].abs().sum(0).max()))
                # the per-row loss through the autograd wrapper's kernel call (bias_* = None there)
                if not with_bias:
                    rows = torch.empty(B, device=DEV); sq2 = torch.empty(N, B, device=DEV); dl2 = torch.empty(B, K, device=DEV)
                    a = _gpu(qt, q1, vals, r, d)
                    fused._check(fused.lib().fbl_td_loss(a[0].data_ptr(), None, a[1].data_ptr(), None, a[2].data_ptr(), a[3].data_ptr(), a[4].data_ptr(), 0.99, N, B, K,
                                                         sq2.data_ptr(), dl2.data_ptr(), None, rows.data_ptr(), None, fused._stream()))
                    torch.cuda.synchronize()
                    ck.check('loss_rows', rows, a64['loss_rows'], a32['loss_rows'])
                    assert torch.equal(dl2, dlog) and torch.equal(sq2, sq)
                # what the inputs reached
                tgt = a64['target']
                on = kind == 0
                if bool(on.any()):
                    want = torch.nn.functional.one_hot(j[on], K).double()
                    assert float((tgt[on] - want).abs().max()) < 1e-12                          # float64: one-hot
                    x1 = (q1 + (b1 if with_bias else 0)).double()                               # (the float32 sum: what the kernel's softmax sees)
                    rec = torch.softmax(x1, -1) - B*dlog.double().cpu()                         # the kernel's target, from d_logits = (softmax - target) / B
                    assert float((rec[on] - want).abs().max()) <= 8*EPS32, float((rec[on] - want).abs().max())
                    one_hot += int(on.sum())
                ends = (kind >= 1) & (kind <= 4)
                if bool(ends.any()):
                    assert bool(((tgt[ends][:, 0] > 1 - 1e-12) | (tgt[ends][:, -1] > 1 - 1e-12)).all()); end_atom += int(ends.sum())
                if scale == 30.0 and K > 8:
                    p32 = torch.softmax(qt, -1); underflow += int((p32 == 0).sum())
                    assert bool(torch.isfinite(torch.log_softmax(qt, -1)).all())
                ck.done()
    assert seen == set(range(N_TARGET_KINDS)) and one_hot > 0 and end_atom > 0
    if K > 8:
        assert underflow > 0


# ====================================================================================================== bias + LayerNorm (+ tanh)
WIDTHS = [1, 63, 64, 65, 200, 256, 512, 1000, 1024]
ROWS = [1, 3, 5, 37]


def _ln_direct(x, bias, gamma, beta, eps, act):
    from flybody_amd.dmpo import fused
    M, W = x.shape
    y = torch.empty_like(x); xhat = torch.empty_like(x); rstd = torch.empty(M, device=x.device)
    fused._check(fused.lib().fbl_bias_ln_act(x.data_ptr(), bias.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None, 1, eps, act, M, W, y.data_ptr(), xhat.data_ptr(),
                                             rstd.data_ptr(), fused._stream()))
    return y, xhat, rstd


@pytest.mark.parametrize('W', WIDTHS)
def test_bias_layernorm_act(W):
    """Forward (y, xhat, rstd) and backward (dx, dbias, dgamma, dbeta) at widths around the 64-lane column blocks, the two exact
    instantiations (256, 512) and the guarded generic one up to its limit, row counts off LN_ROWS = 4; rows of three kinds -- randn, 1e3 + randn
    (a one-pass variance would fail), constant (xhat = 0, y = act(beta), rstd = eps^-1/2) -- with act = 0 and act = 1 (tanh), unit-scale gamma
    and a gamma that saturates a third of the tanh outputs."""
    from flybody_amd.dmpo import fused
    g = torch.Generator().manual_seed(W)
    eps = 1e-5
    bias = torch.randint(-16, 17, (W,), generator=g).float()/8                       # few-bit numbers: x + bias is exact on the constant rows
    sat_seen = unsat_seen = 0
    for M in ROWS:
        kind = torch.arange(M) % 3                                                    # 0 randn, 1 offset, 2 constant
        x = torch.randn(M, W, generator=g)
        x[kind == 1] += 1e3
        x[kind == 2] = 0.5 - bias
        dy = torch.randn(M, W, generator=g)
        for gam_scale in (1.0, 10.0):
            gamma = (torch.rand(W, generator=g) + 0.5)*gam_scale; beta = torch.randn(W, generator=g)
            for act in (0, 1):
                ck = Checker('ln W=%d M=%d gamma*%g act=%d' % (W, M, gam_scale, act))
                a64 = R.bias_ln_act(x, bias, gamma, beta, eps, act, dy, F64); a32 = R.bias_ln_act(x, bias, gamma, beta, eps, act, dy, F32)
                xg, bg, gg, beg, dyg = _gpu(x, bias, gamma, beta, dy)
                y, xhat, rstd = _ln_direct(xg, bg, gg, beg, eps, act)
                leaves = [t.clone().requires_grad_(True) for t in (xg, bg, gg, beg)]
                y2 = fused._BiasLnAct.apply(leaves[0], leaves[1], leaves[2], leaves[3], eps, act, None, True)
                y2.backward(dyg); torch.cuda.synchronize()
                assert torch.equal(y2, y)
                for k in range(3):                                                    # per row kind: an error on a randn row must not hide behind a 1e3 row
                    rows = kind == k
                    if not bool(rows.any()):
                        continue
                    tag = ' [%s rows]' % ('randn', '1e3 + randn', 'constant')[k]
                    ck.check('y' + tag, y[rows], a64['y'][rows], a32['y'][rows], key='ln y')
                    ck.check('xhat' + tag, xhat[rows], a64['xhat'][rows], a32['xhat'][rows], scale=1.0, key='ln xhat')
                    ck.check('rstd' + tag, rstd[rows], a64['rstd'][rows], a32['rstd'][rows], rel=True, key='ln rstd')
                    ck.check('dx' + tag, leaves[0].grad[rows], a64['dx'][rows], a32['dx'][rows], key='ln dx')
                dyd = dy.double()
                ck.check('dbias', leaves[1].grad, a64['dbias'], a32['dbias'], scale=float(a64['dx'].abs().sum(0).max()), key='ln dbias')
                ck.check('dgamma', leaves[2].grad, a64['dgamma'], a32['dgamma'], scale=float((dyd*a64['xhat']).abs().sum(0).max()), key='ln dgamma')
                ck.check('dbeta', leaves[3].grad, a64['dbeta'], a32['dbeta'], scale=float(dyd.abs().sum(0).max()), key='ln dbeta')
                # what the inputs reached
                if bool((kind == 2).any()):
                    c = kind == 2
                    assert float(a64['xhat'][c].abs().max()) == 0.0 and torch.allclose(a64['rstd'][c], torch.tensor(eps, dtype=F32).double().rsqrt())
                    want = a64['y'][c]; assert torch.equal(want, (torch.tanh(beta.double()) if act else beta.double()).expand_as(want))
                if act == 1 and W >= 63 and bool((kind == 0).any()):
                    y32 = a64['y'][kind == 0].float().abs()
                    frac = float((y32 == 1.0).float().mean())
                    if gam_scale == 10.0:
                        assert 0.15 < frac < 0.6, frac                               # about a third of the outputs saturate in float32, the others do not
                        sat_seen += 1
                    else:
                        assert frac < 0.05, frac
                        unsat_seen += 1
                ck.done()
    assert W < 63 or (sat_seen and unsat_seen)


@pytest.mark.parametrize('W', [65, 512, 1000])
def test_bias_layernorm_row_broadcast_addend(W):
    """x [3, 5, W] + rowadd [5, W] (period 5 over M = 15 rows), forward only."""
    from flybody_amd.dmpo import fused
    g = torch.Generator().manual_seed(W + 1)
    N, B = 3, 5
    x = torch.randn(N, B, W, generator=g); ra = torch.randn(B, W, generator=g); bias = torch.randn(W, generator=g)
    ln = torch.nn.LayerNorm(W)
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5, generator=g); ln.bias.normal_(generator=g)
    ck = Checker('ln rowadd W=%d' % W)
    a64, a32 = (R.bias_ln_act(x.view(N*B, W), bias, ln.weight, ln.bias, ln.eps, 1, None, dt, rowadd=ra) for dt in (F64, F32))
    with torch.no_grad():
        y = fused.bias_ln_tanh(x.to(DEV), bias.to(DEV), ln.to(DEV), rowadd=ra.to(DEV))
    torch.cuda.synchronize()
    assert y.shape == (N, B, W)
    ck.check('y', y.view(N*B, W), a64['y'], a32['y'], key='ln y')
    ck.done()


# ====================================================================================================== bias + ELU, and the GEMMs' ELU epilogues
def _elu_specials():
    mags = torch.logspace(-7, math.log10(20.0), 40, dtype=F64)
    return torch.cat([torch.tensor([0.0, -1e-7, -1e-6, 1e-6, -20.0, 20.0, -0.35], dtype=F64), -mags, mags]).float()


@pytest.mark.parametrize('W', WIDTHS)
def test_bias_elu(W):
    """Forward and backward of ELU(x + bias) over [-20, 20], including 0 and -1e-7 (expm1, not exp - 1), compared in RELATIVE terms."""
    from flybody_amd.dmpo import fused
    g = torch.Generator().manual_seed(W + 2)
    sp = _elu_specials()
    bias = torch.randn(W, generator=g); bias[::4] = 0.0                               # special values sit where x + bias is exact
    for M in ROWS:
        ck = Checker('elu W=%d M=%d' % (W, M))
        x = torch.randn(M, W, generator=g)*3
        slots = [(r, c) for r in range(M) for c in range(0, W, 4)]
        for i, (r, c) in enumerate(slots):
            x[r, c] = sp[i % len(sp)]
        dy = torch.randn(M, W, generator=g)
        a64 = R.bias_elu(x, bias, dy, F64); a32 = R.bias_elu(x, bias, dy, F32)
        xg = x.to(DEV).requires_grad_(True); bg = bias.to(DEV).requires_grad_(True)
        y = fused.bias_elu(xg, bg); y.backward(dy.to(DEV)); torch.cuda.synchronize()
        ck.check('y (relative)', y, a64['y'], a32['y'], rel=True, key='elu y')
        ck.check('dx', xg.grad, a64['dx'], a32['dx'], scale=float(dy.abs().max()), key='elu dx')
        ck.check('dbias', bg.grad, a64['dbias'], a32['dbias'], scale=float(a64['dx'].abs().sum(0).max()), key='elu dbias')
        z = a64['z']
        if len(slots) >= len(sp):
            m7 = float(torch.tensor(-1e-7, dtype=F32))
            assert bool((z == 0).any()) and bool((z == m7).any()) and float(z.min()) <= -20 and float(z.max()) >= 20
        ck.done()


def _epilogue_problem(K, N, M, g):
    """A 0/1 selection matrix x [M, K] (row i selects k = i mod K) and weights / bias such that the pre-activation of output (i, j) is
    w[j, i mod K] + b[j]: one float32 addition, exact in the matrix core (every other product is 0)."""
    mags = torch.logspace(-6, math.log10(20.0), (K*N)//2 + 1, dtype=F64)
    z = torch.cat([mags, -mags])[:K*N]
    z[:8] = torch.tensor([0.0, -0.35, -0.3500001, -0.3499999, -1e-6, 1e-6, -20.0, 20.0], dtype=F64)
    z = z[torch.randperm(K*N, generator=g)].view(N, K)
    b = torch.randint(-8, 9, (N,), generator=g).double()/8; b[::2] = 0.0
    w = (z - b[:, None]).float(); b = b.float()
    x = torch.zeros(M, K); x[torch.arange(M), torch.arange(M) % K] = 1.0
    z64 = (w.double() + b.double()[:, None]).T[torch.arange(M) % K]                 # [M, N]
    z32 = (w + b[:, None]).T[torch.arange(M) % K]
    return x, w, b, z64, z32


@pytest.mark.parametrize('kernel', ['sgemm', 'gemm_nt', 'policy_tail'])
def test_gemm_elu_epilogues(kernel):
    """The ELU epilogues of fbl_sgemm (library expm1), fbl_gemm_nt (polynomial elu_f with its switch at -0.35) and fbl_policy_tail, isolated
    from the product: relative error down to |z| = 1e-6."""
    from flybody_amd.dmpo import fused
    g = torch.Generator().manual_seed(5)
    ck = Checker('elu epilogue ' + kernel)
    if kernel == 'policy_tail':
        K = N = 256; M = 300
    else:
        K, N, M = 8, 70, 45
    x, w, b, z64, z32 = _epilogue_problem(K, N, M, g)
    xg, wg, bg = _gpu(x, w, b)
    if kernel == 'sgemm':
        y = fused._sgemm(xg, K, 1, wg, 1, K, M, N, K, 2, bg)
    elif kernel == 'gemm_nt':
        y = fused.gemm_nt(xg, wg, bg, 2)
    else:
        D = 3
        w3 = torch.zeros(256, 256, device=DEV); z256 = torch.zeros(256, device=DEV); wh = torch.zeros(D, 256, device=DEV); zD = torch.zeros(D, device=DEV)
        y = torch.empty(M, 256, device=DEV); h3 = torch.empty(M, 256, device=DEV); mean = torch.empty(M, D, device=DEV); std = torch.empty(M, D, device=DEV)
        fused._check(fused.lib().fbl_policy_tail(xg.data_ptr(), M, 256, wg.data_ptr(), bg.data_ptr(), w3.data_ptr(), z256.data_ptr(), wh.data_ptr(), zD.data_ptr(),
                                                 wh.data_ptr(), zD.data_ptr(), D, 1.0, 1e-6, y.data_ptr(), h3.data_ptr(), mean.data_ptr(), std.data_ptr(), fused._stream()))
    torch.cuda.synchronize()
    assert y.shape == (M, N)
    ck.check('y (relative)', y, R.elu(z64), R.elu(z32), rel=True, key='epilogue ' + kernel)
    az = z64.abs()
    assert float(az[az > 0].min()) <= 1.1e-6 and bool((z64 == 0).any()) and float(az.max()) >= 20 and bool(((z64 < -0.3499) & (z64 > -0.3501)).any())
    ck.done()


# ====================================================================================================== Gaussian head
MUL, MIN_SCALE = 0.7/math.log(2.0), 1e-6


def _head_grid(M, D, g):
    """Pre-activations over [-16, 25] with 20 and the next float above it (softplus_f's switch), as zs + bs with the special values where bs = 0."""
    bs = torch.randint(-8, 9, (D,), generator=g).float()/4; bs[::4] = 0.0
    z = torch.linspace(-16, 25, M*D, dtype=F64)[torch.randperm(M*D, generator=g)].float().view(M, D)
    nxt = float(np.nextafter(np.float32(20.0), np.float32(30.0)))
    sp = [-16.0, 20.0, nxt, 25.0, 4.0, 0.0]
    slots = [(r, c) for r in range(M) for c in range(0, D, 4)]
    for (r, c), v in zip(slots, sp):
        z[r, c] = v
    return (z - bs).float(), bs


@pytest.mark.parametrize('M,D', [(1, 1), (5, 59), (6, 256)])
def test_gaussian_head(M, D):
    """fbl_gauss_head and BOTH backward kernels (from zs; from the stddev) at one row / rows off GH_ROWS = 4 / the 256-column limit.  d zs is
    compared RELATIVELY.  CONDITION 2: d zs from fbl_gauss_head_bwd_std within 1e-5 relative for pre-activations in [-16, 4] (1 - exp(-s)
    was off by up to 0.2 there; -expm1(-s) reaches 8e-7)."""
    from flybody_amd.dmpo import fused
    g = torch.Generator().manual_seed(M*D)
    ck = Checker('gauss head %s' % ((M, D),))
    zs, bs = _head_grid(M, D, g)
    zm = torch.randn(M, D, generator=g); bm = torch.randn(D, generator=g)
    dmean = torch.randn(M, D, generator=g); dstd = torch.randn(M, D, generator=g); dstd[dstd.abs() < 1e-3] = 0.5
    a64, a32 = (R.gauss_head(zm, zs, bm, bs, MUL, MIN_SCALE, dmean, dstd, dt) for dt in (F64, F32))
    s32 = R.gauss_head(zm, zs, bm, bs, MUL, MIN_SCALE, dmean, dstd, F32, from_std=True)
    leaves = [t.to(DEV).requires_grad_(True) for t in (zm, zs, bm, bs)]
    mean, std = fused.gauss_head(leaves[0], leaves[1], leaves[2], leaves[3], MUL, MIN_SCALE)
    (mean*dmean.to(DEV) + std*dstd.to(DEV)).sum().backward(); torch.cuda.synchronize()
    ck.check('mean', mean, a64['mean'], a32['mean'])
    ck.check('std (relative)', std, a64['std'], a32['std'], rel=True, key='head std')
    assert torch.equal(leaves[0].grad.cpu(), dmean)
    ck.check('dzs from zs (relative)', leaves[1].grad, a64['dzs'], a32['dzs'], rel=True, key='head dzs')
    col = float(a64['dzs'].abs().sum(0).max())
    ck.check('dbm', leaves[2].grad, a64['dbm'], a32['dbm'], scale=float(dmean.abs().sum(0).max()))
    ck.check('dbs', leaves[3].grad, a64['dbs'], a32['dbs'], scale=col)
    # from the stddev the forward kernel produced
    dzs = torch.empty(M, D, device=DEV); db = torch.zeros(2, D, device=DEV)
    stdc = std.detach().contiguous(); dmg = dmean.to(DEV); dsg = dstd.to(DEV)
    fused._check(fused.lib().fbl_gauss_head_bwd_std(dmg.data_ptr(), dsg.data_ptr(), stdc.data_ptr(), MUL, MIN_SCALE, M, D, dzs.data_ptr(), db[0].data_ptr(),
                                                    db[1].data_ptr(), fused._stream()))
    torch.cuda.synchronize()
    ck.check('dzs from std (relative)', dzs, a64['dzs'], s32['dzs'], rel=True, key='head dzs from std')
    ck.check('dbm (std)', db[0], a64['dbm'], s32['dbm'], scale=float(dmean.abs().sum(0).max()))
    ck.check('dbs (std)', db[1], a64['dbs'], s32['dbs'], scale=col)
    z = (zs.double() + bs.double())
    low = (z >= -16) & (z <= 4)
    rel = ((dzs.double().cpu() - a64['dzs']).abs()/a64['dzs'].abs())[low]
    ck.limit('CONDITION 2: dzs from std, z in [-16, 4]', float(rel.max()), 1e-5)
    if M*D > 6:
        nxt = float(np.nextafter(np.float32(20.0), np.float32(30.0)))
        assert bool((z == 20.0).any()) and bool((z == nxt).any()) and float(z.min()) <= -15.99 and float(z.max()) >= 24.99 and int((z < -12).sum()) >= 5
    ck.done()


@pytest.mark.parametrize('M,K,D', [(5, 3, 1), (33, 9, 64), (37, 203, 45), (256, 256, 59)])
def test_gaussian_head_linear(M, K, D):
    """fbl_sgemm_pair's head epilogues (+ bias | softplus(. + bias) mul + min) and the head's backward (weight gradients in one launch, the
    summed input gradient in one launch) at ragged shapes, against float64 with the GEMM tolerance of this project."""
    from flybody_amd.dmpo import fused
    g = torch.Generator().manual_seed(M + K + D)
    ck = Checker('head linear %s' % ((M, K, D),))
    h = torch.randn(M, K, generator=g); wm = torch.randn(D, K, generator=g)/math.sqrt(K); ws = torch.randn(D, K, generator=g)*3/math.sqrt(K)
    bm = torch.randn(D, generator=g); bs = torch.randn(D, generator=g); u1 = torch.randn(M, D, generator=g); u2 = torch.randn(M, D, generator=g)
    lg = [t.to(DEV).requires_grad_(True) for t in (h, wm, bm, ws, bs)]
    mean, std = fused.gauss_head_linear(*lg, MUL, MIN_SCALE)
    (mean*u1.to(DEV) + std*u2.to(DEV)).sum().backward(); torch.cuda.synchronize()
    ld = [t.double().requires_grad_(True) for t in (h, wm, bm, ws, bs)]
    mr = ld[0] @ ld[1].T + ld[2]; sr = R.softplus(ld[0] @ ld[3].T + ld[4])*MUL + MIN_SCALE
    (mr*u1.double() + sr*u2.double()).sum().backward()
    ck.close('mean', mean, mr.detach()); ck.close('std', std, sr.detach())
    for name, a, b in zip(('dh', 'dwm', 'dbm', 'dws', 'dbs'), lg, ld):
        ck.close(name, a.grad, b.grad, atol=2e-5 if name == 'dh' else 2e-4)         # (reductions over the M rows: the atol of test_small_mfma_gemm's d W)
    ck.done()


# ====================================================================================================== clipped, floored, segmented Adam; the flat gather
def _adam_case(name):
    """(tensor sizes, tensors per segment, lrs, clips, floors, gradient scale per segment)."""
    if name == 'n3':
        return [1, 2], [1, 1], [1e-3, 1e-2], [0.5, 0.0], [None, -0.25], [1.0, 1.0]
    if name == 'n5':
        return [5], [1], [1e-3], [0.1], [None], [1.0]
    if name == 'segments8':
        sizes = [5, 1, 1, 131, 600, 423, 1025, 3, 514, 63, 2]
        per = [1, 1, 1, 2, 1, 1, 2, 2]
        #        clipped   len 1   zero grad  unclipped  no clip  floor    clipped   unclipped
        return sizes, per, [1e-3, 1e-2, 1e-3, 1e-4, 1e-3, 1e-2, 1e-3, 1e-3], [0.5, 40.0, 1.0, 1e4, 0.0, 0.0, 2.0, 1e3], \
            [None, None, None, None, None, -0.5, -18.0, None], [1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.01]
    if name == 'second_iteration':                                # more than 4096 workgroups x 256 threads x 4 elements: the grid-stride loop goes round again
        return [4096*1024 - 5, 1032], [1, 1], [1e-4, 1e-3], [40.0, 0.0], [None, -0.5], [0.01, 1.0]
    raise KeyError(name)


@pytest.mark.parametrize('norms_ready', [0, 1])
@pytest.mark.parametrize('case', ['n3', 'n5', 'segments8', 'second_iteration'])
def test_flat_adam(case, norms_ready):
    """Six updates of fbl_adam against float64 Adam, the squared group norms from its own pass (norms_ready 0: k_sqnorm) and from
    fbl_gather_flat (norms_ready 1): tail only (n = 3), n = 5, eight segments with odd boundaries -- clipped, unclipped, zero-gradient,
    clip = 0, a binding floor, all in one update -- and a size at which k_adam's grid-stride loop takes a second iteration."""
    from flybody_amd.dmpo.fused import FlatAdam
    sizes, per, lrs, clips, floors, gscale = _adam_case(case)
    g = torch.Generator().manual_seed(len(sizes) + norms_ready)
    n = sum(sizes); seg_sizes = []; i = 0
    for k in per:
        seg_sizes.append(sum(sizes[i:i + k])); i += k
    ends = list(np.cumsum(seg_sizes))
    assert n == ends[-1] and (case != 'segments8' or (all(e % 4 for e in ends[:-1]) and 1 in seg_sizes and len(ends) == 8))
    assert case != 'second_iteration' or n == 4096*1024 + 1027
    p0 = torch.randn(n, generator=g)
    opt = FlatAdam(p0.clone().to(DEV), torch.zeros(n, device=DEV), seg_sizes, lrs, clips, floors)
    opt.set_layout(sizes)
    a64 = R.Adam(p0, ends, lrs, clips, floors, F64); a32 = R.Adam(p0, ends, lrs, clips, floors, F32)
    seg_of = torch.repeat_interleave(torch.arange(len(ends)), torch.tensor(seg_sizes))
    bound_floor = 0
    ck = Checker('adam %s norms_ready=%d' % (case, norms_ready))
    for step in range(6):
        grad = torch.randn(n, generator=g)*torch.tensor(gscale)[seg_of]*(3.0 if step % 2 else 1.0)
        if norms_ready:
            parts = [t.clone().to(DEV) for t in torch.split(grad, sizes)]
            opt.set_grads(parts, with_norms=True)
        else:
            opt.g.copy_(grad.to(DEV))
        opt.step(); a64.step(grad); a32.step(grad)
        fl = torch.tensor([(-math.inf if f is None else f) for f in floors], dtype=F64)[seg_of]
        bound_floor += int((a64.p == fl).sum())
    torch.cuda.synchronize()
    assert int(opt.step_t[0]) == 6 and torch.equal(opt.g.cpu(), grad)
    ck.check('param', opt.p, a64.p, a32.p); ck.check('exp_avg', opt.m, a64.m, a32.m); ck.check('exp_avg_sq', opt.v, a64.v, a32.v)
    # per segment as well: a small segment must not hide behind a large one
    lo = 0
    for s, hi in enumerate(ends):
        if len(ends) > 1:
            ck.check('param seg %d' % s, opt.p[lo:hi], a64.p[lo:hi], a32.p[lo:hi], key='param')
            ck.check('exp_avg_sq seg %d' % s, opt.v[lo:hi], a64.v[lo:hi], a32.v[lo:hi], key='exp_avg_sq')
        lo = hi
    # what the updates reached
    fl = np.array(a64.clipped)                                   # [step][segment]
    if case == 'segments8':
        one = fl[0]
        assert one[0] and one[6] and not one[3] and not one[7] and not one[4], one       # clipped and unclipped segments in ONE update
        assert float(a64.v[ends[1]:ends[2]].abs().max()) == 0.0 and torch.equal(a64.p[ends[1]:ends[2]], p0[ends[1]:ends[2]].double())    # the zero-gradient segment stands still
    if any(f is not None for f in floors) and case != 'n3':
        assert bound_floor > 0
    if case in ('segments8', 'second_iteration', 'n5'):
        assert fl.any()
    ck.done()


def test_gather_flat_many_tensors():
    """fbl_gather_flat with the most tensors it takes (96), sizes around the 1024-element chunk so that chunks lie inside one tensor, end with
    one, and straddle many; a missing gradient in the middle and one as the LAST tensor: the flat buffer is bit-equal to the concatenation,
    the squared group norms match float64 -- and a segment end that is not a tensor end is refused."""
    from flybody_amd.dmpo import fused
    from flybody_amd.dmpo.fused import FlatAdam
    g = torch.Generator().manual_seed(96)
    pool = [1, 3, 7, 1023, 1024, 1025, 2, 2053, 300, 64, 4096, 5]
    sizes = [pool[(5*i + i//12) % len(pool)] for i in range(96)]
    assert len(sizes) == 96 and {1, 1023, 1024, 1025} <= set(sizes)
    per = [10, 1, 30, 7, 20, 8, 19, 1]; assert sum(per) == 96
    seg_sizes = []; i = 0
    for k in per:
        seg_sizes.append(sum(sizes[i:i + k])); i += k
    n = sum(sizes); ends = list(np.cumsum(seg_sizes))
    ck = Checker('gather 96')
    for rnd in range(2):
        opt = FlatAdam(torch.zeros(n, device=DEV), torch.full((n,), 7.0, device=DEV), seg_sizes, [1e-3]*8, [1.0]*8)
        opt.set_layout(sizes)
        grads = [torch.randn(s, generator=g)*(10.0**((i % 5) - 2)) for i, s in enumerate(sizes)]
        missing = (41, 95) if rnd == 0 else (0, 10)
        dev_grads = [None if i in missing else t.to(DEV) for i, t in enumerate(grads)]
        opt.set_grads(dev_grads, with_norms=True); torch.cuda.synchronize()
        want = torch.cat([torch.zeros(s) if i in missing else t for i, (t, s) in enumerate(zip(grads, sizes))])
        assert torch.equal(opt.g.cpu(), want)
        norms = opt._norms.view(2, 32, 8)                                          # [parity][slot][segment] (include/flybody_learner.h)
        assert float(norms[1].abs().max()) == 0.0 and int(opt.step_t[1]) == 1 and int(opt.step_t[0]) == 0
        n64 = R.segment_sqnorms(want, ends, F64); n32 = R.segment_sqnorms(want, ends, F32)
        for s in range(8):
            ck.check('sqnorm seg %d (relative)' % s, norms[0, :, s].double().sum(), n64[s], n32[s], rel=True, key='sqnorm')
    # a segment end inside a tensor: the chunk that holds it would be attributed to one segment only
    bad = FlatAdam(torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), [seg_sizes[0] + 1, seg_sizes[1] - 1] + seg_sizes[2:], [1e-3]*8, [1.0]*8)
    bad.set_layout(sizes)
    with pytest.raises(fused.LearnerLibError, match='segment end'):
        bad.set_grads(dev_grads, with_norms=True)
    bad.set_grads(dev_grads, with_norms=False)                                     # without the norm pass the segments are not read: a plain gather
    torch.cuda.synchronize()
    ck.done()
