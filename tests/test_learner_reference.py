"""CPU checks that go with tests/test_gpu_learner_fp64.py: the package's own float32 MPO loss at the stddev constraint's operating point
against itself in float64, and the float64 references of tests/learner_fp64.py against the package's CPU definitions (dmpo/losses.py,
torch.nn.functional) in float64 -- two statements of the same formulas, written independently, must agree to float64 rounding."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import learner_fp64 as R

F32, F64 = torch.float32, torch.float64
EPS = dict(epsilon=0.1, epsilon_penalty=0.1, epsilon_mean=0.0025, epsilon_stddev=1e-7)


def _mpo_problem(N, B, D, delta, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    tm = rn(B, D)*0.3; ts = torch.rand(B, D, generator=g)*0.5 + 0.2
    om = tm + 0.07*ts*rn(B, D); os_ = (ts*(1 + delta*rn(B, D))).abs()
    acts = tm[None] + ts[None]*rn(N, B, D); q = rn(N, B)*3
    return om, os_, tm, ts, acts, q


@pytest.mark.parametrize('delta', [3e-4, 1e-4])
def test_mpo_loss_float32_keeps_the_stddev_kl_at_its_constraint(delta):
    """epsilon_stddev = 1e-7 holds the online stddev within ~3e-4 of the target's, where the KL is ~1e-7 .. 1e-8.  MPOLoss in float32 must
    keep the per-dimension batch-mean stddev KL within 1e-3 relative of the same module in float64 (B = 256), and with it the dual gradient
    sigmoid (eps - KL) within 1e-3 eps and the statistics built from it.  (The textbook expression log(s1/s0) + s0^2 / (2 s1^2) - 1/2 is off
    by 7e-2 resp. 0.65 here.)"""
    from flybody_amd.dmpo import MPOLoss
    N, B, D = 20, 256, 59
    inp = _mpo_problem(N, B, D, delta, seed=int(delta*1e5))
    m32 = MPOLoss(D, init_log_temperature=1.5, init_log_alpha_mean=2.0, init_log_alpha_stddev=30.0, action_penalization=False, **EPS)
    m64 = copy.deepcopy(m32).double()
    out = {}
    for m, dt in ((m32, F32), (m64, F64)):
        loss, st = m(*(t.to(dt) for t in inp)); loss.backward()
        out[dt] = (m.log_alpha_stddev.grad.double(), {k: float(v.detach()) for k, v in st.items()})
    g32, s32 = out[F32]; g64, s64 = out[F64]
    kl64 = EPS['epsilon_stddev'] - g64; kl32 = EPS['epsilon_stddev'] - g32                # sigmoid(30) == 1 in both formats
    assert 1e-9 < float(kl64.min()) and float(kl64.max()) < 1e-6
    rel = float(((kl32 - kl64).abs()/kl64).max())
    print('delta %g: mean stddev KL %.2e .. %.2e, float32 relative error %.2e' % (delta, float(kl64.min()), float(kl64.max()), rel))
    assert rel <= 1e-3, rel
    assert float((g32 - g64).abs().max()) <= 1e-3*EPS['epsilon_stddev']
    assert abs(s32['kl_stddev_rel'] - s64['kl_stddev_rel']) <= 1e-3*abs(s64['kl_stddev_rel'])


def test_normal_kl_is_the_textbook_expression():
    from flybody_amd.dmpo.losses import _normal_kl
    g = torch.Generator().manual_seed(0)
    m0, m1 = torch.randn(2, 500, generator=g, dtype=F64); s0, s1 = torch.rand(2, 500, generator=g, dtype=F64) + 0.1
    want = torch.log(s1/s0) + (s0*s0 + (m0 - m1)**2)/(2*s1*s1) - 0.5
    assert torch.allclose(_normal_kl(m0, s0, m1, s1), want, rtol=1e-11, atol=1e-14)
    assert float(_normal_kl(m0, s0, m0, s0).abs().max()) == 0.0


@pytest.mark.parametrize('penal', ['off', 'norm', 'ranges'])
def test_reference_mpo_loss_equals_the_cpu_definition_in_float64(penal):
    from flybody_amd.dmpo import MPOLoss
    from flybody_amd.dmpo.losses import PenalizationCostRealActions
    N, B, D = 7, 13, 5
    inp = _mpo_problem(N, B, D, 0.1, seed=4)
    lo = -np.abs(np.random.default_rng(0).normal(size=D)).astype(np.float32) - 0.2; hi = (-lo*1.3).astype(np.float32)
    cost = PenalizationCostRealActions(lo, hi) if penal == 'ranges' else None
    m = MPOLoss(D, init_log_temperature=1.5, init_log_alpha_mean=2.0, init_log_alpha_stddev=3.0, action_penalization=penal != 'off',
                penalization_cost=cost, **EPS)
    with torch.no_grad():
        m.log_alpha_mean[0] = -30.0; m.log_alpha_stddev[1] = -19.0                        # two duals below the projection's floor
    duals = {k: getattr(m, k).detach().clone() for k in ('log_temperature', 'log_alpha_mean', 'log_alpha_stddev', 'log_penalty_temperature')}
    m = m.double()
    if cost is not None:
        cost.scale = cost.scale.double(); cost.offset = cost.offset.double()
    om, os_ = inp[0].double().requires_grad_(True), inp[1].double().requires_grad_(True)
    loss, st = m(om, os_, *(t.double() for t in inp[2:])); loss.backward()
    r = R.mpo_loss(*inp, duals, EPS, None if penal == 'off' else 'norm' if penal == 'norm' else (torch.from_numpy(hi - lo), torch.from_numpy(lo)), F64)
    close = lambda a, b: torch.allclose(torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64), rtol=1e-10, atol=1e-13)
    names = dict(loss='loss_policy', loss_alpha='loss_alpha', loss_temperature='loss_temperature', kl_q_rel='kl_q_rel', kl_mean_rel='kl_mean_rel',
                 kl_stddev_rel='kl_stddev_rel', q_min='q_min', q_max='q_max', pi_stddev_min='pi_stddev_min', pi_stddev_max='pi_stddev_max',
                 temperature='dual_temperature', alpha_mean='dual_alpha_mean', alpha_stddev='dual_alpha_stddev')
    if penal != 'off':
        names['penalty_kl_q_rel'] = 'penalty_kl_q_rel'
    for mine, theirs in names.items():
        assert close(r['stats'][R.STAT_NAMES.index(mine)], st[theirs]), mine
    assert close(r['d_online_mean'], om.grad) and close(r['d_online_std'], os_.grad)
    for k in duals:
        assert torch.equal(r[k], getattr(m, k).detach()) and float(r[k].min()) >= R.MIN_LOG, k
        if k != 'log_penalty_temperature' or penal != 'off':
            assert close(r['d_' + k], getattr(m, k).grad), k


@pytest.mark.parametrize('support', ['uniform', 'random'])
def test_reference_td_loss_equals_the_cpu_definition_in_float64(support):
    from flybody_amd.dmpo.losses import categorical_td_loss
    g = torch.Generator().manual_seed(1)
    N, B, K = 3, 11, 9
    vals = torch.linspace(-10, 10, K) if support == 'uniform' else torch.sort(torch.randn(K, generator=g)*5).values
    qt = torch.randn(N, B, K, generator=g)*2; q1 = torch.randn(B, K, generator=g)*2; bt = torch.randn(K, generator=g); b1 = torch.randn(K, generator=g)
    r = torch.randn(B, generator=g)*8; d = torch.rand(B, generator=g); d[0] = 0.0; r[0] = vals[3]; r[1] = 100.0; r[2] = -100.0
    a = R.td_loss(qt, bt, q1, b1, vals, r, d, 0.99, F64)
    x1 = q1.double().requires_grad_(True); bb = b1.double().requires_grad_(True)
    avg = torch.logsumexp(torch.log_softmax(qt.double() + bt.double(), -1), 0)
    gam = torch.tensor(0.99, dtype=F32).double()
    rows = categorical_td_loss(x1 + bb, vals.double(), r.double(), gam*d.double(), avg); rows.mean().backward()
    assert torch.allclose(a['loss_rows'], rows.detach(), rtol=1e-12, atol=1e-13)
    assert torch.allclose(a['d_logits'], x1.grad, rtol=1e-10, atol=1e-14) and torch.allclose(a['d_bias'], bb.grad, rtol=1e-10, atol=1e-14)
    assert torch.allclose(a['sampled_q'], (torch.softmax(qt.double() + bt.double(), -1)*vals.double()).sum(-1), rtol=1e-12, atol=1e-13)
    onehot = torch.zeros(K, dtype=F64); onehot[3] = 1.0
    assert torch.allclose(a['target'][0], onehot, atol=1e-14) and abs(float(a['target'][1, -1]) - 1) < 1e-14 and abs(float(a['target'][2, 0]) - 1) < 1e-14


def test_reference_layers_and_adam_equal_torch_in_float64():
    g = torch.Generator().manual_seed(2)
    M, W = 5, 37
    x = torch.randn(M, W, generator=g); b = torch.randn(W, generator=g); gam = torch.rand(W, generator=g) + 0.5; be = torch.randn(W, generator=g)
    dy = torch.randn(M, W, generator=g)
    a = R.bias_ln_act(x, b, gam, be, 1e-5, 1, dy, F64)
    xd, bd, gd, bed = (t.double().requires_grad_(True) for t in (x, b, gam, be))
    eps = float(torch.tensor(1e-5, dtype=F32).double())
    y = torch.tanh(F.layer_norm(xd + bd, (W,), gd, bed, eps)); y.backward(dy.double())
    for k, t in (('y', y.detach()), ('dx', xd.grad), ('dbias', bd.grad), ('dgamma', gd.grad), ('dbeta', bed.grad)):
        assert torch.allclose(a[k], t, rtol=1e-10, atol=1e-13), k
    x3 = x*3
    e = R.bias_elu(x3, b, dy, F64)
    zd = (x3.double() + b.double()).requires_grad_(True); F.elu(zd).backward(dy.double())
    assert torch.allclose(e['y'], F.elu(zd).detach(), rtol=1e-12, atol=1e-15) and torch.allclose(e['dx'], zd.grad, rtol=1e-12, atol=1e-15)
    # Adam: torch.optim.Adam with clip_grad_norm_ in float64, two segments
    n0, n1 = 7, 12
    p0 = torch.randn(n0 + n1, generator=g)
    ref = R.Adam(p0, [n0, n0 + n1], [1e-3, 1e-2], [0.5, 0.0], [None, None], F64)
    pa = p0[:n0].double().clone().requires_grad_(True); pb = p0[n0:].double().clone().requires_grad_(True)
    f32 = lambda v: float(torch.tensor(v, dtype=F32).double())
    opt = torch.optim.Adam([dict(params=[pa], lr=f32(1e-3)), dict(params=[pb], lr=f32(1e-2))], betas=(f32(0.9), f32(0.999)), eps=f32(1e-8))
    for _ in range(4):
        grad = torch.randn(n0 + n1, generator=g)
        pa.grad = grad[:n0].double().clone(); pb.grad = grad[n0:].double().clone()
        torch.nn.utils.clip_grad_norm_([pa], 0.5)
        opt.step(); ref.step(grad)
    assert torch.allclose(ref.p, torch.cat([pa, pb]).detach(), rtol=1e-9, atol=1e-12)
    assert ref.clipped[0] == [True, False]
