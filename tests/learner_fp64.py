"""Plain CPU-torch restatements of the operations behind the learner's loss, layer and optimizer kernels (include/flybody_learner.h),
written from the formulas -- nothing here calls dmpo/losses.py or dmpo/fused.py.  Every function takes float32 inputs and a `dtype`:
torch.float64 is the reference the kernels are checked against (tests/test_gpu_learner_fp64.py); torch.float32 is the SAME text
evaluated in the kernels' number format -- the cancellation-free forms are used where they matter, so its distance to the float64
result (`err_ref`) is what float32 can deliver for that quantity on those inputs.  Gradients come from autograd in `dtype`.
Test infrastructure only."""
from __future__ import annotations

import math

import torch

MIN_LOG = -18.0
FEPS = 1e-8
EPS32 = 2.0**-23                  # one ulp of 1.0 in float32


def _c(t, dtype):
    return None if t is None else t.detach().cpu().to(dtype)


def softplus(x):
    return torch.logaddexp(x, torch.zeros_like(x))


# ------------------------------------------------------------------ MPO loss (losses_mpo.py MPO.__call__, decoupled, per-dimension duals)
STAT_NAMES = ['loss', 'loss_policy_mean', 'loss_policy_std', 'loss_kl_mean', 'loss_kl_std', 'loss_alpha', 'loss_temperature', 'kl_q_rel',
              'penalty_kl_q_rel', 'kl_mean_rel', 'kl_stddev_rel', 'q_min', 'q_max', 'pi_stddev_min', 'pi_stddev_max', 'temperature',
              'alpha_mean', 'alpha_stddev']


def _estep(values, eps, temperature):
    """Weights over the N samples (dim 0), the temperature loss and the non-parametric KL; values are constants."""
    n = values.shape[0]
    # the row maximum is taken off BEFORE the division by T: (v - max) / T has the relative error of one subtraction, while
    # v / T - max / T loses |v / T| ulps -- with it logsumexp(v / T) = max / T + lse', and T max / T = max leaves the loss as a constant
    # (and log N goes inside the logarithm: log(mean exp) <= 0 is small where logsumexp - log N is a difference of numbers of size log N)
    vmax = values.max(0, keepdim=True).values
    w = torch.softmax((values - vmax)/temperature.detach(), 0)
    lse = torch.log(torch.exp((values - vmax)/temperature).mean(0))
    loss = temperature*(eps + lse.mean()) + vmax.mean()
    kl = (w*torch.log(n*w + 1e-8)).sum(0)
    return w, loss.sum(), kl.mean(), (w*torch.log(n*w + 1e-8)).abs().sum(0).mean()


def mpo_loss(om, os_, tm, ts, actions, q, duals, eps, penalization, dtype):
    """duals: dict log_temperature [1], log_alpha_mean [D], log_alpha_stddev [D], log_penalty_temperature [1];  eps: dict epsilon,
    epsilon_penalty, epsilon_mean, epsilon_stddev;  penalization: None (off), 'norm' (cost = -||a||) or (scale [D], offset [D])
    (cost = -||0.5 (a + 1) scale + offset||).  Returns a dict: stats [18] (STAT_NAMES), projected duals, d <dual>, d_online_mean,
    d_online_std, kl_std [D] (per-dimension batch mean of the stddev KL)."""
    om, os_, tm, ts, actions, q = (_c(t, dtype) for t in (om, os_, tm, ts, actions, q))
    om.requires_grad_(True); os_.requires_grad_(True)
    D = om.shape[-1]
    P = {k: _c(v, dtype).clamp(min=MIN_LOG).requires_grad_(True) for k, v in duals.items()}       # the projection comes first
    T = softplus(P['log_temperature']) + FEPS
    am = softplus(P['log_alpha_mean']) + FEPS
    as_ = softplus(P['log_alpha_stddev']) + FEPS
    w, loss_t, klq, klq_abs = _estep(q, eps['epsilon'], T); klp_abs = torch.zeros((), dtype=dtype)
    W = w; pen_rel = torch.zeros((), dtype=dtype)
    if penalization is not None:
        pT = softplus(P['log_penalty_temperature']) + FEPS
        real = actions if isinstance(penalization, str) else 0.5*(actions + 1.0)*_c(penalization[0], dtype) + _c(penalization[1], dtype)
        cost = -(real*real).sum(-1).sqrt()
        pw, loss_pt, klp, klp_abs = _estep(cost, eps['epsilon_penalty'], pT)
        W = w + pw; loss_t = loss_t + loss_pt; pen_rel = klp/eps['epsilon_penalty']
    W = W.detach()
    c0 = 0.5*math.log(2*math.pi)
    logp_mean = (-0.5*((actions - om)/ts)**2 - torch.log(ts) - c0).sum(-1)
    logp_std = (-0.5*((actions - tm)/os_)**2 - torch.log(os_) - c0).sum(-1)
    lpm = -(logp_mean*W).sum(0).mean(); lps = -(logp_std*W).sum(0).mean()
    kl_mean = ((tm - om)**2/(2*ts*ts)).mean(0)
    # log(os/ts) + ts^2 / (2 os^2) - 1/2 with ts / os = 1 + r: (r - log1p(r)) + r^2 / 2; r - log1p(r) = r^2 (1/2 - r/3 + r^2/4 - ...) below 1/32
    r = (ts - os_)/os_
    series = r*r*(1/2 + r*(-1/3 + r*(1/4 + r*(-1/5 + r*(1/6 + r*(-1/7 + r*(1/8 + r*(-1/9 + r/10))))))))
    kl_std = (torch.where(r.abs() < 0.03125, series, r - torch.log1p(r)) + r*r/2).mean(0)
    loss_kl_mean = (am.detach()*kl_mean).sum(); loss_kl_std = (as_.detach()*kl_std).sum()
    loss_alpha = (am*(eps['epsilon_mean'] - kl_mean.detach())).sum() + (as_*(eps['epsilon_stddev'] - kl_std.detach())).sum()
    loss = lpm + lps + loss_kl_mean + loss_kl_std + loss_alpha + loss_t
    loss.backward()
    with torch.no_grad():
        stats = torch.stack([loss, lpm, lps, loss_kl_mean, loss_kl_std, loss_alpha, loss_t, klq/eps['epsilon'], pen_rel,
                             kl_mean.sum()/(D*eps['epsilon_mean']), kl_std.sum()/(D*eps['epsilon_stddev']),
                             q.min(0).values.mean(), q.max(0).values.mean(), os_.min(-1).values.mean(), os_.max(-1).values.mean(),
                             T.sum(), am.mean(), as_.mean()]).detach()
    out = dict(stats=stats, d_online_mean=om.grad, d_online_std=os_.grad, kl_std=kl_std.detach(), kl_mean=kl_mean.detach(),
               kl_q_terms=(klq_abs/eps['epsilon']).detach(), kl_p_terms=(klp_abs/eps['epsilon_penalty']).detach())
    for k, v in P.items():
        out[k] = v.detach()
        out['d_' + k] = v.grad if v.grad is not None else torch.zeros_like(v)
    return out


def naive_normal_kl_std(ts, os_, dtype):
    """The textbook expression (accurate in float64: ~1e-8 relative at KL = 1e-8), per-dimension batch mean."""
    ts, os_ = _c(ts, dtype), _c(os_, dtype)
    return (torch.log(os_/ts) + ts*ts/(2*os_*os_) - 0.5).mean(0)


# ------------------------------------------------------------------ categorical TD loss (acme losses.categorical, N target heads)
def l2_project(z, p, support):
    """Cramer projection of the distribution (atoms z [B, K], masses p [B, K]) onto an increasing `support` [K]: returns [B, K]."""
    K = support.shape[0]
    z = torch.minimum(torch.maximum(z, support[0]), support[-1])
    up = torch.zeros_like(support); up[:-1] = support[1:] - support[:-1]                # distance to the next atom (0: none)
    dn = torch.zeros_like(support); dn[1:] = support[1:] - support[:-1]
    delta = z[:, None, :] - support[None, :, None]                                      # [B, target atom j, source atom k]
    width = torch.where(delta >= 0, up[None, :, None], dn[None, :, None]).expand_as(delta)
    frac = torch.where(width > 0, delta.abs()/torch.where(width > 0, width, torch.ones_like(width)), torch.zeros_like(delta))
    return ((1.0 - frac).clamp(0.0, 1.0)*p[:, None, :]).sum(-1)


def td_loss(q_t, bias_t, q_tm1, bias_tm1, support, reward, discount, gamma, dtype):
    """q_t [N, B, K] target logits, q_tm1 [B, K] online logits, biases [K] or None (added here).  Returns a dict: loss_rows [B], loss
    (mean), d_logits [B, K], d_bias [K] (gradients of the MEAN loss), sampled_q [N, B], target [B, K]."""
    q_t, q_tm1, support, reward, discount = (_c(t, dtype) for t in (q_t, q_tm1, support, reward, discount))
    bt = _c(bias_t, dtype) if bias_t is not None else torch.zeros_like(support)
    b1 = (_c(bias_tm1, dtype) if bias_tm1 is not None else torch.zeros_like(support)).requires_grad_(True)
    q_tm1.requires_grad_(True)
    with torch.no_grad():
        logp = torch.log_softmax(q_t + bt, -1)
        sampled_q = (torch.softmax(q_t + bt, -1)*support).sum(-1)
        p_t = torch.softmax(torch.logsumexp(logp, 0), -1)                               # mean of the N head distributions
        g = torch.tensor(gamma, dtype=torch.float32).to(dtype)
        z = reward[:, None] + (g*discount)[:, None]*support[None, :]
        target = l2_project(z, p_t, support)
    rows = -(target*torch.log_softmax(q_tm1 + b1, -1)).sum(-1)
    loss = rows.mean(); loss.backward()
    return dict(loss_rows=rows.detach(), loss=loss.detach(), d_logits=q_tm1.grad, d_bias=b1.grad, sampled_q=sampled_q, target=target, z=z)


# ------------------------------------------------------------------ layer epilogues
def bias_ln_act(x, bias, gamma, beta, eps, act, dy, dtype, rowadd=None):
    """y = act(LayerNorm(x + bias [+ rowadd[r mod period]])) (two-pass variance), act 0 none / 1 tanh.  With dy: also dx, dbias, dgamma, dbeta."""
    x, bias, gamma, beta = (_c(t, dtype).requires_grad_(dy is not None) for t in (x, bias, gamma, beta))
    v = x + bias
    if rowadd is not None:
        ra = _c(rowadd, dtype); v = v + ra.repeat(x.shape[0]//ra.shape[0], 1)
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean)**2).mean(-1, keepdim=True)
    rstd = (var + torch.tensor(eps, dtype=torch.float32).to(dtype)).rsqrt()
    xhat = (v - mean)*rstd
    u = xhat*gamma + beta
    y = torch.tanh(u) if act == 1 else u
    out = dict(y=y.detach(), xhat=xhat.detach(), rstd=rstd.detach()[:, 0])
    if dy is not None:
        y.backward(_c(dy, dtype))
        out.update(dx=x.grad, dbias=bias.grad, dgamma=gamma.grad, dbeta=beta.grad)
    return out


def elu(z):
    return torch.where(z > 0, z, torch.expm1(torch.minimum(z, torch.zeros_like(z))))


def bias_elu(x, bias, dy, dtype):
    x, bias = _c(x, dtype), _c(bias, dtype)
    z = x + bias
    out = dict(y=elu(z), z=z)
    if dy is not None:
        dx = _c(dy, dtype)*torch.where(z > 0, torch.ones_like(z), torch.exp(torch.minimum(z, torch.zeros_like(z))))
        out.update(dx=dx, dbias=dx.sum(0))
    return out


# ------------------------------------------------------------------ Gaussian head
def gauss_head(zm, zs, bm, bs, mul, min_scale, dmean, dstd, dtype, from_std=False):
    """mean = zm + bm, std = softplus(zs + bs) mul + min_scale; dzs = dstd sigmoid(zs + bs) mul, dbm / dbs its column sums.
    from_std: the sigmoid is recovered from the stddev (as fbl_gauss_head_bwd_std has to): -expm1(-(std - min_scale) / mul)."""
    zm, zs, bm, bs = (_c(t, dtype) for t in (zm, zs, bm, bs))
    f = lambda s: torch.tensor(s, dtype=torch.float32).to(dtype)
    mul, min_scale = f(mul), f(min_scale)
    z = zs + bs
    std = softplus(z)*mul + min_scale
    out = dict(mean=zm + bm, std=std)
    if dstd is not None:
        sig = -torch.expm1(-(std - min_scale)/mul) if from_std else torch.sigmoid(z)
        dzs = _c(dstd, dtype)*sig*mul
        out.update(dzs=dzs, dbs=dzs.sum(0), dbm=_c(dmean, dtype).sum(0), sigmoid=sig)
    return out


# ------------------------------------------------------------------ optimizer
def segment_sqnorms(g, ends, dtype):
    g = _c(g, dtype); lo = 0; out = []
    for hi in ends:
        out.append((g[lo:hi]*g[lo:hi]).sum()); lo = hi
    return torch.stack(out)


class Adam:
    """Adam on a flat buffer of consecutive segments: per segment a learning rate, global-norm clipping grad *= min(1, clip / (||grad|| + 1e-6))
    (clip <= 0: none) and a floor the parameters are clamped to after the update.  beta1, beta2, eps, lr, clip are the float32 numbers
    the kernel receives."""

    def __init__(self, p, ends, lrs, clips, floors, dtype, betas=(0.9, 0.999), eps=1e-8):
        f = lambda s: torch.tensor(s, dtype=torch.float32).to(dtype)
        self.dtype = dtype; self.p = _c(p, dtype).clone(); self.m = torch.zeros_like(self.p); self.v = torch.zeros_like(self.p)
        self.ends = list(ends); self.lrs = [f(x) for x in lrs]; self.clips = [f(x) for x in clips]; self.floors = list(floors)
        self.b1, self.b2, self.eps = f(betas[0]), f(betas[1]), f(eps); self.t = 0
        self.clipped = []                    # per step and segment: was the gradient scaled?

    def step(self, g):
        g = _c(g, self.dtype); self.t += 1
        bc1 = -torch.expm1(self.t*torch.log(self.b1)); bc2s = (-torch.expm1(self.t*torch.log(self.b2))).sqrt()       # 1 - beta^t
        lo = 0; flags = []
        for hi, lr, clip, fl in zip(self.ends, self.lrs, self.clips, self.floors):
            gs = g[lo:hi]
            if clip > 0:
                s = torch.clamp(clip/((gs*gs).sum().sqrt() + 1e-6), max=1.0); flags.append(bool(s < 1.0)); gs = gs*s
            else:
                flags.append(False)
            self.m[lo:hi] = self.b1*self.m[lo:hi] + (1 - self.b1)*gs
            self.v[lo:hi] = self.b2*self.v[lo:hi] + (1 - self.b2)*gs*gs
            p = self.p[lo:hi] - (lr/bc1)*self.m[lo:hi]/(self.v[lo:hi].sqrt()/bc2s + self.eps)
            self.p[lo:hi] = p if fl is None else p.clamp(min=fl)
            lo = hi
        self.clipped.append(flags)
