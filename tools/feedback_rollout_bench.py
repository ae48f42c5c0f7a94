#!/usr/bin/env python3
"""Throughput of fb_batch_rollout_feedback (csrc/fb_rollout.hpp: k_closedloop_rollout) beside the open-loop kernel at the same
shape and the host loop it replaces.

walk_imitation, closed-loop rollouts of T = 10 intervals at n_substeps = 1 (feedback at the physics rate) and at the model's own substep
count, every rollout from an environment of its own, n_roll / n_nom consecutive rollouts on each nominal with dense gains -- the order
BatchedFlyEnv.rollout(feedback=..., samples=K) and a line search produce; the rollouts of one nominal share its K_t through the caches
(--scatter: rollout r on nominal r % n_nom instead, so that neighbouring waves read different gains):

    closed      Batch.rollout_feedback (sensors off): device events around a call that ends in a synchronise, after a warm-up call of the
                same shape.  The call includes the shim's transpose of K to the kernel's layout (n_nom x T x 130 KB for the fly)
    open        Batch.rollout(ctrl = u_nom) of the same shape, timed the same way: what the feedback costs on top of the physics
    host_loop   the same law by the means the engine had before: a second batch of n_roll environments in the same states and per
                interval get('QPOS' / 'QVEL' / 'ACT'), lqr.state_difference and the gains in numpy, set('CTRL'), substep(n) -- wall clock
                around the T intervals; creating the second batch and copying the states in is NOT timed
The three are alternated --passes times (default 3) and every pass is reported.  max_rel_diff_to_host_loop: the closed-loop rollouts'
last qpos / qvel against the host loop's (not zero: summation order, and the second batch's warm start -- see tools/rollout_bench.py).
One JSON line.

    python tools/feedback_rollout_bench.py [--sizes 3072,12288] [--horizon 10] [--nominals 64] [--passes 3] [--default-build]
"""
import argparse, json, os, sys, time, types
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
import numpy as np
import torch
from flybody_amd import engine, lqr
from flybody_amd.reference import default_walking_reference

ap = argparse.ArgumentParser()
ap.add_argument('--sizes', default='3072,12288'); ap.add_argument('--horizon', type=int, default=10)
ap.add_argument('--nominals', type=int, default=64); ap.add_argument('--passes', type=int, default=3)
ap.add_argument('--default-build', action='store_true', help='libflybody_hip.so instead of the 12-per-CU build')
ap.add_argument('--scatter', action='store_true', help='rollout r on nominal r %% n_nom: neighbouring waves read different gains')
a = ap.parse_args()
dense = not a.default_build
torch.cuda.set_device(0)
st = torch.cuda.current_stream(); h = st.cuda_stream
T = a.horizon


def make_batch(model, n):
    """n walking flies five random control steps after a reset (legs on the floor), as tools/rollout_bench.py makes them."""
    B = engine.Batch(model, n, precision=64)
    qp, qv = default_walking_reference()
    B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    act = torch.empty(n, model.dim('nact'), device='cuda')
    for k in range(5):
        B.random_actions(act.data_ptr(), k, seed=1, dist=1, stream=h); B.step_ptr(act.data_ptr(), h)
    torch.cuda.synchronize()
    return B


def load_states(H, S):
    H.set('QPOS', S['QPOS']); H.set('QVEL', S['QVEL']); H.set('CTRL', S['CTRL']); H.set('ACT', S['ACT'])
    H.forward(h); torch.cuda.synchronize()


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st); r = f(); e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)*1e-3, r


def host_loop(H, shim, x_nom, u_nom, K, noms, lo, hi, limited, nsub):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(T):
        x = np.concatenate([H.get('QPOS'), H.get('QVEL'), H.get('ACT')], axis=1)
        dx = lqr.state_difference(shim, x, x_nom[noms, t])
        u = u_nom[noms, t].copy()
        for m in range(len(x_nom)):
            u[noms == m] += dx[noms == m] @ K[m, t].T
        H.set('CTRL', np.where(limited, np.clip(u, lo, hi), u)); H.substep(nsub, h)
    q = H.get('QPOS'); v = H.get('QVEL')
    return time.perf_counter() - t0, q, v


model = engine.Model.from_asset('walk_imitation', dense=dense)
shim = types.SimpleNamespace(arrays=model.arrays)
nq, nv, na, nu = (model.dim(k) for k in ('nq', 'nv', 'na', 'nu'))
ndx = 2*nv + na
r_ = np.asarray(model.arrays['actuator_ctrlrange'], float)
lo, hi, limited = r_[:, 0], r_[:, 1], np.asarray(model.arrays['actuator_ctrllimited']).astype(bool)
out = dict(tool='feedback_rollout_bench', engine=engine.version(engine.HIP_LIB_DENSE if dense else None), horizon=T, passes=a.passes,
           k_bytes_per_interval=nu*ndx*8, results=[])
mean = lambda x: float(np.mean(x))
for size in a.sizes.split(','):
    n = int(size)
    n_nom = min(a.nominals, n)
    B = make_batch(model, n)
    S = {f: B.get(f) for f in ('QPOS', 'QVEL', 'CTRL', 'ACT')}
    H = engine.Batch(model, n, precision=64)
    rng = np.random.default_rng(2)
    noms = (np.arange(n) % n_nom if a.scatter else np.arange(n)*n_nom//n).astype(np.int32)
    # nominal m: the state of its first rollout's environment held over the horizon, mid-range inputs, dense gains that move an input
    # by a few per cent of its range for a tangent distance of 0.1 (velocity columns a hundred times smaller)
    first = np.array([np.flatnonzero(noms == m)[0] for m in range(n_nom)])
    x_nom = np.repeat(np.concatenate([S['QPOS'], S['QVEL'], S['ACT']], axis=1)[first, None], T, axis=1)
    u_nom = lo + (hi - lo)*rng.uniform(0.3, 0.7, (n_nom, T, nu))
    K = 0.05*(hi - lo)[:, None]*rng.normal(size=(n_nom, T, nu, ndx)); K[..., nv:2*nv] *= 0.01
    xd, ud, Kd = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (x_nom, u_nom, K))
    uo = ud[torch.from_numpy(noms).long().cuda()].contiguous()
    for nsub in (1, model.dim('nsubstep')):
        closed = lambda: B.rollout_feedback(xd, ud, Kd, nom_ids=noms, n_substeps=nsub, stream=h)
        open_ = lambda: B.rollout(ctrl=uo, n_substeps=nsub, stream=h)
        load_states(B, S)
        timed(closed); timed(open_)                                           # warm-up: allocates the scratch rows
        load_states(H, S); host_loop(H, shim, x_nom, u_nom, K, noms, lo, hi, limited, nsub)
        cs, os_, hs, gap = [], [], [], 0.0
        for _ in range(a.passes):
            t, res = timed(closed); cs.append(t)
            t, _ = timed(open_); os_.append(t)
            load_states(H, S)
            th, q, v = host_loop(H, shim, x_nom, u_nom, K, noms, lo, hi, limited, nsub); hs.append(th)
            last = res.state[:, -1].cpu().numpy()
            gap = max(gap, float(np.abs(last[:, :nq] - q).max()/np.abs(q).max()), float(np.abs(last[:, nq:nq + nv] - v).max()/np.abs(v).max()))
        u = res.ctrl.cpu().numpy()
        sub = n*T*nsub
        row = dict(n_roll=n, n_nom=n_nom, n_substeps=nsub, rollouts_run=B.rollouts_run(), status_any=int(res.status.max().item()),
                   saturated_fraction=round(float((((u == lo) | (u == hi)) & limited).mean()), 4),
                   closed_s=[round(x, 5) for x in cs], open_s=[round(x, 5) for x in os_], host_loop_s=[round(x, 5) for x in hs],
                   closed_substeps_per_s=round(sub/mean(cs)), open_substeps_per_s=round(sub/mean(os_)), host_loop_substeps_per_s=round(sub/mean(hs)),
                   closed_over_open=round(mean(cs)/mean(os_), 4), feedback_us_per_interval=round((mean(cs) - mean(os_))/T*1e6, 1),
                   speedup_over_host_loop=round(mean(hs)/mean(cs), 2), max_rel_diff_to_host_loop=float('%.1e' % gap))
        out['results'].append(row)
        print('feedback_rollout_bench:', json.dumps(row), file=sys.stderr, flush=True)
    del B, H
print(json.dumps(out))
