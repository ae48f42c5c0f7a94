#!/usr/bin/env python3
"""Throughput of fb_batch_rollout (csrc/fb_rollout.hpp) beside the host loop it replaces and the step kernel's substep rate.

For walk_imitation and flight_imitation, ctrl rollouts of T = 10 intervals of the model's own substep count, at n_roll = 64, 1 x and 4 x
the scratch rows (the resident wave slots of the build), every rollout from an environment of its own:

    kernel      Batch.rollout (sensors off): rollouts/s and substeps/s, from device events around a call that ends in a synchronise,
                after a warm-up call of the same shape
    host_loop   the same trajectories by the means the engine had before: a second batch of n_roll environments in the same states
                and per interval set('CTRL'), substep(n), get('QPOS'), get('QVEL') -- wall clock around the T intervals (every one of
                these calls synchronises); creating the second batch and copying the states in is NOT timed
    k_fly       the second batch's T x substep(n) alone, device events, no host copies: the step kernel's substep rate at that size
The three are alternated --passes times (default 3) and every pass is reported.  ceiling: the plain step kernel's substep rate at 4096
walking environments (tools/step_kernel_bench.py --only plain, a child process) and the ratio of the kernel's substeps/s to it
(walk_imitation).  max_rel_diff_to_host_loop: the rollouts' last qpos / qvel against the host loop's, max |difference| over max |value|
(not zero: the second batch's forward() starts its solve from the acceleration its previous pass left, the first batch's from its own;
bit-equality from equal histories is tests/test_gpu_rollout.py's business).  One JSON line.

    python tools/rollout_bench.py [--tasks walk_imitation,flight_imitation] [--sizes 64,1x,4x] [--horizon 10] [--passes 3]
                                  [--default-build] [--no-ceiling]
"""
import argparse, json, os, subprocess, sys, time
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
import numpy as np
import torch
from flybody_amd import engine
from flybody_amd.reference import default_walking_reference

ap = argparse.ArgumentParser()
ap.add_argument('--tasks', default='walk_imitation,flight_imitation'); ap.add_argument('--sizes', default='64,1x,4x')
ap.add_argument('--horizon', type=int, default=10); ap.add_argument('--passes', type=int, default=3)
ap.add_argument('--default-build', action='store_true', help='libflybody_hip.so instead of the 12-per-CU build')
ap.add_argument('--no-ceiling', action='store_true')
a = ap.parse_args()
dense = not a.default_build
torch.cuda.set_device(0)
st = torch.cuda.current_stream(); h = st.cuda_stream


def make_batch(task, n):
    """n environments of `task` in states worth rolling out: walking flies five random control steps after a reset (legs on the floor);
    flying ones in the air with perturbed joints and velocities."""
    model = engine.Model.from_asset(task, dense=dense)
    B = engine.Batch(model, n, precision=64)
    if task == 'walk_imitation':
        qp, qv = default_walking_reference()
        B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
        act = torch.empty(n, model.dim('nact'), device='cuda')
        for k in range(5):
            B.random_actions(act.data_ptr(), k, seed=1, dist=1, stream=h); B.step_ptr(act.data_ptr(), h)
        torch.cuda.synchronize()
    else:
        arr = model.arrays
        rng = np.random.default_rng(0)
        q = np.tile(np.asarray(arr['qpos0'], float), (n, 1)); q[:, 7:] += rng.uniform(-0.05, 0.05, (n, q.shape[1] - 7)); q[:, 2] = 2.0
        lim = [j for j in range(len(arr['jnt_type'])) if arr['jnt_type'][j] == 3 and arr['jnt_limited'][j]]
        lo, hi = np.asarray(arr['jnt_range'])[lim].T; qa = np.asarray(arr['jnt_qposadr'])[lim]
        q[:, qa] = np.clip(q[:, qa], lo + 0.05*(hi - lo), hi - 0.05*(hi - lo))
        B.set('QPOS', q); B.set('QVEL', rng.normal(size=(n, model.dim('nv')))*0.5)
        B.forward(h); torch.cuda.synchronize()
    return model, B


def load_states(H, S):
    """The second batch in the states S = the first batch's (QPOS, QVEL, ACT, CTRL), forward() run as on the first."""
    H.set('QPOS', S['QPOS']); H.set('QVEL', S['QVEL']); H.set('CTRL', S['CTRL'])
    if 'ACT' in S:
        H.set('ACT', S['ACT'])
    H.forward(h); torch.cuda.synchronize()


def time_kernel(B, u, nsub):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st); r = B.rollout(ctrl=u, n_substeps=nsub, stream=h); e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)*1e-3, r


def time_host_loop(H, ctrl, nsub):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(ctrl.shape[1]):
        H.set('CTRL', ctrl[:, t]); H.substep(nsub, h)
        q = H.get('QPOS'); v = H.get('QVEL')
    H.synchronize()
    return time.perf_counter() - t0, q, v


def time_k_fly(H, T, nsub):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(T):
        H.substep(nsub, h)
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)*1e-3


out = dict(tool='rollout_bench', engine=engine.version(engine.HIP_LIB_DENSE if dense else None), horizon=a.horizon, passes=a.passes, results=[])
ceiling = None
if not a.no_ceiling:
    cmd = [sys.executable, os.path.join(HERE, 'step_kernel_bench.py'), '--only', 'plain', '--envs', '4096', '--steps', '30', '--warmup', '10'] + (['--default-build'] if a.default_build else [])
    r = json.loads(subprocess.run(cmd, capture_output=True, text=True, check=True).stdout.strip().splitlines()[-1])
    ceiling = r['env_steps_per_s']['plain']*engine.Model.from_asset('walk_imitation', dense=dense).dim('nsubstep')
    out['k_fly_substeps_per_s_4096_walking_envs'] = ceiling
T = a.horizon
mean = lambda x: float(np.mean(x))
for task in a.tasks.split(','):
    rows = engine.Batch(engine.Model.from_asset(task, dense=dense), 1, precision=64).resident_slots
    for size in a.sizes.split(','):
        n = int(size[:-1])*rows if size.endswith('x') else int(size)
        model, B = make_batch(task, n)
        nsub, na = model.dim('nsubstep'), model.dim('na')
        S = {f: B.get(f) for f in ('QPOS', 'QVEL', 'CTRL') + (('ACT',) if na else ())}
        r_ = np.asarray(model.arrays['actuator_ctrlrange'], float)
        ctrl = r_[:, 0] + (r_[:, 1] - r_[:, 0])*np.random.default_rng(2).uniform(0.3, 0.7, (n, T, len(r_)))
        u = torch.from_numpy(ctrl).cuda()
        H = engine.Batch(model, n, precision=64)
        load_states(B, S)                                                     # (both batches start from a forward() of the same states)
        time_kernel(B, u, nsub)                                               # warm-up: allocates the scratch rows
        try:                                                                  # the scratch rows ARE the resident slots: one more is refused
            B.rollout(ctrl=u[:1], n_substeps=1, pool_rows=rows + 1); exact = False
        except engine.EngineError:
            B.rollout(ctrl=u[:1], n_substeps=1, pool_rows=rows); exact = True
        load_states(H, S); time_host_loop(H, ctrl, nsub)
        ks, hs, fs, gap = [], [], [], 0.0
        for _ in range(a.passes):
            t, res = time_kernel(B, u, nsub); ks.append(t)
            load_states(H, S)
            th, q, v = time_host_loop(H, ctrl, nsub); hs.append(th)
            nq = model.dim('nq')
            last = res.state[:, -1].cpu().numpy()
            lv = last[:, nq:nq + model.dim('nv')]
            gap = max(gap, float(np.abs(last[:, :nq] - q).max()/np.abs(q).max()), float(np.abs(lv - v).max()/np.abs(v).max()))
            load_states(H, S); fs.append(time_k_fly(H, T, nsub))
        sub = n*T*nsub
        row = dict(task=task, n_roll=n, scratch_rows=rows, scratch_rows_exact=exact, n_substeps=nsub, rollouts_run=B.rollouts_run(), status_any=int(res.status.max().item()),
                   kernel_s=[round(x, 5) for x in ks], host_loop_s=[round(x, 5) for x in hs], k_fly_substeps_s=[round(x, 5) for x in fs],
                   rollouts_per_s=round(n/mean(ks), 1), substeps_per_s=round(sub/mean(ks)), host_loop_rollouts_per_s=round(n/mean(hs), 1),
                   host_loop_substeps_per_s=round(sub/mean(hs)), k_fly_substeps_per_s_same_size=round(sub/mean(fs)),
                   speedup_over_host_loop=round(mean(hs)/mean(ks), 3), ratio_to_k_fly_same_size=round(mean(fs)/mean(ks), 3), max_rel_diff_to_host_loop=float('%.1e' % gap))
        if ceiling and task == 'walk_imitation':
            row['ratio_to_k_fly_substep_rate'] = round(sub/mean(ks)/ceiling, 3)
        out['results'].append(row)
        print('rollout_bench:', json.dumps(row), file=sys.stderr, flush=True)
        del B, H
print(json.dumps(out))
