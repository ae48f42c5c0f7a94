#!/usr/bin/env python3
"""Throughput of fb_batch_transition_fd (csrc/fb_deriv.hpp) beside the host loop it replaces and the step kernel's ceiling.

For walk_imitation and flight_imitation, centred differences, n_substeps = 1, A and B, at 64 and 1024 frames:

    kernel      Batch.transition_fd on a batch of `frames` environments: frames/s and perturbed substeps/s, from device events around a
                call that ends in a synchronise, after a warm-up call of the same shape
    host_loop   the same matrices by the means the engine had before: one batch of 2 (ndx + nu) environments per frame, the perturbed
                states written with fb_batch_set, then forward, substep(1), fb_batch_get of QPOS / QVEL / ACT (building the perturbed
                states on the host is NOT timed; at most --host-frames frames are run, the rate is per frame)
    ceiling     the plain step kernel's substep rate at 4096 environments (tools/step_kernel_bench.py --only plain, a child process)
                and the ratio of the kernel's perturbed substeps/s to it

--acceptance N alternates the kernel and the host loop N times at 64 walking frames and reports whether the slowest kernel run beats the
fastest host-loop run.  One JSON line.

    python tools/derivative_bench.py [--frames 64,1024] [--tasks walk_imitation,flight_imitation] [--host-frames 64] [--acceptance 3]
                                     [--default-build] [--no-ceiling]
"""
import argparse, json, os, subprocess, sys, time
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
import numpy as np
import torch
from flybody_amd import derivatives, engine
from flybody_amd.reference import default_walking_reference

ap = argparse.ArgumentParser()
ap.add_argument('--frames', default='64,1024'); ap.add_argument('--tasks', default='walk_imitation,flight_imitation')
ap.add_argument('--host-frames', type=int, default=64); ap.add_argument('--acceptance', type=int, default=3)
ap.add_argument('--default-build', action='store_true', help='libflybody_hip.so instead of the 12-per-CU build')
ap.add_argument('--no-ceiling', action='store_true')
a = ap.parse_args()
dense = not a.default_build
torch.cuda.set_device(0)
st = torch.cuda.current_stream(); h = st.cuda_stream
EPS = 1e-6


def make_batch(task, n):
    """n environments of `task` in states worth linearising: walking flies five random control steps after a reset (legs on the floor);
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
        r = np.asarray(arr['actuator_ctrlrange'], float)
        B.set('CTRL', r[:, 0] + (r[:, 1] - r[:, 0])*rng.uniform(0.3, 0.7, (n, len(r))))
        B.forward(h); torch.cuda.synchronize()
    return model, B


def time_kernel(B):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st); r = B.transition_fd(eps=EPS, stream=h); e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)*1e-3, r


def perturbed_states(model, q, v, act, ctrl):
    """The 2 (ndx + nu) states of one frame's centred columns: minus side, plus side per column."""
    nv, na, nu = model.dim('nv'), model.dim('na'), model.dim('nu')
    ncol = 2*nv + na + nu
    d = np.zeros((2*ncol, ncol)); d[0::2] = -EPS*np.eye(ncol); d[1::2] = EPS*np.eye(ncol)
    Q = derivatives.integrate_pos(model, np.tile(q, (2*ncol, 1)), d[:, :nv])
    return Q, v + d[:, nv:2*nv], act + d[:, 2*nv:2*nv + na], ctrl + d[:, 2*nv + na:]


def time_host_loop(model, B, frames):
    """Seconds per frame of the host loop over `frames` frames of B (set x 4, forward, substep, get x 3 on a helper batch)."""
    nv, na, nu = model.dim('nv'), model.dim('na'), model.dim('nu')
    Q, V, C = B.get('QPOS'), B.get('QVEL'), B.get('CTRL')
    A = B.get('ACT') if na else np.zeros((B.n_env, 0))
    states = [perturbed_states(model, Q[f], V[f], A[f], C[f]) for f in range(frames)]
    H = engine.Batch(model, 2*(2*nv + na + nu), precision=64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for q, v, act, ctrl in states:
        H.set('QPOS', q); H.set('QVEL', v); H.set('CTRL', ctrl)
        if na:
            H.set('ACT', act)
        H.forward(); H.substep(1)
        H.get('QPOS'); H.get('QVEL')
        if na:
            H.get('ACT')
    H.synchronize()
    return (time.perf_counter() - t0)/frames


out = dict(tool='derivative_bench', engine=engine.version(engine.HIP_LIB_DENSE if dense else None), eps=EPS, centered=True, n_substeps=1, results=[])
ceiling = None
if not a.no_ceiling:
    cmd = [sys.executable, os.path.join(HERE, 'step_kernel_bench.py'), '--only', 'plain', '--envs', '4096', '--steps', '30', '--warmup', '10'] + (['--default-build'] if a.default_build else [])
    r = json.loads(subprocess.run(cmd, capture_output=True, text=True, check=True).stdout.strip().splitlines()[-1])
    nsub = engine.Model.from_asset('walk_imitation', dense=dense).dim('nsubstep')
    ceiling = r['env_steps_per_s']['plain']*nsub
    out['k_fly_substeps_per_s_4096_walking_envs'] = ceiling
for task in a.tasks.split(','):
    for n in (int(x) for x in a.frames.split(',')):
        model, B = make_batch(task, n)
        per_frame = 2*(2*model.dim('nv') + model.dim('na') + model.dim('nu'))
        time_kernel(B)                                                        # warm-up: allocates the pool and the staging buffer
        t, r = time_kernel(B)
        tickets = B.fd_tickets()
        hf = min(n, a.host_frames)
        th = time_host_loop(model, B, hf)
        row = dict(task=task, frames=n, kernel_s=round(t, 5), frames_per_s=round(n/t, 1), perturbed_substeps_per_s=round(tickets/t),
                   tickets=tickets, status_any=int(r.status.max().item()), pool_rows=B.resident_slots,
                   host_loop_frames=hf, host_loop_frames_per_s=round(1/th, 2), host_loop_substeps_per_s=round(per_frame/th),
                   speedup_over_host_loop=round((n/t)*th, 1))
        if ceiling and task == 'walk_imitation':
            row['ratio_to_k_fly_substep_rate'] = round(tickets/t/ceiling, 3)
        out['results'].append(row)
        if task == 'walk_imitation' and n == 64 and a.acceptance > 0:
            ks, hs = [], []
            for _ in range(a.acceptance):
                ks.append(time_kernel(B)[0]); hs.append(time_host_loop(model, B, 64)*64)
            out['acceptance_64_walking_frames'] = dict(kernel_s=[round(x, 5) for x in ks], host_loop_s=[round(x, 4) for x in hs],
                                                       slowest_kernel_beats_fastest_host_loop=bool(max(ks) < min(hs)))
        del B
print(json.dumps(out))
