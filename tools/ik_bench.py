#!/usr/bin/env python3
"""Throughput of the batched inverse kinematics (fb_batch_ik, csrc/fb_ik.hpp) on one GPU: `frames` seeded leg poses (hinges uniform in
[lo/2, hi/2] of their ranges), fitted from qpos0 on the 12 leg sites / 66 leg hinges, FP64, a FIXED number of iterations
(progress_threshold = 0: every frame runs all of them).  Device events around the synchronised IK launch; one JSON line.  Run it under
`rocprofv3 --kernel-trace --stats` for the k_ik kernel time alone.

    python tools/ik_bench.py [--frames 4096] [--iters 20000] [--repeat 2] [--lib PATH | --dense]
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
import torch
from flybody_amd import engine

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=4096); ap.add_argument('--iters', type=int, default=20000)
ap.add_argument('--repeat', type=int, default=2); ap.add_argument('--lib', default=None); ap.add_argument('--dense', action='store_true')
a = ap.parse_args()
torch.cuda.set_device(0)
model = engine.Model.from_asset('walk_imitation', lib_path=a.lib, dense=a.dense)
arr = model.arrays
names = [str(s) for s in arr['names_site']]
sites = [names.index(s) for s in names if s.startswith(('tarsus_', 'claw_'))]
legs = [int(j) for j in arr['leg_joints']]
lo, hi = arr['jnt_range'][legs].T
poses = np.tile(arr['qpos0'], (a.frames, 1))
poses[:, arr['jnt_qposadr'][legs]] = np.random.default_rng(7).uniform(0.5*lo, 0.5*hi, (a.frames, len(legs)))
B = engine.Batch(model, a.frames, precision=64)
B.set('QPOS', poses); B.forward()
T = B.get('SITE_XPOS').reshape(a.frames, -1, 3)[:, sites].copy()
st = torch.cuda.current_stream(); h = st.cuda_stream
B.set('QPOS', arr['qpos0']); B.ik(sites, legs, T, progress_threshold=0.0, max_steps=100, stream=h); torch.cuda.synchronize()   # warm-up
ms = []
for _ in range(a.repeat):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    B.set('QPOS', arr['qpos0'])
    e0.record(st)
    B.ik(sites, legs, T, progress_threshold=0.0, max_steps=a.iters, stream=h)
    e1.record(st)
    torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1))
steps = B.get('IK_STEPS'); first = B.get('IK_ERR')[:, 1]
assert (steps[:, 0] == a.iters - 1).all() and np.isfinite(first).all()
t = min(ms) / 1e3
print(json.dumps(dict(tool='ik_bench', engine=engine.version(a.lib if a.lib else (engine.HIP_LIB_DENSE if a.dense else None)), frames=a.frames,
                      iters=a.iters, ms=[round(x, 2) for x in ms], frames_per_s=round(a.frames / t, 1), iters_per_s=round(a.frames*a.iters / t),
                      us_per_iter_per_frame_wall=round(t / a.iters * 1e6, 3), err_first_term_median=float(np.median(first)),
                      err_first_term_max=float(first.max()))))
