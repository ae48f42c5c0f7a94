#!/usr/bin/env python3
"""Cost of the applied-force step kernel (k_step_forces, csrc/fb_forces.hpp) against the plain one (k_fly): ms per control step of two
walk_imitation batches fed the same seeded random actions, one with the force arrays allocated and all zero, one without them.  Zero
forces give the same trajectories, so both batches do the same physics; what differs is the applied-force stage and the sensor stage
that reads xfrc_applied.  Device events around every step, the two batches alternated step by step; median, mean and minimum over
`steps` control steps after `warmup`.  One JSON line.

    python tools/forces_bench.py [--envs 4096] [--steps 100] [--warmup 30] [--default-build] [--precision 64]
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
import torch
from flybody_amd import engine
from flybody_amd.reference import default_walking_reference

ap = argparse.ArgumentParser()
ap.add_argument('--envs', type=int, default=4096); ap.add_argument('--steps', type=int, default=100); ap.add_argument('--warmup', type=int, default=30)
ap.add_argument('--default-build', action='store_true', help='libflybody_hip.so instead of the 12-per-CU build')
ap.add_argument('--precision', type=int, default=64)
a = ap.parse_args()
torch.cuda.set_device(0)
dense = not a.default_build and a.precision == 64
model = engine.Model.from_asset('walk_imitation', dense=dense)
qp, qv = default_walking_reference()
st = torch.cuda.current_stream(); h = st.cuda_stream
batches = {}
for name in ('k_fly', 'k_step_forces'):
    B = engine.Batch(model, a.envs, precision=a.precision)
    B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    if name == 'k_step_forces':
        B.set('XFRC_APPLIED', 0.0)
    assert B.forces_active == (name == 'k_step_forces')
    batches[name] = B
act = torch.empty(a.envs, model.dim('nact'), device='cuda')
ms = {name: [] for name in batches}
for k in range(a.warmup + a.steps):
    batches['k_fly'].random_actions(act.data_ptr(), k, seed=3, dist=1, stream=h)
    for name in (('k_fly', 'k_step_forces') if k % 2 == 0 else ('k_step_forces', 'k_fly')):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); batches[name].step_ptr(act.data_ptr(), h); e1.record(st)
        torch.cuda.synchronize()
        if k >= a.warmup:
            ms[name].append(e0.elapsed_time(e1))
same = all(np.array_equal(batches['k_fly'].get(f), batches['k_step_forces'].get(f)) for f in ('QPOS', 'QVEL'))
stat = lambda x: dict(median=round(float(np.median(x)), 4), mean=round(float(np.mean(x)), 4), min=round(float(np.min(x)), 4))
out = dict(tool='forces_bench', engine=engine.version(engine.HIP_LIB_DENSE if dense else None), envs=a.envs, precision=a.precision, steps=a.steps,
           substep_scheduler=batches['k_fly'].substep_scheduler, same_trajectories=bool(same),
           ms_per_control_step={name: stat(v) for name, v in ms.items()})
out['ratio_median'] = round(out['ms_per_control_step']['k_step_forces']['median']/out['ms_per_control_step']['k_fly']['median'], 4)
out['ratio_mean'] = round(out['ms_per_control_step']['k_step_forces']['mean']/out['ms_per_control_step']['k_fly']['mean'], 4)
print(json.dumps(out))
