#!/usr/bin/env python3
"""Cost of the control-law step kernel (k_step_law, csrc/fb_law.hpp) against the applied-force kernel (k_step_forces) and the plain one
(k_fly): ms per control step of three walk_imitation batches fed the same seeded random actions -- one plain, one with the force arrays
allocated and all zero, one with an all-zero law on top.  Zero forces and a zero law give the same trajectories, so the three batches
do the same physics; what differs is the applied-force stage, the sensor stage that reads xfrc_applied, and the law stage.  Device
events around every step, the batches alternated step by step (the order rotates); median, mean and minimum over `steps` control steps
after `warmup`.  One JSON line.

    python tools/law_bench.py [--envs 4096] [--steps 100] [--warmup 30] [--default-build] [--precision 64]
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
NAMES = ('k_fly', 'k_step_forces', 'k_step_law')
batches = {}
for name in NAMES:
    B = engine.Batch(model, a.envs, precision=a.precision)
    B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    if name == 'k_step_forces':
        B.set('XFRC_APPLIED', 0.0)
    if name == 'k_step_law':
        B.set_control_law()
    assert B.forces_active == (name != 'k_fly') and B.control_law_active == (name == 'k_step_law')
    batches[name] = B
act = torch.empty(a.envs, model.dim('nact'), device='cuda')
ms = {name: [] for name in batches}
for k in range(a.warmup + a.steps):
    batches['k_fly'].random_actions(act.data_ptr(), k, seed=3, dist=1, stream=h)
    for j in range(3):
        name = NAMES[(k + j) % 3]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); batches[name].step_ptr(act.data_ptr(), h); e1.record(st)
        torch.cuda.synchronize()
        if k >= a.warmup:
            ms[name].append(e0.elapsed_time(e1))
same = all(np.array_equal(batches['k_fly'].get(f), batches[n].get(f)) for f in ('QPOS', 'QVEL') for n in NAMES[1:])
stat = lambda x: dict(median=round(float(np.median(x)), 4), mean=round(float(np.mean(x)), 4), min=round(float(np.min(x)), 4))
out = dict(tool='law_bench', engine=engine.version(engine.HIP_LIB_DENSE if dense else None), envs=a.envs, precision=a.precision, steps=a.steps,
           substep_scheduler=batches['k_fly'].substep_scheduler, same_trajectories=bool(same),
           ms_per_control_step={name: stat(v) for name, v in ms.items()})
m = out['ms_per_control_step']
for key in ('median', 'mean'):
    out['law_over_forces_' + key] = round(m['k_step_law'][key]/m['k_step_forces'][key], 4)
    out['forces_over_fly_' + key] = round(m['k_step_forces'][key]/m['k_fly'][key], 4)
print(json.dumps(out))
