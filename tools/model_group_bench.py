#!/usr/bin/env python3
"""Cost of per-environment models (fb_batch_create_group, the kernels k_group_step): env-steps/s of 4096 FP64
walk_imitation environments stepping ONE model (k_fly) against the same batch size stepping 8 variants of +-20 % in friction, mass,
gain and damping (flybody_amd.randomization.sample_models), fed the same seeded random actions.  The two batches do DIFFERENT physics
(that is the point of the variants), so the ratio holds the cost of binding the model per ticket AND whatever the variants' contact
configurations cost; `one_model_group` -- the grouped kernel on 8 copies of the nominal model, the same trajectories as the plain batch --
isolates the first.  Device events around every step, the batches alternated step by step.  One JSON line.

    python tools/model_group_bench.py [--envs 4096] [--models 8] [--steps 100] [--warmup 30] [--default-build] [--precision 64]
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
import torch
from flybody_amd import engine
from flybody_amd.randomization import sample_models
from flybody_amd.reference import default_walking_reference

ap = argparse.ArgumentParser()
ap.add_argument('--envs', type=int, default=4096); ap.add_argument('--models', type=int, default=8)
ap.add_argument('--steps', type=int, default=100); ap.add_argument('--warmup', type=int, default=30)
ap.add_argument('--default-build', action='store_true', help='libflybody_hip.so instead of the 12-per-CU build')
ap.add_argument('--precision', type=int, default=64)
a = ap.parse_args()
torch.cuda.set_device(0)
dense = not a.default_build and a.precision == 64
nominal = dict(engine.load_npz(os.path.join(engine.ASSETS, 'walk_imitation.npz')))
pm = (0.8, 1.2)
varied = sample_models(nominal, a.models, dict(friction_scale=pm, mass_scale=pm, gain_scale=pm, damping_scale=pm), seed=0)
models = dict(plain=engine.Model(nominal, dense=dense), one_model_group=engine.ModelGroup([nominal]*a.models, dense=dense),
              grouped=engine.ModelGroup(varied, dense=dense))
qp, qv = default_walking_reference()
st = torch.cuda.current_stream(); h = st.cuda_stream
batches = {}
for name, m in models.items():
    B = engine.Batch(m, a.envs, precision=a.precision)
    B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    batches[name] = B
assert batches['plain'].n_models == 1 and batches['grouped'].n_models == a.models
act = torch.empty(a.envs, models['plain'].dim('nact'), device='cuda')
ms = {name: [] for name in batches}
names = list(batches)
for k in range(a.warmup + a.steps):
    batches['plain'].random_actions(act.data_ptr(), k, seed=3, dist=1, stream=h)
    for name in names[k % 3:] + names[:k % 3]:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); batches[name].step_ptr(act.data_ptr(), h); e1.record(st)
        torch.cuda.synchronize()
        if k >= a.warmup:
            ms[name].append(e0.elapsed_time(e1))
same = all(np.array_equal(batches['plain'].get(f), batches['one_model_group'].get(f)) for f in ('QPOS', 'QVEL'))
stat = lambda x: dict(median=round(float(np.median(x)), 4), mean=round(float(np.mean(x)), 4), min=round(float(np.min(x)), 4))
rate = lambda x: round(a.envs/(float(np.mean(x))*1e-3))
out = dict(tool='model_group_bench', engine=engine.version(engine.HIP_LIB_DENSE if dense else None), envs=a.envs, models=a.models, precision=a.precision,
           steps=a.steps, substep_scheduler={n: batches[n].substep_scheduler for n in names}, one_model_group_same_trajectories=bool(same),
           warn_ever={n: int(np.bitwise_or.reduce(batches[n].get('WARN_EVER').ravel())) for n in names},
           ms_per_control_step={n: stat(v) for n, v in ms.items()}, env_steps_per_s={n: rate(v) for n, v in ms.items()})
out['ratio_grouped_over_plain'] = round(out['env_steps_per_s']['grouped']/out['env_steps_per_s']['plain'], 4)
out['ratio_one_model_group_over_plain'] = round(out['env_steps_per_s']['one_model_group']/out['env_steps_per_s']['plain'], 4)
print(json.dumps(out))
