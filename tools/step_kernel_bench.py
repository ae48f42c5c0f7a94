#!/usr/bin/env python3
"""Cost of the step kernels beside k_fly: ms per control step of walk_imitation batches of one size fed the same
seeded random actions, one batch per kernel:

    plain            k_fly
    forces           k_step_forces (csrc/fb_forces.hpp): the force arrays allocated and all zero
    law              k_step_law (csrc/fb_law.hpp): an all-zero law on top of them
    one_model_group  k_group_step on `models` copies of the nominal model (fb_batch_create_group)
    grouped          k_group_step on `models` variants of +-20 % in friction, mass, gain and damping (randomization.sample_models)

Zero forces, a zero law and copies of the nominal model give the plain batch's trajectories, so those batches do the same physics; what
differs is the applied-force stage and the sensor stage that reads xfrc_applied, the law stage, and binding the model per ticket.  The
varied group does DIFFERENT physics (that is the point of the variants): its ratio also holds whatever the variants' contact
configurations cost.  Device events around every step, the batches alternated step by step (the order rotates); median, mean and
minimum over `steps` control steps after `warmup`.  --only selects batches (the published figures of DESIGN.md 14 and 16 are runs of
plain,forces,law; those of 15 of plain,one_model_group,grouped).  One JSON line.

    python tools/step_kernel_bench.py [--envs 4096] [--models 8] [--steps 100] [--warmup 30] [--default-build] [--precision 64]
                                      [--only plain,forces,law]
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
import torch
from flybody_amd import engine
from flybody_amd.randomization import sample_models
from flybody_amd.reference import default_walking_reference

NAMES = ('plain', 'forces', 'law', 'one_model_group', 'grouped')
ap = argparse.ArgumentParser()
ap.add_argument('--envs', type=int, default=4096); ap.add_argument('--models', type=int, default=8)
ap.add_argument('--steps', type=int, default=100); ap.add_argument('--warmup', type=int, default=30)
ap.add_argument('--default-build', action='store_true', help='libflybody_hip.so instead of the 12-per-CU build')
ap.add_argument('--precision', type=int, default=64)
ap.add_argument('--only', default=','.join(NAMES), help='comma-separated subset of ' + ','.join(NAMES))
a = ap.parse_args()
names = [n for n in NAMES if n in a.only.split(',')]
assert 'plain' in names and set(a.only.split(',')) <= set(NAMES), '--only: plain and any of ' + ','.join(NAMES[1:])
torch.cuda.set_device(0)
dense = not a.default_build and a.precision == 64
nominal = dict(engine.load_npz(os.path.join(engine.ASSETS, 'walk_imitation.npz')))
pm = (0.8, 1.2)
model = engine.Model(nominal, dense=dense)
qp, qv = default_walking_reference()
st = torch.cuda.current_stream(); h = st.cuda_stream
batches = {}
for name in names:
    m = model
    if name == 'one_model_group':
        m = engine.ModelGroup([nominal]*a.models, dense=dense)
    if name == 'grouped':
        m = engine.ModelGroup(sample_models(nominal, a.models, dict(friction_scale=pm, mass_scale=pm, gain_scale=pm, damping_scale=pm), seed=0), dense=dense)
    B = engine.Batch(m, a.envs, precision=a.precision)
    B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
    if name == 'forces':
        B.set('XFRC_APPLIED', 0.0)
    if name == 'law':
        B.set_control_law()
    assert B.forces_active == (name in ('forces', 'law')) and B.control_law_active == (name == 'law')
    assert B.n_models == (a.models if name in ('one_model_group', 'grouped') else 1)
    batches[name] = B
act = torch.empty(a.envs, model.dim('nact'), device='cuda')
ms = {name: [] for name in names}
for k in range(a.warmup + a.steps):
    batches['plain'].random_actions(act.data_ptr(), k, seed=3, dist=1, stream=h)
    r = k % len(names)
    for name in names[r:] + names[:r]:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); batches[name].step_ptr(act.data_ptr(), h); e1.record(st)
        torch.cuda.synchronize()
        if k >= a.warmup:
            ms[name].append(e0.elapsed_time(e1))
same = lambda others: bool(all(np.array_equal(batches['plain'].get(f), batches[n].get(f)) for f in ('QPOS', 'QVEL') for n in others))
stat = lambda x: dict(median=round(float(np.median(x)), 4), mean=round(float(np.mean(x)), 4), min=round(float(np.min(x)), 4))
rate = lambda x: round(a.envs/(float(np.mean(x))*1e-3))
out = dict(tool='step_kernel_bench', engine=engine.version(engine.HIP_LIB_DENSE if dense else None), envs=a.envs, models=a.models, precision=a.precision,
           steps=a.steps, batches=names, substep_scheduler={n: batches[n].substep_scheduler for n in names},
           warn_ever={n: int(np.bitwise_or.reduce(batches[n].get('WARN_EVER').ravel())) for n in names},
           ms_per_control_step={n: stat(v) for n, v in ms.items()}, env_steps_per_s={n: rate(v) for n, v in ms.items()})
m = out['ms_per_control_step']
if 'forces' in names or 'law' in names:
    out['same_trajectories'] = same([n for n in ('forces', 'law') if n in names])
if 'one_model_group' in names:
    out['one_model_group_same_trajectories'] = same(['one_model_group'])
    out['ratio_one_model_group_over_plain'] = round(out['env_steps_per_s']['one_model_group']/out['env_steps_per_s']['plain'], 4)
if 'grouped' in names:
    out['ratio_grouped_over_plain'] = round(out['env_steps_per_s']['grouped']/out['env_steps_per_s']['plain'], 4)
for key in ('median', 'mean'):
    if 'forces' in names:
        out['forces_over_fly_' + key] = round(m['forces'][key]/m['plain'][key], 4)
    if 'forces' in names and 'law' in names:
        out['law_over_forces_' + key] = round(m['law'][key]/m['forces'][key], 4)
print(json.dumps(out))
