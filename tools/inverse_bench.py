#!/usr/bin/env python3
"""Throughput of the batched inverse dynamics (fb_batch_inverse, csrc/fb_inverse.hpp) on one GPU, with a forward evaluation
(fb_batch_forward) of the same batch for scale.  `frames` walk_imitation environments after a seeded 30-step random-action rollout (the fly
on the floor: contacts, limits), FP64; the forward pass's qacc goes back in.  Device events around each call, best of `repeat`; the
inverse's time includes its host-side check of FB_QACC (a device-to-host copy of [frames][nv] reals) -- run it under
`rocprofv3 --kernel-trace --stats` for the k_inverse kernel time alone.  One JSON line.

    python tools/inverse_bench.py [--frames 4096] [--repeat 10] [--discrete] [--dense]
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
import torch
from flybody_amd import engine
from flybody_amd.reference import default_walking_reference

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=4096); ap.add_argument('--repeat', type=int, default=10)
ap.add_argument('--discrete', action='store_true'); ap.add_argument('--dense', action='store_true')
a = ap.parse_args()
torch.cuda.set_device(0)
model = engine.Model.from_asset('walk_imitation', dense=a.dense)
B = engine.Batch(model, a.frames, precision=64)
qp, qv = default_walking_reference()
B.set_reference(qp, qv, terminal_com_dist=float('inf')); B.reset()
act = torch.empty(a.frames, model.dim('nact'), device='cuda')
for k in range(30):
    B.random_actions(act.data_ptr(), k, seed=3, dist=1); B.step_ptr(act.data_ptr())
B.forward(); torch.cuda.synchronize()
st = torch.cuda.current_stream(); h = st.cuda_stream


def timed(fn):
    fn(); torch.cuda.synchronize()                   # warm-up
    ms = []
    for _ in range(a.repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); fn(); e1.record(st)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


inv = timed(lambda: B.inverse(discrete=a.discrete, stream=h))
fwd = timed(lambda: B.forward(stream=h))
nefc = B.get('NEFC')[:, 0]
ti, tf = min(inv) / 1e3, min(fwd) / 1e3
print(json.dumps(dict(tool='inverse_bench', engine=engine.version(engine.HIP_LIB_DENSE if a.dense else None), frames=a.frames,
                      discrete=a.discrete, nefc_mean=round(float(nefc.mean()), 1), nefc_max=int(nefc.max()),
                      inverse_ms=[round(x, 3) for x in inv], forward_ms=[round(x, 3) for x in fwd],
                      inverse_frames_per_s=round(a.frames / ti), forward_frames_per_s=round(a.frames / tf),
                      inverse_over_forward=round(ti / tf, 3))))
