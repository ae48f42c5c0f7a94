#!/usr/bin/env python3
"""Time of Batch.cast_rays (fb_batch_ray, csrc/fb_ray.hpp) next to the control step it would follow, on one GPU.

    python tools/ray_bench.py [--n-env 4096] [--passes 3] [--reps 20] [--out FILE]

For an FP64 and an FP32 batch of walking environments on the 12-per-CU build, after 20 random-action control steps:
  (a) eye_depth(32) with the fly hidden, over a 401 x 401 sine-bump terrain      2 x 32 x 32 rays per environment, terrain + floor
  (b) the same with see_body=True                                                ... + the fly's geoms but the head's
  (c) 2048 world rays per environment aimed at the fly, all geoms visible
  (s) step_tensor, one control step with random actions
The cases are run in alternation, `passes` times, `reps` calls each between two device events; printed: every pass's ms per call, the
median's rays/s and its ratio to the same run's control step.  One JSON line at the end."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-env', type=int, default=4096)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from flybody_amd import vision
    from flybody_amd.fly_envs import BatchedFlyEnv
    assert torch.cuda.is_available(), 'ray_bench needs a GPU'
    n = args.n_env
    y, x = np.meshgrid(np.linspace(-1, 1, 401), np.linspace(-1, 1, 401), indexing='ij')
    terrain = vision.Terrain(0.5 + 0.5*np.sin(9*x)*np.sin(7*y), (4.0, 4.0, 0.05, 0.1), (0, 0, -0.02))
    result = {}
    for precision in (64, 32):
        env = BatchedFlyEnv(n_env=n, precision=precision, dense=True)
        nact = env.model.dim('nact')
        env.reset_all()
        gen = torch.Generator(device='cuda').manual_seed(0)
        action = lambda: (2*torch.rand(n, nact, device='cuda', generator=gen) - 1).float().contiguous()
        for _ in range(20):
            env.step_tensor(action())
        torch.cuda.synchronize()
        rng = np.random.default_rng(0)
        gx = env.batch.get('GEOM_XPOS').reshape(n, -1, 3)
        tgt = gx[np.arange(n)[:, None], rng.integers(1, gx.shape[1], (n, 2048))] + 0.02*rng.normal(size=(n, 2048, 3))
        u = rng.normal(size=(n, 2048, 3)); u /= np.linalg.norm(u, axis=-1, keepdims=True)
        world = torch.from_numpy(np.concatenate([tgt + 0.5*u, -0.5*u], -1)).cuda()
        acts = [action() for _ in range(args.reps)]
        cases = [('a eye_depth(32), fly hidden, terrain', 2048, lambda i: env.eye_depth(32, terrain=terrain)),
                 ('b eye_depth(32), see_body, terrain', 2048, lambda i: env.eye_depth(32, terrain=terrain, see_body=True)),
                 ('c 2048 world rays, all geoms', 2048, lambda i: env.cast_rays(world)),
                 ('s step_tensor (control step)', 0, lambda i: env.step_tensor(acts[i]))]
        hit = {k: float((f(0) >= 0).float().mean()) if k[0] in 'ab' else None for k, _, f in cases[:2]}
        hit[cases[2][0]] = float((cases[2][2](0).dist >= 0).float().mean())
        ms = {k: [] for k, _, _ in cases}
        for p in range(args.passes + 1):                     # (pass 0 warms every shape up)
            for k, _, f in cases:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(args.reps):
                    f(i)
                e1.record(); torch.cuda.synchronize()
                if p:
                    ms[k].append(e0.elapsed_time(e1)/args.reps)
        step = float(np.median(ms[cases[3][0]]))
        print(f'FP{precision}, {n} walking environments, {env.build}')
        for k, nr, _ in cases:
            med = float(np.median(ms[k]))
            tail = f'  {n*nr/med/1e3:9.0f} M rays/s  {med/step:5.2f} x the control step  {hit[k]:.0%} hit' if nr else ''
            print(f'  {k:40s} ' + ' '.join(f'{m:7.3f}' for m in ms[k]) + f' ms  median {med:7.3f}' + tail)
            result[f'fp{precision} {k}'] = dict(ms=ms[k], median_ms=med, rays_per_s=(n*nr/med*1e3 if nr else None), over_step=(med/step if nr else None))
        del env
    line = json.dumps(dict(n_env=n, reps=args.reps, passes=args.passes, cases=result))
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
