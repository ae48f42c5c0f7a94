"""fb_batch_ray on the MI355X (csrc/fb_ray.hpp: k_raycast): the comparisons of tests/test_ray_emulation.py on live walking
environments, on both engine libraries and both precisions.  The reference, the acceptance rule and the tolerances are in
tests/ray_reference.py: FP64 batch 2^-22 relative, FP32 batch 4 x the emulation build's measured 3.2e-6."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu
N_ENV, STEPS = 4, 6


def _env(dense, precision, seed=0):
    """4 walking environments, six random-action control steps after a reset."""
    import torch
    from flybody_amd.fly_envs import BatchedFlyEnv
    env = BatchedFlyEnv(n_env=N_ENV, precision=precision, dense=dense, seed=seed)
    env.reset_all()
    gen = torch.Generator(device='cuda').manual_seed(seed)
    for _ in range(STEPS):
        env.step_tensor((2*torch.rand(N_ENV, env.model.dim('nact'), device='cuda', generator=gen) - 1).float().contiguous())
    torch.cuda.synchronize()
    return env, gen


@pytest.fixture(scope='module', params=[(False, 64), (True, 64), (False, 32), (True, 32)], ids=['default-fp64', 'dense-fp64', 'default-fp32', 'dense-fp32'])
def live(request):
    dense, precision = request.param
    env, _ = _env(dense, precision)
    b = env.batch
    return dict(env=env, precision=precision, a=env.model.arrays, gx=b.get('GEOM_XPOS'), gm=b.get('GEOM_XMAT'), xpos=b.get('XPOS'), xquat=b.get('XQUAT'),
                ngeom=env.model.dim('ngeom'), head=[str(n) for n in env.model.arrays['names_body']].index('head'))


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _np(r):
    return r.dist.cpu().numpy(), r.geomid.cpu().numpy()


def test_aimed_rays_and_eyes_match_the_reference(live):
    from flybody_amd import vision
    env, p, a = live['env'], live['precision'], live['a']
    assert (np.abs(live['gx'][0] - live['gx'][1]).max() > 1e-4)            # the random actions have taken the environments apart
    rays = np.stack([rr.aimed_rays(live['gx'][e], rr.body_geoms(a), 512, 200 + e) for e in range(N_ENV)])
    dist, gid = _np(env.cast_rays(_cuda(rays)))
    assert dist.shape == (N_ENV, 512)
    for e in range(N_ENV):
        share, err, hits = rr.compare(rr.Scene(a, live['gx'][e], live['gm'][e]), rays[e], dist[e], gid[e], p, verbose=f'FP{p} env {e}')
        print(f'FP{p} env {e}: {share:.2%} ambiguous, largest relative error {err:.3e}, {int((dist[e] < 0).sum())} misses')
    # the eyes, with the body in view: only the head's own geoms are hidden
    depth = env.eye_depth(size=8, see_body=True)
    assert tuple(depth.shape) == (N_ENV, 2, 8, 8)
    local = np.concatenate([vision.camera_rays(150.0, 8, 8, *pq) for pq in vision.EYES.values()])
    vis = np.asarray(a['geom_bodyid']) != live['head']
    r = env.cast_rays(_cuda(local), body=live['head'], geom_mask=vis)
    assert (r.dist.reshape(N_ENV, 2, 8, 8) == depth).all()
    dist, gid = _np(r)
    for e in range(N_ENV):
        world = rr.to_world(local, live['xpos'][e].reshape(-1, 3)[live['head']], live['xquat'][e].reshape(-1, 4)[live['head']])
        share, err, _ = rr.compare(rr.Scene(a, live['gx'][e], live['gm'][e], visible=vis), world, dist[e], gid[e], p, verbose=f'eyes FP{p} env {e}')
        print(f'eyes FP{p} env {e}: {share:.2%} ambiguous, largest relative error {err:.3e}, {int((dist[e] >= 0).sum())} of 128 hit')


@pytest.mark.parametrize('shape', [(5, 4), (33, 17)], ids=['5x4', '33x17'])
def test_terrain(live, shape):
    from flybody_amd import vision
    env, p = live['env'], live['precision']
    h, size, pos = rr.make_terrain(*shape, seed=shape[0])
    rays = rr.terrain_rays(size, pos, seed=shape[1])
    hidden = np.zeros(live['ngeom'], bool)
    T = vision.Terrain(np.stack([h, 1 - h]), size, pos)
    dist, gid = _np(env.cast_rays(_cuda(rays), env_ids=[1, 2], geom_mask=hidden, terrain=T, terrain_ids=[0, 1]))
    for f, hh in enumerate((h, 1 - h)):
        share, err, hits = rr.compare(rr.Scene(live['a'], live['gx'][0], live['gm'][0], visible=hidden, terrain=(hh, size, pos)), rays, dist[f], gid[f], p,
                                      verbose=f'terrain {shape} FP{p} grid {f}')
        print(f'terrain {shape} FP{p} grid {f}: {share:.2%} ambiguous, largest relative error {err:.3e}, {hits[-1]} hits')
        assert hits[-1] > 120 and set(gid[f]) <= {-1, live['ngeom']}
    # with the geoms in view the nearest hit wins
    rays = np.concatenate([rr.clear_of_terrain(rr.aimed_rays(live['gx'][3], rr.body_geoms(live['a']), 256, 9), h, (1.5, 0.9, 0.3, 0.5), (0, 0, -0.25)),
                           rr.terrain_rays((1.5, 0.9, 0.3, 0.5), (0, 0, -0.25), 4, n=8)])
    assert len(rays) > 200
    T = vision.Terrain(h, (1.5, 0.9, 0.3, 0.5), (0, 0, -0.25))
    dist, gid = _np(env.cast_rays(_cuda(rays), env_ids=[3], terrain=T))
    rr.compare(rr.Scene(live['a'], live['gx'][3], live['gm'][3], terrain=(h, T.size, T.pos)), rays, dist[0], gid[0], p, verbose='terrain and geoms')
    assert live['ngeom'] in gid[0] and 0 in gid[0] and len(set(gid[0])) > 10
    # the aimed rays as drawn, those that start next to the terrain included: the plain rule in FP64, with the absolute floor in FP32
    raw = rr.aimed_rays(live['gx'][3], rr.body_geoms(live['a']), 256, 9)
    dist, gid = _np(env.cast_rays(_cuda(raw), env_ids=[3], terrain=T))
    rr.compare(rr.Scene(live['a'], live['gx'][3], live['gm'][3], terrain=(h, T.size, T.pos)), raw, dist[0], gid[0], p, verbose='unfiltered',
               **({} if p == 64 else dict(abs_tol=rr.abs_bound(raw, 1.5))))


def test_two_calls_give_identical_bits(live):
    import torch
    from flybody_amd import vision
    env = live['env']
    T = vision.Terrain(*rr.make_terrain(33, 17, seed=3))
    rays = _cuda(np.stack([np.concatenate([rr.aimed_rays(live['gx'][e], rr.body_geoms(live['a']), 1500, e), rr.terrain_rays(T.size, T.pos, e)]) for e in range(N_ENV)]))
    a = env.cast_rays(rays, terrain=T)
    b = env.cast_rays(rays, terrain=T)
    torch.cuda.synchronize()
    assert torch.equal(a.dist, b.dist) and torch.equal(a.geomid, b.geomid) and int((a.geomid >= 0).sum()) > 3000


def test_eye_depth_over_a_flat_terrain(live):
    """eye_depth(32) with the fly hidden, over a flat terrain at height zt that covers the floor: the analytic plane distance, on
    every pixel that hits, away from the terrain's rim and from |d_z| < 1e-3 (where hit or miss is itself a matter of rounding)."""
    from flybody_amd import vision
    env, p = live['env'], live['precision']
    size, zt = (20.0, 20.0, 0.1, 0.05), 0.02
    T = vision.Terrain(np.full((3, 4), 0.7, np.float32), size, (0, 0, zt - 0.07))
    depth = env.eye_depth(size=32, terrain=T)
    assert tuple(depth.shape) == (N_ENV, 2, 32, 32) and str(depth.dtype) == 'torch.float32'
    depth = depth.cpu().numpy().reshape(N_ENV, -1)
    local = np.concatenate([vision.camera_rays(150.0, 32, 32, *pq) for pq in vision.EYES.values()])
    tol, checked = rr.RULES[p]['tol'], 0
    for e in range(N_ENV):
        w = rr.to_world(local, live['xpos'][e].reshape(-1, 3)[live['head']], live['xquat'][e].reshape(-1, 4)[live['head']])
        o, d = w[:, :3], w[:, 3:]
        assert (o[:, 2] > zt + 0.02).all()
        with np.errstate(divide='ignore'):
            t = (zt - o[:, 2])/d[:, 2]
        xy = o[:, :2] + t[:, None]*d[:, :2]
        hit = (d[:, 2] < 0) & (np.abs(xy) <= 20).all(axis=1)
        clear = (np.abs(np.abs(xy) - 20) > 0.1).all(axis=1) & (np.abs(d[:, 2]) > 1e-3)
        assert ((depth[e] >= 0) == hit)[clear].all() and (depth[e][clear & ~hit] == -1).all()
        # every hitting pixel: the distance is (zt - o_z) / d_z, and d_z -- three products and two sums of the rotation -- carries 4 roundings of
        # the batch's precision relative to |d| = 1, which move the distance by 4 eps / |d_z| of itself on top of the rule's own tolerance
        eps = 2.0**-52 if p == 64 else 2.0**-23
        chk = hit & clear
        bound = (tol + 4*eps/np.abs(d[:, 2]))*t
        assert chk.sum() > 700 and (np.abs(depth[e] - t)[chk] <= bound[chk]).all(), (np.abs(depth[e] - t)/bound)[chk].max()
        checked += int(chk.sum())
    print(f'FP{p}: {checked} eye pixels against the analytic plane distance')


@pytest.mark.parametrize('dense, precision', [(False, 64), (True, 32)])
def test_a_cast_changes_nothing_a_step_reads(dense, precision):
    import torch
    from flybody_amd import vision
    T = vision.Terrain(*rr.make_terrain(5, 4, seed=1))
    out = []
    for cast in (False, True):
        env, gen = _env(dense, precision, seed=5)
        before = [env.batch.get(f) for f in ('QPOS', 'QVEL')]
        if cast:
            r = env.cast_rays(_cuda(rr.aimed_rays(env.batch.get('GEOM_XPOS')[0], rr.body_geoms(env.model.arrays), 2000, 1)), terrain=T)
            env.eye_depth(size=16)
            assert int((r.geomid >= 0).sum()) > 1000
            assert all(np.array_equal(x, env.batch.get(f)) for x, f in zip(before, ('QPOS', 'QVEL')))
        env.step_tensor((2*torch.rand(N_ENV, env.model.dim('nact'), device='cuda', generator=gen) - 1).float().contiguous())
        torch.cuda.synchronize()
        out.append([env.batch.get(f) for f in ('QPOS', 'QVEL', 'OBS', 'REWARD', 'SENSORDATA', 'QACC')])
    for x, y in zip(*out):
        assert np.array_equal(x, y)
