"""fb_batch_ray (csrc/fb_ray.hpp: k_raycast) through the kernel-source emulation build: the source the GPU runs, on the CPU.
No GPU needed.  The reference, the inputs, the acceptance rule and the tolerances -- with the measured FP32 error they come from -- are in
tests/ray_reference.py; tests/test_gpu_ray.py runs the same comparisons on the MI355X.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_reference as rr  # noqa: E402
from test_rollout_emulation import emu_lib  # noqa: E402,F401  (the emulation library's fixture)

TILE = 1024                     # FB_RAY_TILE: rays of one workgroup (csrc/fb_ray.hpp)
TYPES = {0: 'plane', 2: 'sphere', 3: 'capsule', 4: 'ellipsoid', 5: 'cylinder'}


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x))


def _np(r):
    return r.dist.numpy(), r.geomid.numpy()


class Walk:
    """The walking model at the four poses of ray_reference.walking_poses, as an FP64 and an FP32 batch; poses read back."""

    def __init__(self, lib, name='walk_imitation', poses=None):
        from flybody_amd import engine
        self.a = dict(engine.load_npz(os.path.join(engine.ASSETS, name + '.npz')))
        self.model = engine.Model(self.a, lib_path=lib)
        self.q = rr.walking_poses(self.a) if poses is None else poses(self.a)
        self.batch, self.gx, self.gm = {}, {}, {}
        for p in (64, 32):
            b = engine.Batch(self.model, len(self.q), precision=p)
            b.set('QPOS', self.q); b.forward()
            self.batch[p], self.gx[p], self.gm[p] = b, b.get('GEOM_XPOS'), b.get('GEOM_XMAT')
        self.ngeom = len(self.a['geom_type'])
        self.head = [str(n) for n in self.a['names_body']].index('head')

    def scene(self, p, e, **kw):
        return rr.Scene(self.a, self.gx[p][e], self.gm[p][e], **kw)

    def aimed(self, p, e, n=1024):
        return rr.aimed_rays(self.gx[p][e], rr.body_geoms(self.a), n, 100 + e)


@pytest.fixture(scope='module')
def walk(emu_lib):  # noqa: F811
    return Walk(emu_lib)


# ------------------------------------------------------------------ the comparison with the reference
@pytest.mark.parametrize('precision', [64, 32])
def test_aimed_rays_match_the_reference(walk, precision):
    """1024 aimed rays at each of the four poses; all five geom types are hit, at least 20 times each."""
    b = walk.batch[precision]
    per_type = dict.fromkeys(TYPES, 0)
    gtype = np.asarray(walk.a['geom_type'])
    for e in range(len(walk.q)):
        rays = walk.aimed(precision, e)
        dist, gid = _np(b.cast_rays(_t(rays), env_ids=[e]))
        share, err, hits = rr.compare(walk.scene(precision, e), rays, dist[0], gid[0], precision, verbose=f'FP{precision} pose {e}')
        print(f'FP{precision} pose {e}: {share:.2%} ambiguous, largest relative error {err:.3e}, {int((dist < 0).sum())} misses')
        for t in TYPES:
            per_type[t] += int(hits[:-1][gtype == t].sum())
    print({TYPES[t]: n for t, n in per_type.items()})
    assert all(n >= 20 for n in per_type.values()), per_type


@pytest.mark.parametrize('precision', [64, 32])
def test_walk_on_ball(emu_lib, precision):  # noqa: F811
    """Two spheres, no plane; at a jittered pose and at qpos0 (ray_reference's text: NEAR A SURFACE, FP32)."""
    w = Walk(emu_lib, 'walk_on_ball', poses=lambda a: np.array([rr.ball_pose(a), np.asarray(a['qpos0'], float)]))
    assert (np.asarray(w.a['geom_type']) == 0).sum() == 0 and (np.asarray(w.a['geom_type']) == 2).sum() == 2
    sphere = np.asarray(w.a['geom_type']) == 2
    for e in (0, 1):
        # the strict rule: on rays that keep clear of the ball (FP32), on the unfiltered draw (FP64); then FP32 on the unfiltered draw with the
        # absolute floor -- at qpos0, pose 1, that includes the claws' centres that lie on the ball
        for rays, kw in (((rr.ball_rays(w.a, w.gx[precision][e], 1024, 7), {}),) if precision == 32 else ()) + \
                        ((w.aimed(precision, e), {} if precision == 64 else dict(abs_tol=rr.abs_bound(w.aimed(precision, e), 0.9))),):
            dist, gid = _np(w.batch[precision].cast_rays(_t(rays), env_ids=[e]))
            share, err, hits = rr.compare(w.scene(precision, e), rays, dist[0], gid[0], precision, verbose=f'ball FP{precision} pose {e} {list(kw)}', **kw)
            print(f'ball FP{precision} pose {e} {list(kw)}: {share:.2%} ambiguous, largest relative error {err:.3e}')
            assert hits[:-1][sphere].sum() >= 20


# ------------------------------------------------------------------ shapes of the call
def test_ray_count_edges(walk):
    """n_ray of 1, 65, 257 and one more than a workgroup's tile: the same bits as those rays have in one large call, which is compared
    with the reference."""
    b, rays = walk.batch[64], walk.aimed(64, 1, TILE + 1)
    dist, gid = _np(b.cast_rays(_t(rays), env_ids=[1]))
    assert dist.shape == (1, TILE + 1) and dist.dtype == np.float32 and gid.dtype == np.int32
    rr.compare(walk.scene(64, 1), rays, dist[0], gid[0], 64, verbose='1025 rays')
    for n in (1, 65, 257):
        d, g = _np(b.cast_rays(_t(rays[:n]), env_ids=[1]))
        assert d.shape == (1, n) and np.array_equal(d[0], dist[0, :n]) and np.array_equal(g[0], gid[0, :n]), n


@pytest.mark.parametrize('precision', [64, 32])
def test_frames_env_ids_and_per_frame(walk, precision):
    b = walk.batch[precision]
    rays = np.stack([walk.aimed(precision, e, 96) for e in range(4)])
    one = [_np(b.cast_rays(_t(rays[e]), env_ids=[e])) for e in range(4)]
    # per_frame 1: a ray set per frame; env_ids permuted and repeated
    ids = [2, 0, 2]
    d, g = _np(b.cast_rays(_t(rays[ids]), env_ids=ids))
    assert d.shape == (3, 96)
    for f, e in enumerate(ids):
        assert np.array_equal(d[f], one[e][0][0]) and np.array_equal(g[f], one[e][1][0])
    # per_frame 0: one set, cast in every frame's environment; env_ids None: frame f is environment f
    d, g = _np(b.cast_rays(_t(rays[1])))
    assert d.shape == (4, 96) and np.array_equal(d[1], one[1][0][0]) and np.array_equal(g[1], one[1][1][0])
    for e, (de, ge) in enumerate(zip(*_np(b.cast_rays(_t(rays[1]), env_ids=[3, 1, 0])))):
        ref = _np(b.cast_rays(_t(rays[1]), env_ids=[[3, 1, 0][e]]))
        assert np.array_equal(de, ref[0][0]) and np.array_equal(ge, ref[1][0])
    d, g = _np(b.cast_rays(_t(rays[:1]), env_ids=[0]))          # n_frames 1, per_frame 1
    assert np.array_equal(d[0], one[0][0][0])


@pytest.mark.parametrize('precision', [64, 32])
def test_body_frame_rays(walk, precision):
    """Rays given in the head's frame against the same rays taken to the world frame with FB_XPOS / FB_XQUAT in numpy."""
    from flybody_amd import vision
    b, e = walk.batch[precision], 2
    local = np.concatenate([vision.camera_rays(150, 9, 9, *pq) for pq in vision.EYES.values()])
    local[:, 3:] *= 0.3                                           # (not unit length)
    xpos, xquat = b.get('XPOS')[e].reshape(-1, 3)[walk.head], b.get('XQUAT')[e].reshape(-1, 4)[walk.head]
    world = rr.to_world(local, xpos, xquat)
    vis = np.asarray(walk.a['geom_bodyid']) != walk.head            # (both eyes sit inside the head's geoms)
    dist, gid = _np(b.cast_rays(_t(local), body=walk.head, env_ids=[e], bodyexclude=walk.head))
    rr.compare(walk.scene(precision, e, visible=vis), world, dist[0], gid[0], precision, verbose='head frame')
    assert (dist >= 0).sum() > 40
    dw, gw = _np(b.cast_rays(_t(world), env_ids=[e], bodyexclude=walk.head))
    hit = (dist >= 0) & (dw >= 0)
    assert ((dist >= 0) == (dw >= 0)).mean() > 0.97 and np.allclose(dist[hit], dw[hit], rtol=4*rr.RULES[precision]['tol'], atol=0)


def test_eyes_are_inside_the_head(walk):
    """Why excluding and masking are part of the feature: with nothing hidden every eye ray ends on a geom of the fly."""
    from flybody_amd import vision
    local = np.concatenate([vision.camera_rays(150, 8, 8, *pq) for pq in vision.EYES.values()])
    dist, gid = _np(walk.batch[64].cast_rays(_t(local), body=walk.head))
    assert (gid > 0).all() and (np.asarray(walk.a['geom_bodyid'])[gid] != 0).all()


@pytest.mark.parametrize('precision', [64, 32])
def test_mask_exclude_and_cutoff(walk, precision):
    b, e = walk.batch[precision], 3
    rays = walk.aimed(precision, e, 512)
    gbody = np.asarray(walk.a['geom_bodyid'])
    mask = np.ones(walk.ngeom, bool); mask[1::3] = False
    thorax = [str(n) for n in walk.a['names_body']].index('thorax')
    for kw, vis in ((dict(geom_mask=mask), mask), (dict(bodyexclude=thorax), gbody != thorax),
                    (dict(geom_mask=mask, bodyexclude=thorax), mask & (gbody != thorax)),
                    (dict(geom_mask=np.zeros(walk.ngeom, bool)), np.zeros(walk.ngeom, bool))):
        dist, gid = _np(b.cast_rays(_t(rays), env_ids=[e], **kw))
        rr.compare(walk.scene(precision, e, visible=vis), rays, dist[0], gid[0], precision, verbose=str(list(kw)))
        assert vis[gid[0][gid[0] >= 0]].all()
    full = _np(b.cast_rays(_t(rays), env_ids=[e]))[0][0]
    cut = float(np.median(full[full >= 0]))*1.0001
    dist, gid = _np(b.cast_rays(_t(rays), env_ids=[e], cutoff=cut))
    rr.compare(walk.scene(precision, e), rays, dist[0], gid[0], precision, cutoff=cut, verbose='cutoff')
    assert 0 < (dist >= 0).sum() < (full >= 0).sum() and dist.max() <= cut
    for none in (None, 0.0, float('inf')):
        assert np.array_equal(_np(b.cast_rays(_t(rays), env_ids=[e], cutoff=none))[0][0], full)


@pytest.mark.parametrize('precision', [64, 32])
def test_degenerate_rays_and_the_floor(walk, precision):
    b = walk.batch[precision]
    good = np.array([0.5, 0.5, 1.0, 0, 0, -2.0])                  # onto the floor from z = 1: 0.5 in units of |dir|
    bad = [np.r_[good[:3], 0, 0, 0], np.r_[np.nan, good[1:]], np.r_[good[:5], np.nan], np.r_[good[:3], np.inf, 0, 0], np.r_[-np.inf, good[1:]],
           np.r_[good[:3], 1e-200, 0, -1e-200], np.r_[1e200, 0, 1, 0, 0, -1.0], np.r_[good[:3], 0, 0, -1e300], np.r_[good[:3], 0, 0, -1e-100]]
    rays = np.array([good] + bad + [good, np.r_[good[:3], 0, 0, -1e-15]])
    dist, gid = _np(b.cast_rays(_t(rays), env_ids=[0]))
    assert dist[0, 0] == dist[0, -2] == 0.5 and gid[0, 0] == gid[0, -2] == 0
    assert (dist[0, 1:-2] == -1).all() and (gid[0, 1:-2] == -1).all()   # (|dir|^2 under- or overflows; the distance 1e100 does not fit float32)
    assert np.isclose(dist[0, -1], 1e15, rtol=1e-6) and gid[0, -1] == 0          # a tiny direction is a ray like any other
    # the floor is 8 x 8 and finite; it is hit from its front only
    only_floor = np.arange(walk.ngeom) == 0
    assert np.asarray(walk.a['geom_type'])[0] == 0 and tuple(np.asarray(walk.a['geom_size'])[0][:2]) == (8.0, 8.0)
    rays = np.array([[7.5, 0, 1, 0, 0, -1.0], [8.5, 0, 1, 0, 0, -1.0], [6.5, 0, 1, 2.0, 0, -1.0], [0, -7.0, 2, 0, -0.4, -1.0], [0, -7.0, 2, 0, -0.6, -1.0],
                     [0.3, 0.2, -1, 0, 0, 1.0], [0.3, 0.2, -1, 0.1, 0, -1.0], [0.3, 0.2, 1, 1.0, 0, 0]])
    dist, gid = _np(b.cast_rays(_t(rays), env_ids=[0], geom_mask=only_floor))
    assert list(gid[0]) == [0, -1, -1, 0, -1, -1, -1, -1], gid
    assert np.allclose(dist[0, [0, 3]], [1, 2], rtol=1e-6) and (dist[0][gid[0] < 0] == -1).all()


# ------------------------------------------------------------------ terrain
def _terrain(h, size, pos):
    from flybody_amd import vision
    return vision.Terrain(h, size, pos, device='cpu')


@pytest.mark.parametrize('precision', [64, 32])
@pytest.mark.parametrize('shape', [(5, 4), (33, 17)], ids=['5x4', '33x17'])
def test_terrain_alone(walk, precision, shape):
    """Every family of rays of ray_reference.terrain_rays against the brute-force mesh; rows != columns, rx != ry, pos != 0, base_z > 0."""
    h, size, pos = rr.make_terrain(*shape, seed=shape[0])
    rays = rr.terrain_rays(size, pos, seed=shape[1])
    hidden = np.zeros(walk.ngeom, bool)
    dist, gid = _np(walk.batch[precision].cast_rays(_t(rays), env_ids=[0], geom_mask=hidden, terrain=_terrain(h, size, pos)))
    share, err, hits = rr.compare(walk.scene(precision, 0, visible=hidden, terrain=(h, size, pos)), rays, dist[0], gid[0], precision,
                                  verbose=f'terrain {shape} FP{precision}')
    print(f'terrain {shape} FP{precision}: {share:.2%} ambiguous, largest relative error {err:.3e}, {hits[-1]} hits, {int((dist < 0).sum())} misses')
    assert set(gid[0]) <= {-1, walk.ngeom}
    n = len(rays)//9                                              # the families: every one but the last hits, the last misses
    fam = (gid[0].reshape(9, n) == walk.ngeom).mean(axis=1)
    assert (fam[:8] > 0.5).all() and fam[[0, 2, 3, 6, 7]].min() > 0.9 and fam[8] == 0, fam


@pytest.mark.parametrize('precision', [64, 32])
def test_two_terrains_and_geoms(walk, precision):
    """terrain_ids (1, 0, 1) pick the frame's grid; with the fly's geoms visible the nearest hit wins."""
    b = walk.batch[precision]
    ha, size, _ = rr.make_terrain(5, 4, seed=1)
    hb, _, _ = rr.make_terrain(5, 4, seed=2)
    size, pos = (1.5, 0.9, 0.3, 0.5), (0.0, 0.0, -0.25)           # under the fly: the surface between z = -0.25 and 0.05 cuts the floor
    T = _terrain(np.stack([ha, hb]), size, pos)
    assert T.n_terrain == 2
    ids, envs = [1, 0, 1], [0, 3, 2]
    rays = np.stack([np.concatenate([rr.clear_of_terrain(walk.aimed(precision, e, 200), (ha, hb)[t], size, pos)[:140], rr.terrain_rays(size, pos, seed=e, n=8)])
                     for e, t in zip(envs, ids)])
    assert rays.shape == (3, 212, 6)
    dist, gid = _np(b.cast_rays(_t(rays), env_ids=envs, terrain=T, terrain_ids=ids))
    seen = set()
    for f, (e, t) in enumerate(zip(envs, ids)):
        sc = walk.scene(precision, e, terrain=((ha, hb)[t], size, pos))
        rr.compare(sc, rays[f], dist[f], gid[f], precision, verbose=f'frame {f}')
        seen |= set(gid[f])
    # the aimed rays as drawn, those that start next to the terrain included: the plain rule in FP64, with the absolute floor in FP32
    raw = walk.aimed(precision, envs[0], 200)
    d1, g1 = _np(b.cast_rays(_t(raw), env_ids=[envs[0]], terrain=T, terrain_ids=[ids[0]]))
    rr.compare(walk.scene(precision, envs[0], terrain=((ha, hb)[ids[0]], size, pos)), raw, d1[0], g1[0], precision, verbose='unfiltered',
               **({} if precision == 64 else dict(abs_tol=rr.abs_bound(raw, 1.5))))
    assert walk.ngeom in seen and 0 in seen and len(seen) > 10      # terrain, floor and body geoms all win somewhere
    d0, g0 = _np(b.cast_rays(_t(rays[0]), env_ids=[envs[0]], terrain=T))                  # terrain_ids None: grid 0
    rr.compare(walk.scene(precision, envs[0], terrain=(ha, size, pos)), rays[0], d0[0], g0[0], precision, verbose='grid 0')
    assert not np.array_equal(d0[0], dist[0])


# ------------------------------------------------------------------ order independence, refusals, purity
def test_reversed_lane_order_gives_the_same_bits(walk):
    T = _terrain(*rr.make_terrain(5, 4, seed=1))
    rays = np.concatenate([walk.aimed(32, 1, 300), rr.terrain_rays(T.size, T.pos, 3, n=6)])
    run = lambda: [_np(walk.batch[p].cast_rays(_t(rays), env_ids=[1, 2], terrain=T)) for p in (64, 32)]
    a = run()
    os.environ['FB_EMU_REVERSE'] = '1'
    try:
        b = run()
    finally:
        del os.environ['FB_EMU_REVERSE']
    for (da, ga), (db, gb) in zip(a, b):
        assert np.array_equal(da, db) and np.array_equal(ga, gb)


def test_refusals(walk, emu_lib):  # noqa: F811
    from flybody_amd import engine
    b = walk.batch[64]
    L, rays = b.L, _t(walk.aimed(64, 0, 8))
    nb = walk.model.dim('nbody')
    T = _terrain(*rr.make_terrain(5, 4, seed=1))

    def refused(what, **kw):
        with pytest.raises(engine.EngineError, match=what):
            b.cast_rays(rays, **kw)
    refused('environment id 4 out of range', env_ids=[0, 4])
    refused('environment id -1 out of range', env_ids=[-1])
    refused(f'body {nb} out of range', body=nb)
    refused('body -2 out of range', body=-2)
    refused(f'bodyexclude {nb} out of range', bodyexclude=nb)
    refused('cutoff must be >= 0', cutoff=-1.0)
    refused('cutoff must be >= 0', cutoff=float('nan'))
    refused('terrain id 1 out of range', terrain=T, terrain_ids=[0, 1, 0, 0])
    refused('terrain id -1 out of range', env_ids=[0], terrain=T, terrain_ids=[-1])
    for bad, what in ((dict(size=(0.0, 1, 1, 1)), 'terrain size must be'), (dict(size=(1, -1.0, 1, 1)), 'terrain size must be'),
                      (dict(size=(1, 1, -0.1, 1)), 'terrain size must be'), (dict(size=(1, 1, 1, -0.1)), 'terrain size must be'),
                      (dict(size=(1, 1, float('nan'), 1)), 'terrain size must be finite'), (dict(pos=(0, float('inf'), 0)), 'terrain pos must be finite')):
        Tb = _terrain(T.heights.numpy(), bad.get('size', T.size), bad.get('pos', T.pos))
        refused(what, terrain=Tb)
    # what the Python layer cannot express goes through the C-ABI itself
    dist, gid, ids5 = np.zeros(8, np.float32), np.zeros(8, np.int32), np.zeros(5, np.int32)

    def c_call(cfg=None, ter=None, rays_p=rays.data_ptr(), dist_p=dist.ctypes.data, gid_p=gid.ctypes.data, batch=b.h, **kw):
        c = engine._RayConfig(1, 8, 0, None, -1, -1, None, 0.0)
        for k, v in kw.items():
            setattr(c, k, v)
        rc = L.fb_batch_ray(batch, C.byref(c) if cfg is None else cfg, rays_p, ter, dist_p, gid_p, None)
        return rc, L.fb_last_error().decode()
    assert c_call() == (0, c_call()[1])
    for kw in (dict(batch=None), dict(cfg=C.c_void_p(None)), dict(rays_p=None), dict(dist_p=None), dict(gid_p=None)):
        rc, msg = c_call(**kw)
        assert rc != 0 and 'null argument' in msg, kw
    for kw, what in ((dict(n_frames=0), 'n_frames and n_ray must be >= 1'), (dict(n_ray=0), 'n_frames and n_ray must be >= 1'),
                     (dict(n_frames=-3), 'n_frames and n_ray must be >= 1'), (dict(per_frame=2), 'per_frame must be 0 or 1'),
                     (dict(n_frames=5), 'n_frames exceeds the batch'), (dict(n_ray=2**31 - 1, n_frames=5, env_ids=ids5.ctypes.data), 'too many rays')):
        rc, msg = c_call(**kw)
        assert rc != 0 and what in msg, (kw, msg)
    for kw, what in ((dict(nrow=1), 'nrow and ncol must be 2 .. 4096'), (dict(ncol=4097), 'nrow and ncol must be 2 .. 4096'),
                     (dict(n_terrain=0), 'n_terrain must be >= 1'), (dict(data=None), 'terrain data is NULL')):
        t = engine._Terrain(5, 4, 1, (C.c_double*4)(1, 1, 1, 1), (C.c_double*3)(0, 0, 0), T.heights.data_ptr(), None)
        for k, v in kw.items():
            setattr(t, k, v)
        rc, msg = c_call(ter=C.byref(t))
        assert rc != 0 and what in msg, (kw, msg)
    # a grouped batch of more than one model
    g = engine.Batch(engine.ModelGroup([walk.a, walk.a], lib_path=emu_lib), 2, precision=64)
    with pytest.raises(engine.EngineError, match='group of 2 models'):
        g.cast_rays(rays)
    # the Python layer's own checks
    with pytest.raises(ValueError, match='rays must be'):
        b.cast_rays(_t(np.zeros((3, 5))))
    with pytest.raises(ValueError, match='geom_mask must be'):
        b.cast_rays(rays, geom_mask=np.ones(3))
    with pytest.raises(ValueError, match='terrain_ids without a terrain'):
        b.cast_rays(rays, terrain_ids=[0])


@pytest.mark.parametrize('precision', [64, 32])
def test_a_cast_changes_nothing_a_step_reads(emu_lib, precision):  # noqa: F811
    """QPOS / QVEL and the bits of a following control step are the same with and without a cast in between -- with a control law set,
    which the call allows (it only reads poses)."""
    from flybody_amd import engine
    from flybody_amd.reference import constant_speed_trajectory
    a = dict(engine.load_npz(os.path.join(engine.ASSETS, 'walk_imitation.npz')))
    model = engine.Model(a, lib_path=emu_lib)
    qp, qv = constant_speed_trajectory(300, 2.0)
    act = np.random.default_rng(3).uniform(-0.5, 0.5, (2, 59)).astype(np.float32)
    T = _terrain(*rr.make_terrain(5, 4, seed=1))
    out = []
    for cast in (False, True):
        b = engine.Batch(model, 2, precision=precision)
        b.set_reference(qp, qv, terminal_com_dist=float('inf'))
        b.set_control_law(vel_gain=np.full(model.dim('nv'), 1e-4))
        b.reset()
        b.step_ptr(act.ctypes.data)
        before = [b.get(f) for f in ('QPOS', 'QVEL')]
        if cast:
            rays = rr.aimed_rays(b.get('GEOM_XPOS')[0], rr.body_geoms(a), 300, 1)
            r = b.cast_rays(_t(rays), terrain=T)
            assert (r.geomid.numpy() >= 0).any()
            assert all(np.array_equal(x, b.get(f)) for x, f in zip(before, ('QPOS', 'QVEL')))
        b.step_ptr(act.ctypes.data)
        out.append([b.get(f) for f in ('QPOS', 'QVEL', 'OBS', 'REWARD', 'SENSORDATA', 'QACC')])
    for x, y in zip(*out):
        assert np.array_equal(x, y)
