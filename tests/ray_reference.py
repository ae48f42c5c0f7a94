"""An independent FP64 reference for fb_batch_ray (csrc/fb_ray.hpp), its inputs and its acceptance rule, shared by
tests/test_ray_emulation.py (kernel-source emulation build, no GPU) and tests/test_gpu_ray.py (MI355X).

REFERENCE.  Geoms: the textbook quadratic a t^2 + 2 b t + c = 0 per type in the geom's frame, with the geom poses READ BACK from the engine
(FB_GEOM_XPOS / FB_GEOM_XMAT); it returns EVERY geom's own distance.  Terrain: brute force over the closed triangle mesh of the solid --
surface, four walls, bottom -- with a two-sided Moeller-Trumbore test; no grid walk, no clipping.  Neither shares a formula with the kernel,
which solves its quadratics from the closest-approach vector and finds the surface by the sign of z - h(x, y) along a cell-by-cell walk.

ACCEPTANCE, per ray: hit or miss agrees; |dist - t*| <= tol; geomid is any geom whose reference distance is within 2 tol of the nearest
t* (overlapping fly geoms meet along curves where either id is right).

AMBIGUOUS rays are left out: those whose reference answer itself changes under a tilt of the direction by `tilt` radians (four tilts: +-
two perpendiculars) -- a different hit / miss, or a distance moved by more than `crit` relative.  The share left out is capped, and the
tests assert the cap:          tilt    crit    cap     the reference alone on the aimed rays below
    FP64 batch                 1e-6    1e-4    1 %     0.1 %
    FP32 batch                 3e-4    3e-2    5 %     2.1 %

TOLERANCES.  FP64 batch: tol = 2^-22 t*, derived: the output is float32 (rounding 2^-24), and FP64 arithmetic on rays whose conditioning
the tilt rule bounds is far below that.  FP32 batch: tol = FP32_TOL t*, four times the largest relative error of the emulation build's
FP32 results against this reference on the aimed rays of the four walking poses below, MEASURED at 3.11e-6 (per pose 7.9e-7, 2.7e-6,
3.1e-6, 1.8e-6; FP64 batch on the same rays: 5.8e-8, the float32 rounding of the output); the margin is for the GPU's fused multiply-adds,
which the x86 build does not contract the same way.

NEAR A SURFACE, FP32.  A float32 batch holds coordinates of size 0.5 .. 1.5 with a spacing of 6e-8 .. 1.2e-7, and the origin is rounded
to that before anything is computed, so a distance carries an ABSOLUTE error of that order however it is formed; against a tolerance
relative to t* that is 1.28e-5 only while t* stays above about 0.01.  The aimed rays of the four walking poses, which the tolerance was
measured on, have no ray that starts that close to what it meets.  walk_on_ball does: the ball has radius 0.454, the fly sits on it and
origins drawn 0.5 away land anywhere near its surface -- at qpos0 the claws' centres lie ON it to 7.5e-7 (measured FP32 error of the ray
from there: 0.9 % of t* = 2e-6; on the draw at the jittered pose: 1.5e-5 of t* = 0.003) -- and so does a terrain put under the fly
(measured on the MI355X: 6.8e-5 of t* = 3e-4, that is 1e-8 in length).  Two things are done about it, for FP32 batches only:
  * the strict relative rule is run on inputs that keep clear: ball_rays() redraws origins closer than 0.05 to the ball's surface,
    clear_of_terrain() drops fly-aimed rays that start within 0.05 of the terrain, terrain_rays() starts its inside-the-solid family
    mid-way through a thick base -- rules on the INPUT's geometry, never on a result;
  * the UNFILTERED draws are compared as well, with compare(abs_tol=abs_bound(...)): 16 float32 spacings of the largest coordinate
    involved (1.9e-6 at size 1) as a floor under the relative tolerance, and origins within that of the surface they meet counted as
    ambiguous, under the same cap.
FP64 batches run the unfiltered draws under the plain rule (walk_on_ball at qpos0: 5.9e-8).
"""
import numpy as np

PLANE, SPHERE, CAPSULE, ELLIPSOID, CYLINDER = 0, 2, 3, 4, 5
TOL64 = 2.0**-22
FP32_MEASURED = 3.2e-6
FP32_TOL = 4*FP32_MEASURED
RULES = {64: dict(tilt=1e-6, crit=1e-4, cap=0.01, tol=TOL64), 32: dict(tilt=3e-4, crit=3e-2, cap=0.05, tol=FP32_TOL)}


# ------------------------------------------------------------------ geoms
def _roots(a, b, c):
    """Both roots of a t^2 + 2 b t + c = 0 per ray, ascending; NaN where there is none."""
    with np.errstate(invalid='ignore', divide='ignore'):
        disc = b*b - a*c
        s = np.sqrt(np.where(disc >= 0, disc, np.nan))
        return (-b - s)/a, (-b + s)/a


def _first(*cands):
    """Smallest candidate >= 0 per ray (inf: none); NaN candidates are ignored."""
    t = np.stack(cands)
    t = np.where(np.isfinite(t) & (t >= 0), t, np.inf)
    return t.min(axis=0)


def geom_distances(o, d, gtype, gsize, gxpos, gxmat):
    """[n_ray, ngeom]: the smallest x >= 0 with o + x d on the boundary of every geom (inf: none).  o, d: [n_ray, 3] world frame."""
    n, ng = len(o), len(gtype)
    out = np.full((n, ng), np.inf)
    for g in range(ng):
        R = np.asarray(gxmat[g], float).reshape(3, 3)
        p = (o - gxpos[g]) @ R            # local = R^T (o - c)
        v = d @ R
        sz = gsize[g]
        with np.errstate(invalid='ignore', divide='ignore'):
            if gtype[g] == PLANE:
                t = -p[:, 2]/v[:, 2]
                x, y = p[:, 0] + t*v[:, 0], p[:, 1] + t*v[:, 1]
                ok = (v[:, 2] < 0) & (t >= 0)
                if sz[0] > 0:
                    ok &= np.abs(x) <= sz[0]
                if sz[1] > 0:
                    ok &= np.abs(y) <= sz[1]
                out[:, g] = np.where(ok, t, np.inf)
            elif gtype[g] in (SPHERE, ELLIPSOID):
                s = np.array([sz[0]]*3) if gtype[g] == SPHERE else sz
                ps, vs = p/s, v/s
                out[:, g] = _first(*_roots((vs*vs).sum(1), (ps*vs).sum(1), (ps*ps).sum(1) - 1))
            else:
                r, h = sz[0], sz[1]
                cands = []
                for t in _roots((v[:, :2]**2).sum(1), (p[:, :2]*v[:, :2]).sum(1), (p[:, :2]**2).sum(1) - r*r):
                    cands.append(np.where(np.abs(p[:, 2] + t*v[:, 2]) <= h, t, np.nan))
                for ze in (-h, h):
                    if gtype[g] == CYLINDER:
                        t = (ze - p[:, 2])/v[:, 2]
                        q = p[:, :2] + t[:, None]*v[:, :2]
                        cands.append(np.where((q*q).sum(1) <= r*r, t, np.nan))
                    else:
                        pc = p - np.array([0, 0, ze])
                        for t in _roots((v*v).sum(1), (pc*v).sum(1), (pc*pc).sum(1) - r*r):
                            z = pc[:, 2] + t*v[:, 2]
                            cands.append(np.where(z*np.sign(ze) >= 0, t, np.nan))
                out[:, g] = _first(*cands)
    return out


# ------------------------------------------------------------------ terrain
def terrain_mesh(heights, size, pos):
    """[n_tri, 3, 3]: the closed surface of the solid {|x| <= rx, |y| <= ry, -base <= z <= h(x, y)} at `pos`: every cell's triangles
    (v00, v11, v10) and (v00, v11, v01), the four walls down to -base, the bottom."""
    H = np.asarray(heights, np.float64)
    nrow, ncol = H.shape
    rx, ry, ez, base = size
    xs = -rx + 2*rx*np.arange(ncol)/(ncol - 1); ys = -ry + 2*ry*np.arange(nrow)/(nrow - 1)
    V = lambda r, c: np.array([xs[c], ys[r], ez*H[r, c]])
    B = lambda r, c: np.array([xs[c], ys[r], -base])
    tri = []
    for r in range(nrow - 1):
        for c in range(ncol - 1):
            tri += [(V(r, c), V(r + 1, c + 1), V(r + 1, c)), (V(r, c), V(r + 1, c + 1), V(r, c + 1))]
    edge = [((r, 0), (r + 1, 0)) for r in range(nrow - 1)] + [((r, ncol - 1), (r + 1, ncol - 1)) for r in range(nrow - 1)] + \
           [((0, c), (0, c + 1)) for c in range(ncol - 1)] + [((nrow - 1, c), (nrow - 1, c + 1)) for c in range(ncol - 1)]
    for a, b in edge:
        tri += [(B(*a), B(*b), V(*b)), (B(*a), V(*b), V(*a))]
    tri += [(B(0, 0), B(0, ncol - 1), B(nrow - 1, ncol - 1)), (B(0, 0), B(nrow - 1, ncol - 1), B(nrow - 1, 0))]
    return np.array(tri) + np.asarray(pos, float)


def mesh_distance(o, d, tri):
    """[n_ray]: the smallest x >= 0 at which o + x d crosses any triangle, from either side (inf: none)."""
    a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    out = np.full(len(o), np.inf)
    with np.errstate(invalid='ignore', divide='ignore'):
        for k in range(len(o)):
            pv = np.cross(d[k], e2)
            det = (e1*pv).sum(1)
            tv = o[k] - a
            u = (tv*pv).sum(1)/det
            qv = np.cross(tv, e1)
            v = (qv*d[k]).sum(1)/det
            t = (e2*qv).sum(1)/det
            ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0)
            if ok.any():
                out[k] = t[ok].min()
    return out


# ------------------------------------------------------------------ the whole reference, the tilt rule, the comparison
class Scene:
    """What a frame's rays can meet: the model's geoms at the poses read back from the engine (visible: bool [ngeom]) and an optional
    terrain (heights [nrow, ncol], size, pos)."""

    def __init__(self, arrays, gxpos, gxmat, visible=None, terrain=None):
        self.gtype = np.asarray(arrays['geom_type']); self.gsize = np.asarray(arrays['geom_size'], float)
        self.gxpos = np.asarray(gxpos, float).reshape(-1, 3); self.gxmat = np.asarray(gxmat, float).reshape(-1, 9)
        self.ngeom = len(self.gtype)
        self.visible = np.ones(self.ngeom, bool) if visible is None else np.asarray(visible, bool)
        self.mesh = None if terrain is None else terrain_mesh(*terrain)

    def distances(self, o, d):
        """[n_ray, ngeom + 1]: every object's own distance (the last column: the terrain), inf for a miss or a hidden geom."""
        t = geom_distances(o, d, self.gtype, self.gsize, self.gxpos, self.gxmat)
        t[:, ~self.visible] = np.inf
        tt = np.full(len(o), np.inf) if self.mesh is None else mesh_distance(o, d, self.mesh)
        return np.concatenate([t, tt[:, None]], 1)


def perpendiculars(d):
    a = np.where(np.abs(d[:, [0]]) < 0.6*np.linalg.norm(d, axis=1, keepdims=True), [[1.0, 0, 0]], [[0, 1.0, 0]])
    p1 = np.cross(d, a); p1 /= np.linalg.norm(p1, axis=1, keepdims=True)
    p2 = np.cross(d, p1); p2 /= np.linalg.norm(p2, axis=1, keepdims=True)
    return p1, p2


def ambiguous(scene, o, d, tstar, tilt, crit, cutoff=None):
    """bool [n_ray]: the reference's own answer changes under a tilt of the direction."""
    L = np.linalg.norm(d, axis=1, keepdims=True)
    p1, p2 = perpendiculars(d)
    amb = np.zeros(len(o), bool)
    for p in (p1, -p1, p2, -p2):
        dt = d + np.tan(tilt)*L*p
        dt *= L/np.linalg.norm(dt, axis=1, keepdims=True)
        t = scene.distances(o, dt).min(axis=1)
        if cutoff is not None:
            t = np.where(t > cutoff, np.inf, t)
        hit, hit0 = np.isfinite(t), np.isfinite(tstar)
        with np.errstate(invalid='ignore'):
            amb |= (hit != hit0) | (hit & hit0 & (np.abs(t - tstar) > crit*tstar))
    return amb


def compare(scene, rays, dist, geomid, precision, cutoff=None, verbose='', abs_tol=None):
    """Assert the acceptance rule on every unambiguous ray; returns (share left out, largest relative distance error, hits per object).
    abs_tol (a LENGTH; abs_bound() gives it): the near-surface rule of the module text -- the tolerance of a ray is then the larger of the
    relative one and abs_tol / |dir|, and a ray whose origin lies within abs_tol of the surface it meets is ambiguous."""
    rule = RULES[precision]
    rays = np.asarray(rays, float); o, d = rays[:, :3], rays[:, 3:]
    dist = np.asarray(dist, float); geomid = np.asarray(geomid)
    T = scene.distances(o, d)
    tstar = T.min(axis=1)
    if cutoff is not None:
        amb_cut = np.abs(tstar - cutoff) <= 4*rule['tol']*cutoff
        T = np.where(T > cutoff, np.inf, T); tstar = T.min(axis=1)
    amb = ambiguous(scene, o, d, tstar, rule['tilt'], rule['crit'], cutoff)
    if cutoff is not None:
        amb |= amb_cut
    if abs_tol is not None:
        amb |= tstar*np.linalg.norm(d, axis=1) < abs_tol
    keep = ~amb
    share = amb.mean()
    hit = np.isfinite(tstar)
    got_hit = dist >= 0
    bad = keep & (hit != got_hit)
    assert not bad.any(), f'{verbose}: hit / miss differs on rays {np.flatnonzero(bad)[:8]}: ref {tstar[bad][:8]} got {dist[bad][:8]} id {geomid[bad][:8]}'
    assert (geomid[~got_hit] == -1).all() and (dist[~got_hit] == -1).all(), f'{verbose}: a miss is dist -1, geomid -1'
    k = keep & hit
    tol = rule['tol']*tstar
    if abs_tol is not None:
        tol = np.maximum(tol, abs_tol/np.linalg.norm(d, axis=1))
    with np.errstate(invalid='ignore'):
        err = np.where(k, np.abs(dist - tstar)/np.where(k, tstar, 1), 0)
    worst = int(np.where(k, np.abs(dist - np.where(k, tstar, 0)) - np.where(k, tol, 0), -np.inf).argmax())
    assert (np.abs(dist - tstar)[k] <= tol[k]).all(), f'{verbose}: ray {worst} dist {dist[worst]!r} ref {tstar[worst]!r} rel {err[worst]:.3e} > {rule["tol"]:.3e} (geom {geomid[worst]})'
    idx = np.flatnonzero(k)
    gid = geomid[idx]
    assert ((gid >= 0) & (gid <= scene.ngeom)).all(), f'{verbose}: geomid out of range'
    own = T[idx, gid]
    badid = ~(own <= tstar[idx] + 2*tol[idx])
    assert not badid.any(), f'{verbose}: geomid of rays {idx[badid][:8]}: got {gid[badid][:8]} at {own[badid][:8]}, nearest {tstar[idx][badid][:8]}'
    assert share <= rule['cap'], f'{verbose}: {share:.3%} of the rays are ambiguous, cap {rule["cap"]:.0%}'
    return share, float(err.max()), np.bincount(gid, minlength=scene.ngeom + 1)


# ------------------------------------------------------------------ inputs
def walking_poses(arrays, seed=5):
    """qpos [4, nq]: qpos0, and three poses with a random root attitude and joints jittered by 0.2 rad at root heights 0.13 / 0.2 / 0.5."""
    rng = np.random.default_rng(seed)
    q0 = np.asarray(arrays['qpos0'], float)
    out = [q0.copy()]
    for z in (0.13, 0.2, 0.5):
        q = q0.copy()
        q[2] = z
        quat = rng.normal(size=4); q[3:7] = quat/np.linalg.norm(quat)
        q[7:] += 0.2*rng.normal(size=len(q) - 7)
        out.append(q)
    return np.array(out)


def abs_bound(rays, extent):
    """16 float32 spacings of the largest coordinate a ray's arithmetic meets: its origin's, or `extent`, the size of what it is cast at."""
    return 16*float(np.spacing(np.float32(max(np.abs(np.asarray(rays, float)[:, :3]).max(), extent))))


def ball_pose(arrays, seed=9):
    """walk_on_ball's qpos0 with every hinge jittered by 0.2 rad (see the module text for why not qpos0 itself)."""
    rng = np.random.default_rng(seed)
    q = np.asarray(arrays['qpos0'], float).copy()
    adr = np.asarray(arrays['jnt_qposadr'])[np.asarray(arrays['jnt_type']) == 3]
    q[adr] += 0.2*rng.normal(size=len(adr))
    return q


def aimed_rays(gxpos, body_geoms, n, seed):
    """[n, 6]: each ray starts 0.5 away in a random direction from a point drawn 0.02 (normal) around a random body geom's centre and
    points at that point (|dir| = 0.5: distances are in units of it); every eighth ray starts AT a geom's centre instead, in a random
    direction -- the inside case."""
    rng = np.random.default_rng(seed)
    gxpos = np.asarray(gxpos, float).reshape(-1, 3)
    g = rng.choice(body_geoms, n)
    target = gxpos[g] + 0.02*rng.normal(size=(n, 3))
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    rays = np.concatenate([target + 0.5*u, -0.5*u], 1)
    inside = np.arange(n) % 8 == 7
    rays[inside, :3] = gxpos[g[inside]]
    return rays


def ball_rays(arrays, gxpos, n, seed, clear=0.05):
    """aimed_rays for walk_on_ball, keeping the first n whose origin is at least `clear` away from the ball's surface (module text)."""
    gxpos = np.asarray(gxpos, float).reshape(-1, 3)
    ball = [str(s) for s in arrays['names_geom']].index('ball')
    rays = aimed_rays(gxpos, body_geoms(arrays), 3*n, seed)
    gap = np.abs(np.linalg.norm(rays[:, :3] - gxpos[ball], axis=1) - np.asarray(arrays['geom_size'])[ball, 0])
    rays = rays[gap >= clear]
    assert len(rays) >= n
    return rays[:n]


def surface_height(heights, size, x, y):
    """h(x, y) of the terrain's surface in its own frame (x, y clamped into the grid): the triangles (v00, v11, v10) and (v00, v11, v01)."""
    H = np.asarray(heights, float); nrow, ncol = H.shape
    rx, ry, ez, _ = size
    fx = np.clip((np.asarray(x, float) + rx)/(2*rx)*(ncol - 1), 0, ncol - 1); fy = np.clip((np.asarray(y, float) + ry)/(2*ry)*(nrow - 1), 0, nrow - 1)
    c = np.minimum(fx.astype(int), ncol - 2); r = np.minimum(fy.astype(int), nrow - 2)
    u, v = fx - c, fy - r
    h00, h01, h10, h11 = H[r, c], H[r, c + 1], H[r + 1, c], H[r + 1, c + 1]
    return ez*np.where(v >= u, h00 + u*(h11 - h10) + v*(h10 - h00), h00 + u*(h01 - h00) + v*(h11 - h01))


def clear_of_terrain(rays, heights, size, pos, clear=0.05):
    """The rays whose origin is not within `clear` of the solid's boundary (twice that vertically: the surface slopes) -- the rule on FP32
    inputs of the module text, applied to rays that were aimed at the fly without regard to the terrain."""
    o = np.asarray(rays, float)[:, :3] - np.asarray(pos, float)
    rx, ry, ez, base = size
    near_box = (np.abs(o[:, 0]) <= rx + clear) & (np.abs(o[:, 1]) <= ry + clear) & (o[:, 2] >= -base - clear) & (o[:, 2] <= ez + 2*clear)
    gap = np.minimum.reduce([np.abs(o[:, 2] - surface_height(heights, size, o[:, 0], o[:, 1]))/2, np.abs(np.abs(o[:, 0]) - rx),
                             np.abs(np.abs(o[:, 1]) - ry), np.abs(o[:, 2] + base)])
    return rays[~(near_box & (gap < clear))]


def body_geoms(arrays):
    """Geoms that are not on the world body (the floor is)."""
    return np.flatnonzero(np.asarray(arrays['geom_bodyid']) != 0)


def quat_rotate(q, v):
    w, x, y, z = q
    R = np.array([[w*w + x*x - y*y - z*z, 2*(x*y - w*z), 2*(x*z + w*y)], [2*(x*y + w*z), w*w - x*x + y*y - z*z, 2*(y*z - w*x)],
                  [2*(x*z - w*y), 2*(y*z + w*x), w*w - x*x - y*y + z*z]])
    return np.asarray(v, float) @ R.T


def to_world(rays, xpos, xquat):
    """Body-frame rays [n, 6] as world-frame rays, through the body's pose (FB_XPOS / FB_XQUAT rows of one body)."""
    rays = np.asarray(rays, float)
    return np.concatenate([xpos + quat_rotate(xquat, rays[:, :3]), quat_rotate(xquat, rays[:, 3:])], 1)


# terrains of the tests: (heights, size, pos); rows != columns catches a transposed index, rx != ry, pos != 0, base_z > 0
def make_terrain(nrow, ncol, seed):
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(0, 1, nrow), np.linspace(0, 1, ncol), indexing='ij')
    h = 0.5 + 0.25*np.sin(5*x + 1)*np.cos(4*y) + 0.2*rng.uniform(-1, 1, (nrow, ncol))
    return np.clip(h, 0, 1).astype(np.float32), (1.5, 0.9, 0.4, 0.6), (0.3, -0.2, -0.1)



def terrain_rays(size, pos, seed, n=24):
    """World rays of every family of the issue, n each: from above, from the side (walls), from below (bottom), from inside the solid,
    parallel to a grid axis, exactly vertical, missing the box."""
    rng = np.random.default_rng(seed)
    rx, ry, ez, base = size
    pos = np.asarray(pos, float)
    U = lambda lo, hi, *s: rng.uniform(lo, hi, s)
    inbox = lambda z: np.stack([U(-rx, rx, n), U(-ry, ry, n), z], 1)
    out = []
    o = inbox(U(ez + 0.3, ez + 1, n)); t = inbox(U(-base, ez, n)); out.append(np.concatenate([o, t - o], 1))                      # from above
    ang = U(0, 2*np.pi, n); o = np.stack([3*rx*np.cos(ang), 3*ry*np.sin(ang), U(-base, ez + 0.2, n)], 1)
    t = inbox(U(-base, ez, n)); out.append(np.concatenate([o, t - o], 1))                                                        # from the side
    o = inbox(U(-base - 1, -base - 0.2, n)); t = inbox(U(-base, ez, n)); out.append(np.concatenate([o, t - o], 1))                  # from below
    o = inbox(U(-0.65*base, -0.35*base, n))*[0.8, 0.8, 1]; u = rng.normal(size=(n, 3)); out.append(np.concatenate([o, u], 1))   # from inside the solid (z < 0 <= h), away from its faces
    o = np.stack([np.full(n, -2*rx), U(-ry, ry, n), U(0, ez, n)], 1); out.append(np.concatenate([o, np.tile([1.0, 0, 0], (n, 1))], 1))   # along x
    o = np.stack([U(-rx, rx, n), np.full(n, 2*ry), U(0, ez, n)], 1); out.append(np.concatenate([o, np.tile([0, -2.0, 0], (n, 1))], 1))   # along -y
    o = inbox(U(ez + 0.1, ez + 1, n)); out.append(np.concatenate([o, np.tile([0, 0, -1.0], (n, 1))], 1))                          # exactly vertical, down
    o = inbox(U(-base - 1, -base - 0.1, n)); out.append(np.concatenate([o, np.tile([0, 0, 3.0], (n, 1))], 1))                     # ... and up
    o = np.stack([U(2*rx, 3*rx, n), U(-ry, ry, n), U(ez + 0.5, ez + 1, n)], 1); out.append(np.concatenate([o, np.tile([0.1, 0.3, 1.0], (n, 1))], 1))  # missing the box
    rays = np.concatenate(out)
    rays[:, :3] += pos
    return rays

