"""What the ray caster (engine.Batch.cast_rays, csrc/fb_ray.hpp) needs to make pictures: the rays of a pinhole camera, the
fly's two eye cameras, and a height-field terrain held on the device.  The eye cameras are not in the compiled assets; their poses are the
ones fruitfly.xml gives them on the `head` body.
"""
from __future__ import annotations

import collections

import numpy as np

# (pos, quat) in the head body's frame, in the order BatchedFlyEnv.eye_depth returns them
EYES = collections.OrderedDict([
    ('eye_right', ((0.0219, 0.0131, 0.0), (0.474, 0.688, -0.344, -0.429))),
    ('eye_left', ((-0.0219, 0.0131, 0.0), (0.474, 0.688, 0.344, 0.429)))])
EYE_FOVY, EYE_SIZE = 150.0, 32          # the vision task's camera settings


def quat_to_mat(quat) -> np.ndarray:
    """Rotation matrix of a quaternion (w, x, y, z), normalised first as MuJoCo's compiler does."""
    w, x, y, z = np.asarray(quat, np.float64)/np.linalg.norm(quat)
    return np.array([[w*w + x*x - y*y - z*z, 2*(x*y - w*z), 2*(x*z + w*y)],
                     [2*(x*y + w*z), w*w - x*x + y*y - z*z, 2*(y*z - w*x)],
                     [2*(x*z - w*y), 2*(y*z + w*x), w*w - x*x - y*y + z*z]])


def camera_rays(fovy: float, height: int, width: int, pos=(0, 0, 0), quat=(1, 0, 0, 0)) -> np.ndarray:
    """[height*width, 6] (origin, unit direction): the pinhole rays of a MuJoCo camera with vertical field of view `fovy` (degrees) at
    (pos, quat) in its parent body's frame, through the pixel centres, row 0 at the top, row-major.  The camera looks along its -z with
    +y up; pixels are square, so the horizontal field follows from the aspect ratio."""
    height, width = int(height), int(width)
    if height < 1 or width < 1 or not 0 < float(fovy) < 180:
        raise ValueError('camera_rays needs height, width >= 1 and 0 < fovy < 180 degrees')
    half = np.tan(np.deg2rad(float(fovy))/2)                                 # image-plane half height at distance 1
    ys = half*(1 - (2*np.arange(height) + 1)/height)                         # top row first
    xs = half*(width/height)*((2*np.arange(width) + 1)/width - 1)
    d = np.stack([np.broadcast_to(xs[None, :], (height, width)), np.broadcast_to(ys[:, None], (height, width)),
                  -np.ones((height, width))], -1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out = np.empty((height*width, 6))
    out[:, :3] = np.asarray(pos, np.float64)
    out[:, 3:] = d @ quat_to_mat(quat).T
    return out


class Terrain:
    """Height fields on the device, as MuJoCo's hfield asset: heights [n_terrain, nrow, ncol] (or [nrow, ncol]) in [0, 1], row <-> y,
    column <-> x; size = (rx, ry, elevation_z, base_z); pos: where the grid's centre sits in the world.  Sample (r, c) is at
    x = -rx + 2 rx c / (ncol - 1), y = -ry + 2 ry r / (nrow - 1) and has height elevation_z * heights[r, c].  `device`: a torch device
    (None: cuda:0 if there is one, else the CPU -- what the kernel-emulation build of the tests computes on)."""

    def __init__(self, heights, size, pos=(0.0, 0.0, 0.0), device=None):
        import torch
        h = np.asarray(heights, np.float32)
        if h.ndim == 2:
            h = h[None]
        if h.ndim != 3 or min(h.shape) < 1 or h.shape[1] < 2 or h.shape[2] < 2:
            raise ValueError('heights must be [n_terrain, nrow, ncol] with nrow, ncol >= 2')
        if not (np.isfinite(h).all() and h.min() >= 0 and h.max() <= 1):
            raise ValueError('heights must lie in [0, 1] (elevation_z scales them)')
        self.size = tuple(float(s) for s in size); self.pos = tuple(float(p) for p in pos)
        if len(self.size) != 4 or len(self.pos) != 3:
            raise ValueError('size is (rx, ry, elevation_z, base_z) and pos (x, y, z)')
        if device is None:
            device = 'cuda:0' if torch.cuda.is_available() else 'cpu'
        self.heights = torch.from_numpy(np.ascontiguousarray(h)).to(device)
        self.n_terrain, self.nrow, self.ncol = (int(s) for s in h.shape)

    def height_at(self, xy, terrain_ids=None):
        """World z of the surface at the sample NEAREST to the world points xy [..., 2] (a torch tensor on the terrain's device), per point's
        terrain terrain_ids [...] (None: terrain 0): the reference's get_hfield_height rule, with the y axis on its own grid.  Points
        outside the grid read the nearest edge sample; a point midway between two samples reads the lower index, as argmin does.  For reward and termination functions; the ray caster itself interpolates."""
        import torch
        rx, ry, ez, _ = self.size
        xy = torch.as_tensor(xy, device=self.heights.device)
        c = torch.ceil((xy[..., 0] - self.pos[0] + rx)/(2*rx)*(self.ncol - 1) - 0.5).clamp(0, self.ncol - 1).long()
        r = torch.ceil((xy[..., 1] - self.pos[1] + ry)/(2*ry)*(self.nrow - 1) - 0.5).clamp(0, self.nrow - 1).long()
        t = torch.zeros_like(c) if terrain_ids is None else torch.as_tensor(terrain_ids, device=self.heights.device).long().expand_as(c)
        return self.pos[2] + ez*self.heights[t, r, c].to(xy.dtype if xy.is_floating_point() else torch.float32)
