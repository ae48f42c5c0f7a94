"""flybody_amd.vision without any engine library: the pinhole rays of a MuJoCo camera, the eye poses, and Terrain.height_at."""
import re

import numpy as np
import pytest

from flybody_amd import vision


def test_camera_rays_geometry():
    pos, quat = (0.1, -0.2, 0.3), (0.5, -0.5, 0.5, 0.5)
    R = vision.quat_to_mat(quat)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and np.isclose(np.linalg.det(R), 1)
    fovy, h, w = 70.0, 5, 7
    rays = vision.camera_rays(fovy, h, w, pos, quat)
    assert rays.shape == (h*w, 6) and np.allclose(rays[:, :3], pos)
    d = rays[:, 3:].reshape(h, w, 3)
    assert np.allclose(np.linalg.norm(d, axis=-1), 1, atol=1e-15)                      # unit length
    assert np.allclose(d[h//2, w//2], -R[:, 2], atol=1e-15)                           # the centre of an odd image is the camera's -z
    loc = d @ R                                                                        # back in the camera's frame: x right, y up, -z ahead
    assert (loc[..., 2] < 0).all()
    assert (np.diff(loc[:, 0, 1]/-loc[:, 0, 2]) < 0).all() and (np.diff(loc[0, :, 0]/-loc[0, :, 2]) > 0).all()     # row 0 at the top, column 0 on the left
    # pixel CENTRES: the outermost rows sit half a pixel inside the field of view, and the corner's angle follows
    half = np.tan(np.deg2rad(fovy)/2)
    ty, tx = half*(1 - 1/h), half*(w/h)*(1 - 1/w)
    assert np.isclose(loc[0, 0, 1]/-loc[0, 0, 2], ty) and np.isclose(loc[0, 0, 0]/-loc[0, 0, 2], -tx)
    assert np.isclose(np.arccos(-loc[0, 0, 2]), np.arctan(np.hypot(tx, ty)))
    assert np.isclose(np.arccos(-loc[-1, -1, 2]), np.arccos(-loc[0, 0, 2]))
    # the vision task's camera: the top-centre pixel pair of a 32 x 32 image at fovy 150 looks 75 deg up less half a pixel
    e = vision.camera_rays(150, 32, 32).reshape(32, 32, 6)[..., 3:]
    assert np.isclose(e[0, 15, 1]/-e[0, 15, 2], np.tan(np.deg2rad(75))*(1 - 1/32))
    with pytest.raises(ValueError):
        vision.camera_rays(180, 4, 4)


def test_eyes_match_the_reference_model_file():
    from flybody_amd import model_zoo
    path = model_zoo.find_xml()
    if path is None:
        pytest.skip('the reference model file is not readable here')
    xml = open(path).read()
    assert list(vision.EYES) == ['eye_right', 'eye_left']
    for name, (pos, quat) in vision.EYES.items():
        m = re.search(r'<camera\s[^>]*name="%s"[^>]*>' % name, xml)
        assert m, name
        get = lambda k: tuple(float(x) for x in re.search(r'\b%s="([^"]*)"' % k, m.group(0)).group(1).split())
        assert get('pos') == pos and get('quat') == quat


def test_terrain_height_at_is_the_nearest_sample():
    import torch
    rng = np.random.default_rng(0)
    H = rng.uniform(0, 1, (2, 7, 5)).astype(np.float32)
    size, pos = (1.5, 0.7, 0.4, 0.1), (0.3, -0.2, 0.05)
    T = vision.Terrain(H, size, pos, device='cpu')
    assert (T.n_terrain, T.nrow, T.ncol) == (2, 7, 5) and T.heights.dtype == torch.float32
    xy = np.concatenate([rng.uniform(-2, 2, (400, 2)), [[pos[0] - 1.5, pos[1] - 0.7], [pos[0] + 1.5, pos[1] + 0.7], [pos[0], pos[1]]]])
    tid = rng.integers(0, 2, len(xy))
    xs, ys = pos[0] + np.linspace(-1.5, 1.5, 5), pos[1] + np.linspace(-0.7, 0.7, 7)      # the y axis on its own grid
    c = np.abs(xs[None, :] - xy[:, [0]]).argmin(1); r = np.abs(ys[None, :] - xy[:, [1]]).argmin(1)
    want = pos[2] + 0.4*H[tid, r, c].astype(np.float64)
    got = T.height_at(torch.from_numpy(xy), torch.from_numpy(tid))
    assert got.dtype == torch.float64 and np.allclose(got.numpy(), want, atol=1e-15)
    assert np.allclose(T.height_at(torch.from_numpy(xy)).numpy(), pos[2] + 0.4*H[0, r, c].astype(np.float64), atol=1e-15)
    assert T.height_at(torch.from_numpy(xy.reshape(13, 31, 2)), torch.from_numpy(tid.reshape(13, 31))).shape == (13, 31)
    assert vision.Terrain(H[0], size, device='cpu').n_terrain == 1
    for bad in (H[0, :1], H + 1, np.full((3, 3), np.nan)):
        with pytest.raises(ValueError):
            vision.Terrain(bad, size, device='cpu')
