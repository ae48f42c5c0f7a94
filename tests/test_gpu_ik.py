"""fb_batch_ik (multi-site inverse kinematics, csrc/fb_ik.hpp) on the MI355X: parity with the FP64 restatement of the reference algorithm
(tests/ik_reference.py), a 4096-frame round trip at the reference's defaults, chunking, the batch's later use, both engine binaries."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ik_reference as ikr  # noqa: E402

pytestmark = pytest.mark.gpu

# GPU vs restatement: FP64 sum-order differences only (the emulation build of the same kernel source stays within 8e-16 in qpos,
# tests/test_ik_emulation.py); three orders of magnitude of margin
TOL_QPOS = 1e-12
TOL_ERR = 1e-11
# Round trip: 4096 poses, leg hinges uniform in [lo/2, hi/2] of their ranges (default_rng(7)), fitted from qpos0 on the 12 leg sites /
# 66 leg hinges with the reference's defaults (lr 0.01, beta 0.99, progress_threshold 0.01, 20 000 steps).  The restatement on the
# first 512 of these seeds (tests/golden/ik_roundtrip_restatement.npy: err_norm, err_norm_first_term per frame) ends every frame at
# err_norm_first_term <= ROUNDTRIP_REF_MAX (median 5.0e-7; all 512 run the 20 000 steps: the criterion lr |update| / err grows as err
# shrinks); the bound for all 4096 frames is 10 x that maximum.  (Starting error at qpos0: 0.05 - 0.1.)
ROUNDTRIP_REF_MAX = 5.04e-5
ROUNDTRIP_BOUND = 10*ROUNDTRIP_REF_MAX


def _leg_setup(model):
    a = model.arrays
    names = [str(s) for s in a['names_site']]
    sites = [names.index(s) for s in names if s.startswith(('tarsus_', 'claw_'))]
    legs = [int(j) for j in a['leg_joints']]
    return sites, legs


def _targets(model, poses):
    from flybody_amd import engine
    B = engine.Batch(model, len(poses), precision=64)
    B.set('QPOS', poses); B.forward()
    sites, _ = _leg_setup(model)
    return B.get('SITE_XPOS').reshape(len(poses), -1, 3)[:, sites].copy()


def _poses(model, n, seed, scale=0.5):
    a = model.arrays
    _, legs = _leg_setup(model)
    lo, hi = a['jnt_range'][legs].T
    q = np.tile(a['qpos0'], (n, 1))
    q[:, a['jnt_qposadr'][legs]] = np.random.default_rng(seed).uniform(scale*lo, scale*hi, (n, len(legs)))
    return q


@pytest.fixture(scope='module')
def model():
    from flybody_amd import engine
    print('engine:', engine.version(), '| sources in tree:', engine.source_hash())
    return engine.Model.from_asset('walk_imitation')


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize('thr,max_steps,reg', [(0.0, 250, 1e-4), (0.1, 301, 0.0)])
def test_parity_with_restatement_64_frames(model, thr, max_steps, reg):
    from flybody_amd import engine
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    a = model.arrays
    sites, legs = _leg_setup(model)
    joints = [0] + legs
    T = _targets(model, _poses(model, 64, 3))
    B = engine.Batch(model, 64, precision=64)
    B.ik(sites, joints, T, reg_strength=reg, progress_threshold=thr, max_steps=max_steps)
    Q, E, S = B.get('QPOS'), B.get('IK_ERR'), B.get('IK_STEPS')
    od = fbo.OracleData(fbo.OracleModel(pack_model(a)))
    nsucc = 0
    for e in range(64):
        od.field('qpos')[:] = a['qpos0']
        q, err, first, steps, ok = ikr.qpos_from_site_xpos(od, a, sites, T[e], joints, reg_strength=reg, progress_threshold=thr, max_steps=max_steps)
        assert (int(S[e, 0]), int(S[e, 1])) == (steps, int(ok)), e
        assert np.abs(Q[e] - q).max() < TOL_QPOS, e
        assert _rel(E[e, 0], err) < TOL_ERR and _rel(E[e, 1], first) < TOL_ERR, e
        nsucc += int(ok)
    assert (nsucc == 0) if thr == 0 else (0 < nsucc < 64)


def test_round_trip_4096_frames_reference_defaults(model):
    from flybody_amd.inverse_kinematics import qpos_from_site_xpos
    a = model.arrays
    sites, legs = _leg_setup(model)
    poses = _poses(model, 4096, 7)
    T = _targets(model, poses)
    names_s = [str(a['names_site'][s]) for s in sites]; names_j = [str(a['names_jnt'][j]) for j in legs]
    r = qpos_from_site_xpos(model, names_s, T, names_j)
    print('round trip: err_norm_first_term max %.3e median %.3e, steps %s, success %d' % (r.err_norm_first_term.max(), np.median(r.err_norm_first_term),
                                                                                        np.unique(r.steps), r.success.sum()))
    assert np.all(np.isfinite(r.qpos))
    assert r.err_norm_first_term.max() < ROUNDTRIP_BOUND
    # ... and the frames the restatement ran end where it ended (20 000 FP64 iterations apart in summation order only)
    ref = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ik_roundtrip_restatement.npy'))
    n = len(ref)
    assert np.all(r.steps[:n] == 19999) and not r.success[:n].any()
    assert np.abs(r.err_norm_first_term[:n] - ref[:, 1]).max() <= 1e-6*ref[:, 1].max()
    assert np.abs(r.err_norm[:n] - ref[:, 0]).max() <= 1e-6*ref[:, 0].max()


def test_chunking_is_bit_identical(model):
    from flybody_amd.inverse_kinematics import qpos_from_site_xpos
    a = model.arrays
    sites, legs = _leg_setup(model)
    T = _targets(model, _poses(model, 2500, 5))
    names_s = [str(a['names_site'][s]) for s in sites]; names_j = [str(a['names_jnt'][j]) for j in [0] + legs]
    one = qpos_from_site_xpos(model, names_s, T, names_j, max_steps=400, progress_threshold=0.05)
    chunked = qpos_from_site_xpos(model, names_s, T, names_j, max_steps=400, progress_threshold=0.05, batch_size=1000)
    for f in one._fields:
        assert np.array_equal(getattr(one, f), getattr(chunked, f)), f


def test_batch_steps_after_ik(model):
    """IK leaves a batch that the physics can use: forward, then control steps, without warnings."""
    import torch
    from flybody_amd import engine
    from flybody_amd.reference import constant_speed_trajectory
    sites, legs = _leg_setup(model)
    n = 128
    B = engine.Batch(model, n, precision=64)
    qp, qv = constant_speed_trajectory(300, 2.0)
    B.set_reference(qp, qv, terminal_com_dist=float('inf'))
    B.reset()
    q = B.get('QPOS')
    T = _targets(model, _poses(model, n, 9)) + (q[:, None, :3] - model.arrays['qpos0'][:3])
    B.ik(sites, legs, T, max_steps=300)
    B.forward()
    act = torch.zeros(n, model.dim('nact'), device='cuda')
    for _ in range(3):
        B.step_ptr(act.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.all(np.isfinite(B.get('QPOS'))) and np.all(np.isfinite(B.get('QVEL')))
    assert not B.get('WARN_EVER').any()


def test_default_and_dense_binaries_agree(model):
    from flybody_amd import engine
    sites, legs = _leg_setup(model)
    T = _targets(model, _poses(model, 256, 13))
    out = []
    for dense in (False, True):
        M = engine.Model.from_asset('walk_imitation', dense=dense)
        B = engine.Batch(M, 256, precision=64)
        B.ik(sites, [0] + legs, T, reg_strength=1e-4, max_steps=500, progress_threshold=0.05)
        out.append((B.get('QPOS'), B.get('IK_ERR'), B.get('IK_STEPS'), B.get('SITE_XPOS')))
    for x, y in zip(*out):
        assert np.array_equal(x, y)
