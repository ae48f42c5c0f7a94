"""Batch.device_view on the MI355X: the zero-copy torch tensor over a device field has the dtype, shape and strides that the field table and
the batch give, and holds what Batch.get copies out -- the default build, 3 environments (odd and above 1, so a wrong row stride shows),
FP64 and FP32."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 3


@pytest.fixture(scope='module')
def model():
    from flybody_amd import engine
    return engine.Model.from_asset('walk_imitation')


def _batch(model, precision, reference_traj):
    from flybody_amd import engine
    B = engine.Batch(model, N, precision=precision)
    B.set_reference(*reference_traj, terminal_com_dist=float('inf')); B.reset()
    return B


def _step(B):
    import torch
    act = torch.from_numpy(np.random.default_rng(0).uniform(-0.5, 0.5, (N, 59)).astype(np.float32)).cuda()
    B.step_ptr(act.data_ptr(), torch.cuda.current_stream().cuda_stream); torch.cuda.synchronize()


def _real(precision):
    return np.float64 if precision == 64 else np.float32


def _same_bits(view, got):
    """The view's content, copied to the host, and get()'s array cast to the view's dtype: the same bytes."""
    v = view.cpu().numpy()
    assert v.shape == got.shape and v.tobytes() == got.astype(v.dtype).tobytes()


@pytest.mark.parametrize('precision', [64, 32])
def test_views_hold_what_get_returns(model, reference_traj, precision):
    import torch
    B = _batch(model, precision, reference_traj)
    _step(B)
    real = _real(precision)
    want = dict(OBS=np.float32, REWARD=np.float32, DISCOUNT=np.float32, STEP_TYPE=np.int32, QPOS=real, QVEL=real)
    for name, dtype in want.items():
        view, got = B.device_view(name), B.get(name)
        assert view.device == torch.device('cuda', 0) and view.cpu().numpy().dtype == dtype and tuple(view.shape) == (N, B._field(name)[2]), name
        _same_bits(view, got)
    assert (B.get('STEP_TYPE') == 1).all() and np.abs(B.get('QVEL')).max() > 0             # (a MID step that moved: not a comparison of zeros)
    row = B.row_bytes(0)//np.dtype(real).itemsize
    assert B.device_view('QPOS').stride() == (row, 1) and B.device_view('QVEL').stride() == (row, 1) and row > model.dim('nq')
    assert B.device_view('OBS').is_contiguous()


@pytest.mark.parametrize('precision', [64, 32])
def test_forces_written_through_the_view_are_read_back_and_consumed(model, reference_traj, precision):
    import torch
    B, plain = _batch(model, precision, reference_traj), _batch(model, precision, reference_traj)
    assert not B.forces_active
    qf, xf = B.device_view('QFRC_APPLIED'), B.device_view('XFRC_APPLIED')                   # (the first access allocates both, zeroed)
    assert B.forces_active and not qf.any() and not xf.any()
    nv, nbody, real = model.dim('nv'), model.dim('nbody'), _real(precision)
    assert tuple(qf.shape) == (N, nv) and tuple(xf.shape) == (N, 6*nbody) and qf.cpu().numpy().dtype == real and xf.cpu().numpy().dtype == real
    rng = np.random.default_rng(1)
    weight = np.asarray(model.arrays['body_mass'])*np.linalg.norm(model.arrays['opt_gravity'])
    q = rng.uniform(-1e-3, 1e-3, (N, nv)).astype(real)
    x = np.zeros((N, nbody, 6), real); x[:, 1:, 2] = rng.uniform(5, 10, (N, 1))*weight[1:]            # every body pulled up, harder than it weighs
    qf.copy_(torch.from_numpy(q)); xf.view(N, nbody, 6).copy_(torch.from_numpy(x)); torch.cuda.synchronize()
    assert np.array_equal(B.get('QFRC_APPLIED'), q.astype(np.float64)) and np.array_equal(B.get('XFRC_APPLIED'), x.reshape(N, -1).astype(np.float64))
    _step(B); _step(plain)
    assert B.forces_active and not plain.forces_active
    rise, rise_plain = B.get('QVEL')[:, 2], plain.get('QVEL')[:, 2]
    assert (rise > rise_plain).all(), (rise, rise_plain)                                    # (the step read them: the root moves up against the unforced twin)


@pytest.mark.parametrize('precision', [64, 32])
def test_env_model_view_of_a_group(reference_traj, precision):
    from flybody_amd import engine
    from flybody_amd.randomization import vary_model
    a = engine.Model.from_asset('walk_imitation').arrays
    G = engine.Batch(engine.ModelGroup([dict(a), vary_model(a, friction_scale=0.5)]), N, precision=precision)
    view = G.device_view('ENV_MODEL')
    assert tuple(view.shape) == (N, 1) and view.cpu().numpy().dtype == np.int32 and view.cpu().ravel().tolist() == [0, 1, 0]
    _same_bits(view, G.get('ENV_MODEL'))


@pytest.mark.parametrize('precision', [64, 32])
def test_control_law_views(model, reference_traj, precision):
    from flybody_amd import engine
    B = _batch(model, precision, reference_traj)
    nv, real = model.dim('nv'), _real(precision)
    vel_gain = np.random.default_rng(2).uniform(0.0, 1e-3, (N, nv))
    B.set_control_law(vel_gain=vel_gain)
    block = B.device_view('CONTROL_LAW')
    assert tuple(block.shape) == (N, 5*nv) and block.cpu().numpy().dtype == real
    law = block.view(N, len(engine.LAW_ROWS), nv).cpu().numpy()
    for r, row in enumerate(engine.LAW_ROWS):
        assert np.array_equal(law[:, r], vel_gain.astype(real) if row == 'vel_gain' else np.zeros((N, nv))), row
    _step(B)
    out = B.device_view('QFRC_LAW')
    assert tuple(out.shape) == (N, nv) and out.cpu().numpy().dtype == real and out.any()
    _same_bits(out, B.get('QFRC_LAW'))
