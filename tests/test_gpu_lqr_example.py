"""The README's closed-loop example (tests/test_gpu_feedback_example.py) with the gains computed on the device (DESIGN.md
23): nominal rollout -> derivatives.transition_fd along it -> A, B uploaded once -> Batch.lqr_backward -> closed-loop rollouts under the
tensor it returns.  These are physical matrices, less well conditioned than the synthetic ones of tests/lqr_cases.py (Q is singular, R is
1e-3 / range^2), so K is held to the project's standing 1e-6 relative against lqr.tvlqr (tests/test_gpu_parity.py's contract and measure).

Measured on the MI355X: K against lqr.tvlqr 2.5e-15, P 3.3e-16; closed / open cost ratio of the eight starts 0.78 .. 0.88, in the linear
model and in the simulation alike."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_feedback_example import N_START, T, cost, weights  # noqa: E402
from test_gpu_parity import _rel  # noqa: E402

pytestmark = pytest.mark.gpu


def test_device_gains_close_the_loop():
    import torch
    from conftest import random_state
    from flybody_amd import derivatives, engine, lqr, rollout
    from test_deriv_emulation import mid_ctrl
    model = engine.Model.from_asset('walk_imitation')
    shim = types.SimpleNamespace(arrays=model.arrays); a = model.arrays
    nq, nv, na, nu = (model.dim(k) for k in ('nq', 'nv', 'na', 'nu'))
    rng = np.random.default_rng(0)
    q0, v0 = random_state(a, np.random.default_rng(0), spread=0.0, z=2.0)
    act0 = np.zeros(na)
    u_bar = np.tile(mid_ctrl(a, rng, 0.45, 0.55), (T, 1))
    nom = rollout.rollout(model, q0, v0, act0, u_bar)
    x_nom, u_nom = lqr.nominal_from_rollout(np.r_[q0, v0, act0], nom.state, u_bar)
    fd = derivatives.transition_fd(model, x_nom[:, :nq], x_nom[:, nq:nq + nv], x_nom[:, nq + nv:], u_nom, n_substeps=model.dim('nsubstep'))
    assert not np.asarray(fd.status).any()
    width = np.asarray(a['actuator_ctrlrange'], float) @ [-1.0, 1.0]
    Q, R = weights(nv, na, nu, width)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float64)).cuda()
    batch = engine.Batch(model, 1, precision=64)
    res = batch.lqr_backward(up(np.asarray(fd.A)[None]), up(np.asarray(fd.B)[None]), up(Q), up(R), want_P=True)
    K_host, P_host = lqr.tvlqr(fd.A, fd.B, Q, R)
    K = res.K[0].cpu().numpy()
    eK, eP = _rel(K, K_host), _rel(res.P[0].cpu().numpy(), P_host)
    print(f'device gains against lqr.tvlqr: K {eK:.1e}  P {eP:.1e}')
    assert res.status.tolist() == [0] and eK < 1e-6 and eP < 1e-6
    d0 = np.zeros((N_START, 2*nv + na))
    d0[:, 6:nv] = 0.02*rng.normal(size=(N_START, nv - 6)); d0[:, nv + 6:2*nv] = 0.5*rng.normal(size=(N_START, nv - 6))
    lin = []
    for gains in (np.zeros_like(K), K):
        dx = [d0]; du = []
        for t in range(T):
            du.append(dx[-1] @ gains[t].T)
            dx.append(dx[-1] @ fd.A[t].T + du[-1] @ fd.B[t].T)
        lin.append(cost(np.stack(dx, 1), np.stack(du, 1), Q, R))
    qs = derivatives.integrate_pos(shim, np.tile(q0, (N_START, 1)), d0[:, :nv])
    vs, acts = v0 + d0[:, nv:2*nv], act0 + d0[:, 2*nv:]
    # the simulation: the source environments hold the starts, and the gains go from lqr_backward to rollout_feedback as they are
    sim_batch = engine.Batch(model, N_START, precision=64)
    sim_batch.set('QPOS', qs); sim_batch.set('QVEL', vs); sim_batch.set('CTRL', np.tile(u_bar[0], (N_START, 1)))
    if na:
        sim_batch.set('ACT', acts)
    sim_batch.forward(torch.cuda.current_stream().cuda_stream)
    u_open = np.tile(u_bar, (N_START, 1, 1))
    open_ = sim_batch.rollout(ctrl=up(u_open))
    closed = sim_batch.rollout_feedback(up(x_nom[None]), up(u_nom[None]), res.K, nom_ids=np.zeros(N_START, np.int32), env_ids=np.arange(N_START, dtype=np.int32))
    torch.cuda.synchronize()
    x_end = np.concatenate([x_nom, nom.state[-1:]])
    sim = []
    for r, u in ((open_, u_open), (closed, closed.ctrl.cpu().numpy())):
        x = np.concatenate([np.c_[qs, vs, acts][:, None], r.state.cpu().numpy()], axis=1)
        sim.append(cost(lqr.state_difference(shim, x, np.broadcast_to(x_end, x.shape)), u - u_nom, Q, R))
    print('closed / open: linear model', np.round(lin[1]/lin[0], 2), ' simulated', np.round(sim[1]/sim[0], 2))
    assert (lin[1] <= 0.9*lin[0]).all(), lin[1]/lin[0]
    assert not open_.status.cpu().numpy().any() and not closed.status.cpu().numpy().any()
    assert (sim[1] < sim[0]).all(), sim[1]/sim[0]


def test_lqr_gains_of_live_environments():
    """env.lqr_gains(env.linearize(...)): stationary-mode gains of two live environments, shaped for env.rollout(feedback=...), with the
    status the numpy recursion gives on the same A, B."""
    import torch
    from flybody_amd import fly_envs, lqr
    env = fly_envs.BatchedFlyEnv(4, terminal_com_dist=float('inf'))
    env.reset_all()
    m = env.model
    nv, na, nu = (m.dim(k) for k in ('nv', 'na', 'nu'))
    width = np.asarray(m.arrays['actuator_ctrlrange'], float) @ [-1.0, 1.0]
    Q, R = weights(nv, na, nu, width)
    lin = env.linearize([0, 1], n_substeps=10)
    res = env.lqr_gains(lin, Q, R, horizon=20)
    torch.cuda.synchronize()
    A, B = lin.A.cpu().numpy(), lin.B.cpu().numpy()
    ref = lqr.backward_pass(np.repeat(A[:, None], 20, 1), np.repeat(B[:, None], 20, 1), Q, R)
    assert res.K.shape == (2, 1, nu, 2*nv + na) and res.P.shape == (2, 2, 2*nv + na, 2*nv + na)
    assert res.status.tolist() == ref[5].tolist()
    assert torch.isfinite(res.K).all() and torch.isfinite(res.P).all()
    if not ref[5].any():
        assert res.status.tolist() == [0, 0]
        assert _rel(res.K[:, 0].cpu().numpy(), ref[0][:, 0]) < 1e-6
        assert res.K.transpose(2, 3).is_contiguous()
