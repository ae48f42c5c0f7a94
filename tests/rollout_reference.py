"""The recipe of fb_batch_rollout in ctrl mode, once, on the CPU oracle: the position and velocity stages of the start state (step1),
then per control interval the interval's ctrl and n substeps, the state and the sensors recorded behind every interval -- the loop of
fd_reference.Frame.transition with a record per interval.  Test helper, not a test."""
import numpy as np

NSENS = 33


def oracle_rollout(om, a, qpos, qvel, act, ctrl, n_substeps, w=None):
    """(state [T, nq + nv + na], sensordata [T, 33], nefc of every solve) of the rollout of ctrl [T, nu] from (qpos, qvel, act); w: the
    warm start of the first constraint solve (None: the acceleration of a forward evaluation at the start state under ctrl0 = 0, which
    is what a helper batch's forward() leaves when its CTRL was never set)."""
    from oracle import fbo
    od = fbo.OracleData(om)
    na = int((np.asarray(a['actuator_actadr']) >= 0).sum())
    ctrl = np.asarray(ctrl, float)

    def put(ws, u):
        od.field('qpos')[:] = qpos; od.field('qvel')[:] = qvel; od.field('ctrl')[:] = u; od.field('qacc_warmstart')[:] = ws
        if na:
            od.field('act')[:] = act
    if w is None:
        put(np.zeros(len(qvel)), np.zeros(ctrl.shape[1]))
        od.call('forward')
        w = od.field('qacc').copy()
    put(w, ctrl[0])
    od.call('step1')
    states, sens, nefc = [], [], []
    for u in ctrl:
        od.field('ctrl')[:] = u
        for _ in range(n_substeps):
            nefc.append(int(od.scalar('nefc')))
            od.call('step')
        act_n = od.field('act')[:na].copy() if na else np.zeros(0)
        states.append(np.r_[od.field('qpos'), od.field('qvel'), act_n])
        sens.append(od.field('sensordata')[:NSENS].copy())
    return np.array(states), np.array(sens), nefc


def rel_err(got, ref):
    """max |got - ref| over max |ref| of one vector: the measure of tests/test_gpu_parity.py's contract (its _rel)."""
    got, ref = np.asarray(got, float).ravel(), np.asarray(ref, float).ravel()
    return float(np.abs(got - ref).max()/max(np.abs(ref).max(), 1e-300))
