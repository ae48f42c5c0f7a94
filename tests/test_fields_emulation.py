"""engine.FIELDS against the library's own field table (csrc/fb_engine.hip: field_desc) through the kernel-source emulation build: fb_batch_get
checks the byte count it is given, so a get() that succeeds says the Python table's dtype and row width are the library's.  Every field,
both precisions, each once its documented precondition is met -- and the documented refusal before that.  No GPU needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_rollout_emulation import emu_lib  # noqa: E402,F401  (the emulation library's fixture)

N = 2
WRITABLE = ('QPOS', 'QVEL', 'ACT', 'CTRL', 'QACC', 'TIME', 'QFRC_APPLIED', 'XFRC_APPLIED')          # ... and ENV_MODEL, on the grouped batch
FP64_ONLY = {'IK_ERR': 'run fb_batch_ik first', 'IK_STEPS': 'run fb_batch_ik first', 'QFRC_INVERSE': 'run fb_batch_inverse first',
             'CONTACT_FORCE': 'run fb_batch_inverse first'}


def _refuses(call, text):
    from flybody_amd import engine
    with pytest.raises(engine.EngineError, match=text):
        call()


@pytest.mark.parametrize('precision', [64, 32])
def test_every_field_has_the_tables_dtype_and_width(emu_lib, walk_arrays, reference_traj, precision):  # noqa: F811
    from flybody_amd import engine
    from flybody_amd.randomization import vary_model
    model = engine.Model(walk_arrays, lib_path=emu_lib)
    nv = model.dim('nv')
    B = engine.Batch(model, N, precision=precision)
    qp, qv = reference_traj
    B.set_reference(qp[:8], qv[:8], future_steps=2, terminal_com_dist=float('inf')); B.reset()

    # preconditions, and the refusal each field documents before its own is met
    ik = lambda: B.ik([0], np.asarray(walk_arrays['leg_joints'])[:3], np.zeros((N, 1, 3)), max_steps=1)
    for name, text in FP64_ONLY.items():
        _refuses(lambda: B.get(name), text)
    if precision == 64:
        ik(); B.inverse()
    else:
        _refuses(ik, 'needs an FP64 batch'); _refuses(B.inverse, 'needs an FP64 batch')
        for name, text in FP64_ONLY.items():
            _refuses(lambda: B.get(name), text)
    _refuses(lambda: B.get('QFRC_APPLIED'), 'no applied forces'); _refuses(lambda: B.get('XFRC_APPLIED'), 'no applied forces')
    B.set('QFRC_APPLIED', 0.0); B.set('XFRC_APPLIED', 0.0)
    assert B.forces_active
    _refuses(lambda: B.get('QFRC_LAW'), 'no control law')
    vel_gain = np.random.default_rng(3).uniform(0.0, 1e-3, (N, nv))
    B.set_control_law(vel_gain=vel_gain)
    _refuses(lambda: B.get('ENV_MODEL'), 'needs a grouped batch')

    # the sweep: every field but CONTROL_LAW (and ENV_MODEL, which the grouped batch below serves)
    swept = []
    for name, (_, dtype, _) in engine.FIELDS.items():
        if name in ('CONTROL_LAW', 'ENV_MODEL') or (precision == 32 and name in FP64_ONLY):
            continue
        got = B.get(name)
        assert got.shape == (N, B._field(name)[2]) and got.dtype == dtype and got.shape[1] >= 1, name
        swept.append(name)
    assert len(swept) == len(engine.FIELDS) - 2 - (len(FP64_ONLY) if precision == 32 else 0)

    # CONTROL_LAW is not one row per environment: its (5, 'nv') rows through the pointer (the emulation build's "device" memory is the host's)
    _refuses(lambda: B.get('CONTROL_LAW'), 'not one row per environment')
    assert B.control_law_rows == N and B._field('CONTROL_LAW')[2] == len(engine.LAW_ROWS)*nv
    real = C.c_double if precision == 64 else C.c_float
    law = np.ctypeslib.as_array((real*(N*len(engine.LAW_ROWS)*nv)).from_address(B.device_ptr('CONTROL_LAW'))).reshape(N, len(engine.LAW_ROWS), nv)
    as_real = lambda x: np.asarray(x, real).astype(np.float64)                # a value as the batch's precision holds it
    for r, row in enumerate(engine.LAW_ROWS):
        assert np.array_equal(law[:, r], as_real(vel_gain) if row == 'vel_gain' else np.zeros((N, nv))), row

    # set then get, at the batch's precision (TIME is FP64 at either)
    rng = np.random.default_rng(4)
    for name in WRITABLE:
        v = rng.uniform(-1, 1, (N, B._field(name)[2]))
        B.set(name, v)
        assert np.array_equal(B.get(name), v if name == 'TIME' else as_real(v)), name

    # ENV_MODEL: a group of two models
    G = engine.Batch(engine.ModelGroup([dict(walk_arrays), vary_model(walk_arrays, friction_scale=0.5)], lib_path=emu_lib), N, precision=precision)
    em = G.get('ENV_MODEL')
    assert em.shape == (N, 1) and em.dtype == np.int32 and em.ravel().tolist() == [0, 1]
    G.set('ENV_MODEL', [[1], [0]])
    assert G.get('ENV_MODEL').ravel().tolist() == [1, 0]
