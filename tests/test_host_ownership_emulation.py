"""The engine's host layer owns its device memory and events through DevBuf / DevEvent (csrc/fb_host.hpp): whatever a batch allocated is
released when it is destroyed, a buffer that grows keeps the results, and an allocation that fails -- at any point of any entry point that
allocates -- leaves the batch as it was, usable, and leaks nothing.  Emulation build (csrc/emu/hip_emu.hpp counts the live blocks and
events and can make the k-th allocation fail); the stand-alone program tests/host_lifecycle_main.cpp runs the same life cycle under
AddressSanitizer, UBSan and LeakSanitizer."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

N_ENV = 3


@pytest.fixture(scope='module')
def emu_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    return g.build_emu()


@pytest.fixture(scope='module')
def lib(emu_lib, tmp_path_factory):
    """(path, handle) of a private copy of the emulation library: a library of its own in this process, so the live counts are this
    module's alone whatever batches other test modules keep or drop."""
    from flybody_amd import engine
    path = str(tmp_path_factory.mktemp('host_ownership') / 'libflybody_emu_host.so')
    shutil.copy(emu_lib, path)
    L = engine.load_library(path)
    L.fb_emu_fail_alloc.argtypes = [C.c_int]; L.fb_emu_fail_alloc.restype = None
    return path, L


@pytest.fixture(scope='module')
def model(lib, walk_arrays):
    from flybody_amd import engine
    return engine.Model(walk_arrays, lib_path=lib[0])


def _live(L):
    return L.fb_emu_live_allocs(), L.fb_emu_live_events()


def _destroy(B):
    B.L.fb_batch_destroy(B.h); B.h = None          # (Batch.__del__ then destroys a null handle: a no-op)


def _actions(steps, n=N_ENV, seed=3):
    return np.random.default_rng(seed).uniform(-1, 1, (steps, n, 59)).astype(np.float32)


def _step(B, a):
    a = np.ascontiguousarray(a, np.float32)
    B.step_ptr(a.ctypes.data)


def _fresh(model, reference_traj, n=N_ENV, precision=64):
    from flybody_amd import engine
    qp, qv = reference_traj
    B = engine.Batch(model, n, precision=precision)
    B.set_reference(qp[:8], qv[:8], future_steps=2, terminal_com_dist=float('inf')); B.reset()
    return B


def _ik_problem(arrays, B, n_site):
    """The first n_site leg-tip sites, the leg hinges, targets a little off where the sites are."""
    names = [str(s) for s in arrays['names_site']]
    sites = [names.index(s) for s in names if s.startswith(('tarsus_', 'claw_'))][:n_site]
    legs = [int(j) for j in arrays['leg_joints']]
    T = B.get('SITE_XPOS').reshape(B.n_env, -1, 3)[:, sites] + 0.01
    return sites, legs, np.ascontiguousarray(T)


def _ik(B, arrays, n_site):
    sites, legs, T = _ik_problem(arrays, B, n_site)
    B.ik(sites, legs, T, max_steps=3)


def _fd(B, n_frames):
    return B.transition_fd(env_ids=list(range(n_frames)), centered=False, n_substeps=1, want_A=False, want_B=True).B.numpy().copy()


# ------------------------------------------------------------------ life cycle
@pytest.mark.parametrize('kind', ['f64', 'f32', 'group'])
def test_lifecycle_releases_everything(lib, model, walk_arrays, reference_traj, kind):
    """Every entry point that allocates, twice where a second call grows or replaces a buffer; after fb_batch_destroy the live blocks and
    events are back at what they were with only the models loaded."""
    from flybody_amd import engine
    from flybody_amd.randomization import vary_model
    path, L = lib
    m = model
    if kind == 'group':
        m = engine.ModelGroup([dict(walk_arrays), vary_model(walk_arrays, friction_scale=0.5)], lib_path=path)
    base = _live(L)
    B = _fresh(m, reference_traj, precision=32 if kind == 'f32' else 64)
    acts = _actions(3)
    _step(B, acts[0])
    nv, nbody = model.dim('nv'), model.dim('nbody')
    B.set('XFRC_APPLIED', np.zeros((N_ENV, 6*nbody)))
    assert B.forces_active
    if kind != 'group':
        B.set_control_law(bias=np.zeros(nv)); assert B.control_law_rows == 1
        B.set_control_law(bias=np.full((N_ENV, nv), 1e-9)); assert B.control_law_rows == N_ENV
        _step(B, acts[1])
        B.clear_control_law(); assert not B.control_law_active and B.forces_active
    else:
        B.set('ENV_MODEL', np.array([[1], [0], [1]], np.int32))
        _step(B, acts[1])
    if kind == 'f64':
        _ik(B, walk_arrays, 1); _ik(B, walk_arrays, 3)
        B.inverse()
    B.clear_forces(); assert not B.forces_active
    if kind == 'f64':
        assert _fd(B, 1).shape[0] == 1 and _fd(B, 3).shape[0] == 3
        assert B.fd_tickets() > 0
    if kind != 'group':
        B.stage(engine.stage_sequence(model.dim('nsubstep'))[0][1], acts[2].ctypes.data)
    B.timing_begin(); _step(B, acts[2]); ms, n = B.timing_end()
    assert n == 1 and len(B.timing_launches()) == 1
    B.synchronize()
    live = _live(L)
    assert live[0] > base[0] + 20 and live[1] >= base[1] + 4           # (the counts see the batch at all: tables, arenas; two event pairs)
    _destroy(B)
    assert _live(L) == base


# ------------------------------------------------------------------ growth keeps results
def test_a_grown_derivative_buffer_keeps_results(lib, model, reference_traj):
    path, L = lib
    base = _live(L)
    B = _fresh(model, reference_traj)
    _step(B, _actions(1)[0])
    first, mid, third = _fd(B, 1), _fd(B, 3), _fd(B, 1)
    assert first.tobytes() == third.tobytes() and first.tobytes() == mid[:1].tobytes()
    assert np.abs(first).max() > 0
    _destroy(B)
    assert _live(L) == base


def test_a_grown_ik_buffer_keeps_results(lib, model, walk_arrays, reference_traj):
    path, L = lib
    base = _live(L)
    B = _fresh(model, reference_traj)
    q0 = B.get('QPOS')
    out = []
    for n_site in (1, 3, 1):
        B.set('QPOS', q0); B.forward()
        _ik(B, walk_arrays, n_site)
        out.append(B.get('QPOS'))
    assert out[0].tobytes() == out[2].tobytes()
    assert out[0].tobytes() != q0.tobytes() and out[0].tobytes() != out[1].tobytes()
    _destroy(B)
    assert _live(L) == base


# ------------------------------------------------------------------ allocation failures
@pytest.mark.parametrize('kind', ['single', 'group'])
def test_allocation_failure_sweep_at_creation(lib, model, walk_arrays, kind):
    """Every allocation of fb_batch_create fails in turn: an error with a message, and nothing is left behind."""
    from flybody_amd import engine
    from flybody_amd.randomization import vary_model
    path, L = lib
    m = model
    if kind == 'group':
        m = engine.ModelGroup([dict(walk_arrays), vary_model(walk_arrays, friction_scale=0.5)], lib_path=path)
    base = _live(L)
    failed, k = 0, 0
    for k in range(500):
        L.fb_emu_fail_alloc(k)
        try:
            B = engine.Batch(m, 2, precision=64)
        except engine.EngineError as e:
            L.fb_emu_fail_alloc(-1)
            assert str(e).strip(), k
            assert _live(L) == base, k
            failed += 1
            continue
        L.fb_emu_fail_alloc(-1)
        _destroy(B)
        break
    assert k < 499 and failed >= 20, (k, failed)
    assert _live(L) == base


def _op_law(B, arrays):
    nv = len(arrays['dof_bodyid'])
    B.set_control_law(bias=np.full(nv, 1e-6), vel_gain=np.full((N_ENV, nv), 1e-7))


def _op_forces(B, arrays):
    B.set('QFRC_APPLIED', np.full((N_ENV, len(arrays['dof_bodyid'])), 1e-6))


def _op_reference(B, arrays):
    from flybody_amd.reference import default_walking_reference
    qp, qv = default_walking_reference()
    B.set_reference(qp[:9], qv[:9], future_steps=3, terminal_com_dist=float('inf'))


def _op_ik(B, arrays):
    _ik(B, arrays, 2)


def _op_fd(B, arrays):
    _fd(B, 1)


# entry point -> (the call, the allocations it makes on a batch that has stepped: each of them must have been seen to fail)
LIVE_OPS = {'set_control_law': (_op_law, 5), 'set_qfrc_applied': (_op_forces, 2), 'set_reference': (_op_reference, 3), 'ik': (_op_ik, 3),
            'transition_fd': (_op_fd, 5)}


@pytest.mark.parametrize('name', list(LIVE_OPS))
def test_allocation_failure_sweep_on_a_live_batch(lib, model, walk_arrays, reference_traj, name):
    """Every allocation of the entry point fails in turn, each on a fresh batch that has been reset: the call fails with a message, the
    batch's law and force state reads as before, the same call then succeeds, and a reset and a step from there equal, to the bit, those of
    a twin batch that never saw a fault."""
    from flybody_amd import engine
    path, L = lib
    op, n_allocs = LIVE_OPS[name]
    act = _actions(1, seed=11)[0]
    base = _live(L)

    def outcome(B):
        B.reset(); _step(B, act)
        return [B.get(f).tobytes() for f in ('QPOS', 'QVEL', 'OBS')]

    twin = _fresh(model, reference_traj)
    op(twin, walk_arrays)
    want = outcome(twin)
    _destroy(twin)
    failed = 0
    for k in range(50):
        B = _fresh(model, reference_traj)
        before = (B.control_law_active, B.forces_active)
        L.fb_emu_fail_alloc(k)
        try:
            op(B, walk_arrays)
            ok = True
        except engine.EngineError as e:
            ok = False
            assert str(e).strip(), k
        L.fb_emu_fail_alloc(-1)
        if not ok:
            failed += 1
            assert (B.control_law_active, B.forces_active) == before, k
            if name == 'set_reference':
                with pytest.raises(engine.EngineError, match='fb_batch_step: call fb_batch_set_reference first'):
                    _step(B, act)
            op(B, walk_arrays)                        # the same call, no fault: succeeds
            assert outcome(B) == want, k
        _destroy(B)
        assert _live(L) == base, k
        if ok:
            break
    assert ok and failed >= n_allocs, (k, failed)


# ------------------------------------------------------------------ the host layer under the sanitizers
def test_host_lifecycle_program_is_clean_under_the_sanitizers(walk_arrays, tmp_path):
    """tests/host_lifecycle_main.cpp includes fb_engine.hip (emulation, launches compiled out) and runs the life cycle above and one failed
    allocation per entry point through the C-ABI; built with AddressSanitizer and UBSan, it exits 0 and neither they nor LeakSanitizer
    report anything."""
    from flybody_amd.model_blob import pack_model
    exe, blob = str(tmp_path / 'host_lifecycle'), str(tmp_path / 'walk.fbm')
    open(blob, 'wb').write(pack_model(walk_arrays))
    subprocess.check_call(['g++', '-O0', '-std=c++17', '-x', 'c++', '-DFB_EMULATE', '-DFB_EMU_NO_LAUNCH', '-DFB_BUILD_ID="host_lifecycle"',
                           '-fsanitize=address,undefined', '-fno-omit-frame-pointer', '-static-libasan', '-static-libubsan', '-I' + os.path.join(ROOT, 'flybody_amd', 'csrc'),
                           '-o', exe, os.path.join(ROOT, 'tests', 'host_lifecycle_main.cpp')], cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([exe, blob], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'host lifecycle ok' in r.stdout
    for word in ('ERROR: AddressSanitizer', 'ERROR: LeakSanitizer', 'runtime error:'):
        assert word not in r.stderr, r.stderr[-4000:]
