"""Per-environment physics models in one batch (fb_batch_create_group, the kernels k_group_step / k_group_reset) through the
kernel-source emulation build:
  * every environment of a grouped batch equals, to the bit, the same environment index of a plain batch of its variant, under both
    schedulers and through an auto-reset;
  * the grouped batch against one CPU oracle per variant (the oracle loads any blob of its model class);
  * what the host validates: compatibility of the models, the assignment, the entry points that refuse a group;
  * flybody_amd.randomization.vary_model and the compiler refactor behind it.
No GPU needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

_rel = lambda a, b: np.abs(np.asarray(a).ravel() - np.asarray(b).ravel()).max() / max(np.abs(np.asarray(b)).max(), 1e-300)

# the bounds tests/test_kernel_emulation.py holds for control steps against the oracle (test_env_steps_match_oracle_and_golden)
TOL_QPOS, TOL_QVEL = 1e-9, 1e-8
FIELDS = ('QPOS', 'QVEL', 'OBS', 'REWARD', 'STEP_TYPE')


@pytest.fixture(scope='module')
def emu_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    return g.build_emu()


@pytest.fixture(scope='module')
def variants(walk_arrays):
    """Two variants of walk_imitation: the nominal model, and one with other friction, gains, damping, gravity and per-body masses."""
    from flybody_amd.randomization import vary_model
    nb = len(walk_arrays['body_mass'])
    f = np.random.default_rng(7).uniform(0.8, 1.2, nb); f[0] = 1
    g = np.asarray(walk_arrays['opt_gravity'], float)
    other = vary_model(walk_arrays, friction_scale=0.5, gain_scale=0.8, damping_scale=1.5, mass_scale=f,
                       gravity=g + 0.1*np.linalg.norm(g)*np.array([np.cos(0.7), np.sin(0.7), 0.0]))
    return [dict(walk_arrays), other]


def _short(B, reference_traj):
    """The short reference of tests/test_forces_emulation.py: an episode ends (LAST) and auto-resets (FIRST) within six steps."""
    qp, qv = reference_traj
    B.set_reference(qp[:8], qv[:8], future_steps=2, terminal_com_dist=float('inf')); B.reset()


def test_grouped_batch_equals_plain_batches_of_its_variants(emu_lib, variants, reference_traj, monkeypatch):
    """5 environments, 2 variants, 6 control steps with an auto-reset inside, substep scheduler (the emulation build's two slots put five
    environments on tickets) and one environment per wave: environment e of the group == environment e of a plain batch of variant e % 2."""
    from flybody_amd import engine
    acts = np.random.default_rng(9).uniform(-1, 1, (6, 5, 59)).astype(np.float32)
    for flag in (None, '1'):
        if flag is None: monkeypatch.delenv('FB_NO_TICKETS', raising=False)
        else: monkeypatch.setenv('FB_NO_TICKETS', flag)
        group = engine.ModelGroup(variants, lib_path=emu_lib)
        G = engine.Batch(group, 5, precision=64)
        P = [engine.Batch(m, 5, precision=64) for m in group.models]
        assert G.n_models == 2 and P[0].n_models == 1 and G.substep_scheduler == (flag is None)
        em = G.get('ENV_MODEL').ravel()
        assert em.tolist() == [0, 1, 0, 1, 0]
        for B in [G] + P:
            _short(B, reference_traj)
        types = []
        for k in range(6):
            a = np.ascontiguousarray(acts[k])
            for B in [G] + P:
                B.step_ptr(a.ctypes.data)
            for name in FIELDS:
                g = G.get(name)
                for e in range(5):
                    assert np.array_equal(g[e], P[em[e]].get(name)[e]), (flag, k, name, e)
            types.append(G.get('STEP_TYPE').ravel())
            if k == 0:                                                        # the check can fail: the two variants do not step alike
                assert _rel(P[0].get('QVEL')[0], P[1].get('QVEL')[0]) > 1e-3
        types = np.array(types)
        assert (types == 2).any() and (types == 0).any()
        assert not G.get('WARN_EVER').any()
        del G, P, group


def test_grouped_batch_matches_one_oracle_per_variant(emu_lib, variants, reference_traj):
    """The same batch against the CPU oracle: one OracleModel per variant, one OracleData per environment, through the auto-reset."""
    from flybody_amd import engine
    from flybody_amd.model_blob import pack_model
    from oracle import fbo
    qp, qv = reference_traj
    acts = np.random.default_rng(9).uniform(-1, 1, (6, 5, 59)).astype(np.float32)
    group = engine.ModelGroup(variants, lib_path=emu_lib)
    G = engine.Batch(group, 5, precision=64)
    _short(G, reference_traj)
    oms = [fbo.OracleModel(pack_model(v)) for v in variants]
    ods = []
    for e in range(5):
        od = fbo.OracleData(oms[e % 2]); od.configure_env(qp[:8], qv[:8], future_steps=2, terminal_com_dist=float('inf')); od.env_reset(); ods.append(od)
    worst = [0.0, 0.0]
    for k in range(6):
        a = np.ascontiguousarray(acts[k])
        G.step_ptr(a.ctypes.data)
        for e in range(5):
            ods[e].env_step(acts[k, e].astype(np.float64))
        Q, V = G.get('QPOS'), G.get('QVEL')
        assert G.get('STEP_TYPE').ravel().tolist() == [int(od.scalar('step_type')) for od in ods]
        for e in range(5):
            worst = [max(worst[0], _rel(Q[e], ods[e].field('qpos'))), max(worst[1], _rel(V[e], ods[e].field('qvel')))]
        assert all(int(od.scalar('ncon')) < 64 and int(od.scalar('nefc')) < 192 for od in ods)
        if k == 0:          # the check can fail: environment 1 (variant 1) against the oracle of environment 0 (variant 0, same actions apart) is far outside
            assert _rel(V[1], ods[0].field('qvel')) > 1e-3
    print('grouped batch vs one oracle per variant, 6 control steps: qpos %.2e qvel %.2e' % tuple(worst))
    assert worst[0] < TOL_QPOS and worst[1] < TOL_QVEL, worst
    assert not G.get('WARN_EVER').any()


def test_host_validation(emu_lib, variants, reference_traj):
    from flybody_amd import engine
    nominal, other = variants
    # an incompatible model is rejected with the array named: one integer entry changed, another time step
    bad = dict(other); bad['jnt_limited'] = np.array(other['jnt_limited']); bad['jnt_limited'][10] ^= 1
    with pytest.raises(engine.EngineError, match="model 1 is not compatible with model 0: array 'jnt_limited' differs"):
        engine.ModelGroup([nominal, bad], lib_path=emu_lib)
    bad = dict(other); bad['opt_timestep'] = np.array(float(other['opt_timestep'])*0.5)
    with pytest.raises(engine.EngineError, match="array 'opt_timestep' differs"):
        engine.ModelGroup([nominal, bad], lib_path=emu_lib)
    bad = dict(other); bad['opt_iterations'] = np.array(50)
    with pytest.raises(engine.EngineError, match="array 'opt_iterations' differs"):
        engine.ModelGroup([nominal, nominal, bad], lib_path=emu_lib)
    group = engine.ModelGroup(variants, lib_path=emu_lib)
    L = group.L
    h = C.c_void_p()
    assert L.fb_batch_create_group(group.handles, 0, 2, 0, 64, C.byref(h)) != 0
    assert L.fb_batch_create_group(group.handles, 257, 2, 0, 64, C.byref(h)) != 0 and b'FB_MAX_MODELS' in L.fb_last_error()
    assert L.fb_batch_create_group(None, 2, 2, 0, 64, C.byref(h)) != 0
    G = engine.Batch(group, 3, precision=64)
    # the assignment: set() validates, the row / pointer path is clamped by the kernel and flagged
    G.set('ENV_MODEL', np.array([[1], [1], [0]]))
    assert G.get('ENV_MODEL').ravel().tolist() == [1, 1, 0]
    for v in (2, -1):
        with pytest.raises(engine.EngineError, match=r'FB_ENV_MODEL of environment 1 is %d, outside \[0, 2\)' % v):
            G.set('ENV_MODEL', np.array([[0], [v], [0]]))
    assert G.get('ENV_MODEL').ravel().tolist() == [1, 1, 0]                   # a rejected set changes nothing
    with pytest.raises(engine.EngineError, match='size mismatch'):
        engine._check(L, L.fb_batch_set(G.h, engine.FIELDS['ENV_MODEL'][0], np.zeros(2, np.int32).ctypes.data, 8))
    _short(G, reference_traj)
    P = engine.Batch(group.models[1], 3, precision=64); _short(P, reference_traj)
    ptr = (C.c_int32*3).from_address(G.device_ptr('ENV_MODEL'))               # (the emulation build's "device" memory is host memory)
    ptr[0] = 7; ptr[2] = -3
    G.reset(); P.reset()
    a = np.random.default_rng(1).uniform(-1, 1, (3, 59)).astype(np.float32)
    G.step_ptr(a.ctypes.data); P.step_ptr(a.ctypes.data)
    warn, ever = G.get('WARN').ravel(), G.get('WARN_EVER').ravel()
    bit = engine.WARN_BITS['MODEL_ID']
    assert bit == 64 and (warn & bit).tolist() == [bit, 0, bit] and (ever & bit).tolist() == [bit, 0, bit]
    # clamped: 7 -> model 1, -3 -> model 0
    assert np.array_equal(G.get('QPOS')[:2], P.get('QPOS')[:2]) and not np.array_equal(G.get('QPOS')[2], P.get('QPOS')[2])
    ptr[0] = 1; ptr[2] = 0
    G.step_ptr(a.ctypes.data)
    assert not (G.get('WARN').ravel() & bit).any() and (G.get('WARN_EVER').ravel() & bit).tolist() == [bit, 0, bit]
    # entry points that never silently use model 0
    with pytest.raises(engine.EngineError, match='fb_batch_ik: per-model inverse kinematics is not supported'):
        G.ik([0], [1], np.zeros((3, 1, 3)))
    with pytest.raises(engine.EngineError, match='fb_batch_inverse: per-model inverse dynamics is not supported'):
        G.inverse()
    with pytest.raises(engine.EngineError, match='fb_batch_stage: .*group of 2 models'):
        G.stage(engine.ST['PRE'], a.ctypes.data)
    # a plain batch has no assignment
    with pytest.raises(engine.EngineError, match='FB_ENV_MODEL needs a grouped batch'):
        P.get('ENV_MODEL')
    with pytest.raises(engine.EngineError, match='FB_ENV_MODEL needs a grouped batch'):
        P.set('ENV_MODEL', 0)
    with pytest.raises(engine.EngineError, match='no device pointer'):
        P.device_ptr('ENV_MODEL')
    # a group of one model steps like fb_batch_create
    one = engine.Batch(engine.ModelGroup([other], lib_path=emu_lib), 3, precision=64); _short(one, reference_traj)
    assert one.n_models == 1 and not one.get('ENV_MODEL').any()
    P.reset(); one.step_ptr(a.ctypes.data); P.step_ptr(a.ctypes.data)
    for name in FIELDS:
        assert np.array_equal(one.get(name), P.get(name)), name
    one.inverse()                                                            # (nothing to refuse)


def test_group_with_forces_and_fp32(emu_lib, variants, reference_traj):
    """k_group_step with the applied-force stage, and an FP32 group: bit-equal to plain batches of the variants."""
    from flybody_amd import engine
    rng = np.random.default_rng(4)
    nb = len(variants[0]['body_mass'])
    xf = rng.normal(size=(4, 6*nb))*1e-3
    a = rng.uniform(-1, 1, (2, 4, 59)).astype(np.float32)
    for precision, forces in ((64, True), (32, False), (32, True)):
        group = engine.ModelGroup(variants, lib_path=emu_lib)
        G = engine.Batch(group, 4, precision=precision)
        P = [engine.Batch(m, 4, precision=precision) for m in group.models]
        for B in [G] + P:
            _short(B, reference_traj)
            if forces:
                B.set('XFRC_APPLIED', xf)
        for k in range(2):
            for B in [G] + P:
                B.step_ptr(np.ascontiguousarray(a[k]).ctypes.data)
        for name in FIELDS:
            g = G.get(name)
            for e in range(4):
                assert np.array_equal(g[e], P[e % 2].get(name)[e]), (precision, forces, name, e)
        assert np.isfinite(G.get('QPOS')).all()


def test_vary_model_and_compiler_refactor(walk_arrays):
    from flybody_amd import randomization as R
    from flybody_amd.mjcf_compile import set_const0
    a = walk_arrays
    same = R.vary_model(a)
    assert set(same) == set(a)
    for k in a:
        assert np.array_equal(same[k], a[k]) and same[k].dtype == np.asarray(a[k]).dtype, k
    # recomputing the derived constants of the shipped asset reproduces them bit for bit (mjcf_compile.set_const0 is the compiler's code)
    m = R.recompute_constants({k: np.array(v) for k, v in a.items()})
    for k in R.DERIVED:
        assert np.array_equal(m[k], a[k]), k
    assert callable(set_const0)
    # mass x 2 (inertia with it): M0 -> 2 M0 - armature, so an inverse weight halves except for the armature's share.  walk_imitation HAS
    # armature-dominated dofs (armature 1e-6 is up to 0.999997 of dof_M0), so on the shipped model the ratio new / old deviates from 1/2 by
    # up to 0.440 (body), 0.499997 (dof) and 0.49976 (tendon): measured.  The same model with the armature removed has none: measured
    # deviation 0.0 for all three (a factor 2 is exact in binary floating point) -- asserted there, at 1e-12.
    bare = dict(a); bare['dof_armature'] = np.zeros_like(a['dof_armature'])
    bare = R.recompute_constants({k: np.array(v) for k, v in bare.items()})
    two = R.vary_model(bare, mass_scale=2.0)
    dev = {}
    for k in ('body_invweight0', 'dof_invweight0', 'tendon_invweight0'):
        nz = np.abs(bare[k]) > 0
        dev[k] = float(np.abs(two[k][nz]/bare[k][nz] - 0.5).max())
    print('mass x 2, deviation of invweight ratio from 1/2 (no armature):', dev)
    assert max(dev.values()) < 1e-12, dev
    assert np.allclose(two['body_subtreemass'], 2*bare['body_subtreemass'], rtol=1e-14) and np.allclose(two['dof_M0'], 2*bare['dof_M0'], rtol=1e-13)
    assert np.isclose(float(two['stat_meaninertia']), 2*float(bare['stat_meaninertia']), rtol=1e-13)
    with_arm = R.vary_model(a, mass_scale=2.0)
    r = with_arm['dof_invweight0']/a['dof_invweight0']
    assert (r > 0.5 - 1e-12).all() and (r <= 1.0).all()                        # armature does not scale: weights fall by less than half
    # per-body factors, the world body's ignored; gains and biases move together; halteres keep their compiled spring-damper
    f = np.random.default_rng(7).uniform(0.8, 1.2, len(a['body_mass'])); f0 = f.copy(); f[0] = 5.0
    v = R.vary_model(a, mass_scale=f, gain_scale=0.8, damping_scale=1.5, stiffness_scale=1.1, friction_scale=2.0, density=1.2e-3, viscosity=2e-4)
    f0[0] = 1
    assert np.array_equal(v['body_mass'], a['body_mass']*f0) and np.array_equal(v['body_inertia'], a['body_inertia']*f0[:, None])
    assert np.array_equal(v['actuator_gainprm'], a['actuator_gainprm']*0.8) and np.array_equal(v['actuator_biasprm'], a['actuator_biasprm']*0.8)
    assert np.array_equal(v['dof_damping'], a['dof_damping']*1.5) and np.array_equal(v['jnt_stiffness'], a['jnt_stiffness']*1.1)
    assert np.array_equal(v['pair_friction'][:, :2], a['pair_friction'][:, :2]*2.0) and np.array_equal(v['pair_friction'][:, 2:], a['pair_friction'][:, 2:])
    assert float(v['opt_density']) == 1.2e-3 and float(v['opt_viscosity']) == 2e-4
    for k in a:                                                               # integer arrays, shapes and the time steps stay
        assert v[k].shape == np.asarray(a[k]).shape and v[k].dtype == np.asarray(a[k]).dtype, k
        if np.asarray(a[k]).dtype.kind in 'iuUS' or k in ('opt_timestep', 'opt_control_timestep'):
            assert np.array_equal(v[k], a[k]), k
    with pytest.raises(ValueError):
        R.vary_model(a, mass_scale=np.ones(3))
    with pytest.raises(ValueError):
        R.vary_model(a, damping_scale=-1.0)
    s1, s2 = (R.sample_models(a, 3, dict(friction_scale=(0.8, 1.2), gain_scale=(0.8, 1.2)), seed=5) for _ in range(2))
    assert len(s1) == 3 and all(np.array_equal(x['pair_friction'], y['pair_friction']) for x, y in zip(s1, s2))
    assert not np.array_equal(s1[0]['pair_friction'], s1[1]['pair_friction'])
    with pytest.raises(ValueError):
        R.sample_models(a, 1, dict(gravity=(0, 1)))


def test_compiler_output_is_unchanged():
    """The refactor (Compiler._set0 -> mjcf_compile.set_const0, a function of the array dict) leaves the compiler's output as it was: the
    function the compiler now calls, run on each shipped asset, reproduces the asset's reference-configuration constants bit for bit.
    (tests/test_model_variants.py compiles the committed models from the MJCF where the reference XML is present; with this refactor
    the three assets came out byte-identical.)"""
    from flybody_amd import engine
    from flybody_amd.mjcf_compile import set_const0
    for name in ('walk_imitation', 'flight_imitation', 'walk_on_ball'):
        a = dict(engine.load_npz(os.path.join(engine.ASSETS, name + '.npz')))
        m = {k: np.array(v) for k, v in a.items()}
        set_const0(m)
        for k in ('dof_M0', 'M0_full', 'body_invweight0', 'dof_invweight0', 'tendon_invweight0'):
            assert np.array_equal(m[k], a[k]), (name, k)


def test_symbols_and_fields(emu_lib):
    import re
    import subprocess
    import __graft_entry__ as g
    from flybody_amd import engine
    lib = g.build_hip()
    syms = subprocess.check_output(['nm', '-D', '--defined-only', lib], text=True)
    assert ' fb_batch_create_group' in syms and ' fb_batch_n_models' in syms
    assert engine.FIELDS['ENV_MODEL'][0] == 42
    names = [re.search(r'Function Name: (\S+)', l).group(1) for l in open(g.HIP_RES) if 'Function Name' in l]
    assert sum('k_group_step' in n for n in names) == 4 and sum('k_group_reset' in n for n in names) == 2
    assert not any('k_fly' in n and 'group' in n for n in names) and sum('k_flyI' in n for n in names) == 2
