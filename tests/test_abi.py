"""The C-ABI library: loads, exports every symbol include/flybody_engine.h declares, validates its
arguments, and fails loudly (no CPU fallback) when there is no GPU."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def _declared_symbols():
    hdr = open(os.path.join(ROOT, 'include', 'flybody_engine.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    return sorted(set(re.findall(r'\b(fb_[a-z_0-9]+)\s*\(', hdr)))


@pytest.mark.parametrize('which', ['default', 'dense'])
def test_library_exports_header_symbols(which):
    """Both builds of the engine (default; FB_F64_DENSE = 12 FP64 environments per CU, engine.HIP_LIB_DENSE) export the whole header."""
    import __graft_entry__ as g
    lib = C.CDLL(g.build_hip() if which == 'default' else g.build_hip_dense())
    syms = _declared_symbols()
    assert len(syms) >= 17 and "fb_batch_step" in syms
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in flybody_engine.h but not exported'


def test_learner_library_exports_header_symbols():
    """libflybody_learner.so exports every entry point include/flybody_learner.h declares (no compute calls without a GPU)."""
    import __graft_entry__ as g
    hdr = open(os.path.join(ROOT, 'include', 'flybody_learner.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    syms = sorted(set(re.findall(r'\b(fbl_[a-z_0-9]+)\s*\(', hdr)))
    lib = C.CDLL(g.build_learner())
    assert len(syms) >= 20 and 'fbl_sgemm_op' in syms and 'fbl_mpo_loss' in syms
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in flybody_learner.h but not exported'
    lib.fbl_version.restype = C.c_char_p
    from flybody_amd.dmpo import fused
    assert fused.source_hash().encode() in lib.fbl_version()          # the binary names the sources it was built from


def test_learner_gather_refuses_a_segment_end_inside_a_tensor():
    """fbl_gather_flat attributes a chunk that lies inside one tensor to the Adam segment of the chunk's first element, which is right only
    when every segment ends where a tensor ends: any other layout is an error, decided on the host before anything is launched (so no GPU is
    needed, and the pointers below are never read)."""
    from flybody_amd.dmpo import fused
    L = fused.lib()
    ends = (C.c_int64*3)(1000, 3000, 3005); src = (C.c_void_p*3)(64, 64, None)
    fake = C.c_void_p(64)
    call = lambda seg: L.fbl_gather_flat(src, ends, 3, fake, len(seg), (C.c_int64*len(seg))(*seg), fake, fake, None)
    for seg in ([2999, 3005], [1000, 3001, 3005], [1, 3005]):
        assert call(seg) != 0 and b'segment end' in L.fbl_last_error(), seg
    assert call([1000, 3004]) != 0 and b'bad segments' in L.fbl_last_error()          # (the last end must be the total, as before)


def test_model_load_and_argument_validation(walk_arrays):
    from flybody_amd import engine
    M = engine.Model(walk_arrays)
    assert M.dim('nq') == 109 and M.dim('nv') == 108 and M.dim('nu') == 59 and M.dim('nsubstep') == 10
    assert M.dim('no_such_dim') == -1
    h = C.c_void_p()
    assert M.L.fb_model_load(b'XXXX0000', 8, C.byref(h)) != 0
    assert b'magic' in M.L.fb_last_error()
    assert M.L.fb_batch_create(M.h, 0, 0, 64, C.byref(h)) != 0
    assert M.L.fb_batch_create(M.h, 4, 0, 16, C.byref(h)) != 0
    assert b'precision' in M.L.fb_last_error()


def test_malformed_blobs_are_errors_not_aborts(walk_arrays):
    """fb_model_load validates every array it will read (a missing array used to abort() the process)."""
    import numpy as np
    from flybody_amd import engine
    from flybody_amd.model_blob import pack_model
    L = engine.load_library()
    assert 'flybody_engine' in engine.version() and engine.source_hash() in engine.version()      # the binary names the sources it was built from
    h = C.c_void_p()

    def load(arrays):
        blob = pack_model(arrays)
        rc = L.fb_model_load(blob, len(blob), C.byref(h))
        if rc == 0:
            L.fb_model_destroy(h)
        return rc, L.fb_last_error().decode()

    assert load(dict(walk_arrays))[0] == 0
    a = dict(walk_arrays); del a['jnt_solimp']
    rc, msg = load(a); assert rc != 0 and 'jnt_solimp' in msg
    a = dict(walk_arrays); a['body_mass'] = np.asarray(a['body_mass'])[:10]
    rc, msg = load(a); assert rc != 0 and 'body_mass' in msg
    a = dict(walk_arrays); a['geom_type'] = np.asarray(a['geom_type'], np.float64)
    rc, msg = load(a); assert rc != 0 and 'geom_type' in msg
    a = dict(walk_arrays); g = np.asarray(a['pair_geom2']).copy(); g[5] = 10_000; a['pair_geom2'] = g
    rc, msg = load(a); assert rc != 0 and 'pair_geom2' in msg
    a = dict(walk_arrays); a['opt_timestep'] = np.float64(0.0)
    rc, msg = load(a); assert rc != 0 and 'timestep' in msg
    # truncated blob / corrupt table of contents
    blob = pack_model(dict(walk_arrays))
    assert L.fb_model_load(blob[:200], 200, C.byref(h)) != 0
    assert L.fb_model_load(blob[:len(blob)//2], len(blob)//2, C.byref(h)) != 0 and b'outside the blob' in L.fb_last_error()
    assert L.fb_model_load(blob, len(blob), None) != 0
    assert L.fb_model_dim(None, b'nq') == -1


def test_no_cpu_fallback(walk_arrays):
    """Without a GPU the product path must raise, not silently compute on the CPU."""
    import torch
    from flybody_amd import engine
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    M = engine.Model(walk_arrays)
    with pytest.raises(engine.EngineError, match='no HIP device|hipGetDeviceCount|no CPU fallback'):
        engine.Batch(M, 4)
    # the package never references the oracle or the emulation build
    for root, _, files in os.walk(os.path.join(ROOT, 'flybody_amd')):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(root, f)).read()
                assert 'from oracle' not in src and 'import oracle' not in src and 'libflybody_emu' not in src, f


def test_a_library_without_a_declared_symbol_is_refused_at_load(monkeypatch):
    """load_library applies engine._SIGNATURES to the whole library: a symbol the table declares and the binary lacks is an EngineError that
    names the symbol and the build command, not a call without argtypes later."""
    from flybody_amd import engine
    monkeypatch.setattr(engine, '_libs', {})
    monkeypatch.setitem(engine._SIGNATURES, 'fb_no_such_call', (C.c_int, [C.c_void_p]))
    with pytest.raises(engine.EngineError, match=r'does not export fb_no_such_call.*g\.build\(\)'):
        engine.load_library()


def test_python_field_table_matches_header():
    """engine.FIELDS names every field of the header's field enum (FB_QPOS ... ) with the header's id, and no other."""
    from flybody_amd import engine
    hdr = open(os.path.join(ROOT, 'include', 'flybody_engine.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    block = next(b for b in re.findall(r'enum\s*\{(.*?)\}', hdr, flags=re.S) if 'FB_QPOS' in b)
    ids = {name: int(v) for name, v in re.findall(r'\bFB_([A-Z0-9_]+)\s*=\s*(\d+)', block)}
    assert len(ids) >= 40 and ids['QPOS'] == 0 and ids['CONTACT_FORCE'] == 39
    assert {name: f[0] for name, f in engine.FIELDS.items()} == ids


def test_python_warn_bits_match_header():
    """engine.WARN_BITS names every bit of the header's FB_WARN_* enum with the header's value, and no other."""
    from flybody_amd import engine
    hdr = open(os.path.join(ROOT, 'include', 'flybody_engine.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    block = next(b for b in re.findall(r'enum\s*\{(.*?)\}', hdr, flags=re.S) if 'FB_WARN_CONTACT_CAP' in b)
    bits = {name: int(v) for name, v in re.findall(r'\bFB_WARN_([A-Z0-9_]+)\s*=\s*(\d+)', block)}
    assert len(bits) >= 7 and bits['CONTACT_CAP'] == 1 and bits['MODEL_ID'] == 64
    assert engine.WARN_BITS == bits


_SCALARS = {'int': C.c_int, 'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint8_t': C.c_uint8, 'uint32_t': C.c_uint32, 'uint64_t': C.c_uint64,
            'float': C.c_float, 'double': C.c_double, 'size_t': C.c_size_t}
_STRUCT = r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;'


def _base(decl):
    """The type name a declaration starts with: 'const float *a' -> 'float'."""
    return [t for t in re.findall(r'\w+', decl) if t != 'const'][0]


def _kinds(decl, base=None):
    """The ctypes kinds that may declare one C parameter or return type (`base`: its type name, for the later declarators of 'const float
    *a, *b').  A scalar is the kind of its type name and void is None.  Any pointer is c_void_p, or the typed pointer that byref() of its
    pointee needs: POINTER(scalar) for a scalar's, POINTER(c_void_p) for a pointer's; `char*` is c_char_p."""
    base, stars = base or _base(decl), decl.count('*')
    if not stars:
        return (None,) if base == 'void' else (_SCALARS[base],)
    if base == 'char':
        return (C.c_char_p,)
    typed = (C.POINTER(C.c_void_p),) if stars > 1 else (C.POINTER(_SCALARS[base]),) if base in _SCALARS else ()
    return (C.c_void_p,) + typed


def _struct_fields(body):
    """[(field, ctypes kind)] of a struct's body, in order: a pointer is c_void_p, `double size[4]` is c_double*4."""
    out = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        for piece in decl.split(','):
            name, count = re.search(r'(\w+)\s*(?:\[(\d+)\])?\s*$', piece).groups()
            kind = C.c_void_p if '*' in piece else _SCALARS[_base(decl)]
            out.append((name, kind*int(count) if count else kind))
    return out


def _name(t):
    return getattr(t, '__name__', t)


def _check_declarations(header, prefix, signatures, mirrors):
    """A ctypes signature table {name: (restype, argtypes)} and the Structure mirrors {struct: mirror} of one library against the prototypes
    and structs of its header: an entry for every function and no others, as many argument types as parameters, each of the parameter's
    kind, the return type; a mirror for every struct, field by field.  Returns the names of the prototypes."""
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
    hdr = re.sub(r'^\s*#.*$', '', hdr, flags=re.M)                            # (preprocessor lines: an #endif in front of a prototype)
    structs = {name: body for body, name in re.findall(_STRUCT, hdr, flags=re.S)}
    protos = re.findall(r'([\w\s\*]+?)\b(%s\w+)\s*\(([^()]*)\)\s*;' % prefix, re.sub(_STRUCT, '', hdr, flags=re.S))
    for ret, name, params in protos:
        assert name in signatures, f'{name}: declared in {header}, no ctypes declaration'
        restype, argtypes = signatures[name]
        params = [] if params.strip() == 'void' else params.split(',')
        assert len(argtypes) == len(params), f'{name}: {len(argtypes)} argument types for {len(params)} parameters'
        for i, (t, prm) in enumerate(zip(argtypes, params)):
            assert any(t is k for k in _kinds(prm)), f'{name}: parameter {i} ({prm.strip()}) declared as {_name(t)}'
        assert restype is _kinds(ret)[0], f'{name}: return type {ret.strip()} declared as {_name(restype)}'
    assert set(signatures) == {name for _, name, _ in protos}
    assert set(mirrors) == set(structs), set(mirrors) ^ set(structs)
    for struct, mirror in mirrors.items():
        assert [(n, t) for n, t in mirror._fields_] == _struct_fields(structs[struct]), struct
    return {name for _, name, _ in protos}


def test_learner_ctypes_declarations_match_header():
    """fused._SIGNATURES against the prototypes of include/flybody_learner.h: an entry for every function (and for every lib().fbl_* call of
    fused.py), as many argument types as parameters, each of the parameter's kind, the return type; and the two Structure mirrors field by
    field.  A miscounted pointer would otherwise stay silent until it corrupts memory on a GPU."""
    from flybody_amd.dmpo import fused
    protos = _check_declarations('flybody_learner.h', 'fbl_', fused._SIGNATURES, {'fbl_gemm_op': fused._GemmOp, 'fbl_mpo_args': fused._MpoArgs})
    assert len(protos) >= 24 and {'fbl_sgemm_op', 'fbl_mpo_loss', 'fbl_nstep_add'} <= protos
    called = set(re.findall(r'lib\(\)\.(fbl_\w+)', open(os.path.join(ROOT, 'flybody_amd', 'dmpo', 'fused.py')).read()))
    assert len(called) >= 20 and called <= set(fused._SIGNATURES), called - set(fused._SIGNATURES)


def test_engine_ctypes_declarations_match_header():
    """engine._SIGNATURES against the prototypes of include/flybody_engine.h, as the learner's above: an entry for every function (and for
    every .fb_*( call of engine.py), the argument count, each parameter's kind, the return type; and the ten Structure mirrors field by
    field.  The engine's calls take device pointers from torch: ctypes would pass one as a C int where a declaration is missing."""
    from flybody_amd import engine
    mirrors = dict(fb_walk_dataset=engine._WalkDataset, fb_flight_dataset=engine._FlightDataset, fb_ik_config=engine._IKConfig,
                   fb_fd_config=engine._FDConfig, fb_rollout_config=engine._RolloutConfig, fb_feedback=engine._Feedback,
                   fb_lqr_config=engine._LQRConfig, fb_terrain=engine._Terrain, fb_ray_config=engine._RayConfig,
                   fb_control_law=engine._ControlLaw)
    protos = _check_declarations('flybody_engine.h', 'fb_', engine._SIGNATURES, mirrors)
    assert len(protos) >= 45 and {'fb_batch_lqr_backward', 'fb_batch_ray', 'fb_random_actions'} <= protos
    assert len(mirrors) == 10
    called = set(re.findall(r'\.(fb_\w+)\(', open(os.path.join(ROOT, 'flybody_amd', 'engine.py')).read()))
    assert len(called) >= 40 and called <= set(engine._SIGNATURES), called - set(engine._SIGNATURES)
