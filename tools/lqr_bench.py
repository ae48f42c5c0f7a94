#!/usr/bin/env python3
"""Time of fb_batch_lqr_backward (csrc/fb_riccati.hpp) beside the host recursion it replaces and beside itself without the
matrix core.

Walking-fly sizes (ndx 275, nu 59), T = 10 intervals, n_nom = 1, 8, 64, 512 nominals with A, B on the device (where transition_fd leaves
them); synthetic, well-conditioned inputs (A = 0.9 I-scaled noise, B normal, Q = G'G/ndx + 0.1 I, R = H'H/nu + I) -- the time does not
depend on the values as long as no nominal fails, which the tool checks:

    device      Batch.lqr_backward (want_P off): device events around a call that ends in a synchronise, after a warm-up call of the same
                shape (which grows the workspace)
    plain       the same call on a comparison build of the same sources with -DFB_RICCATI_NO_MFMA, where the tile primitive is its plain
                C++ branch (operands through LDS, 16 fma per lane and k-step) -- so the matrix core's share is a measurement.  The build
                is made here on first use (build_variants/, --build-only to make it where there is no GPU); --no-plain skips it
    host        lqr.tvlqr in numpy on the same inputs, wall clock, INCLUDING the copy of A, B to the host and of K back to the device
The three are alternated --passes times (default 3) and every pass is reported.  gflops: 2 (2 ndx^3 + 3 ndx^2 nu + ndx nu^2) +
2 nu^2 ndx + nu^3 / 3 per interval and nominal (the short form of P_t: mu is NULL), over the mean device time; fp64_matrix_peak_fraction
against 78.6 TFLOP/s, AMD's published FP64 matrix peak of the MI355X.  One JSON line.

    python tools/lqr_bench.py [--sizes 1,8,64,512] [--horizon 10] [--passes 3] [--no-plain] [--no-host] [--build-only]
"""
import argparse, json, os, subprocess, sys, time
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, '..')
sys.path.insert(0, ROOT)
import numpy as np

PLAIN_LIB = os.path.join(ROOT, 'build_variants', 'libflybody_hip_riccati_plain.so')
PEAK = 78.6e12


def build_plain():
    """The engine sources with -DFB_RICCATI_NO_MFMA (the bench's comparison build only; no product path loads it)."""
    import __graft_entry__ as g
    if g._lib_hash(PLAIN_LIB) == g._source_hash():
        return PLAIN_LIB
    os.makedirs(os.path.dirname(PLAIN_LIB), exist_ok=True)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-shared', '-fPIC', '-DFB_RICCATI_NO_MFMA=1'] + g.hip_flags() +
                          ['-DFB_BUILD_ID="%s"' % g._source_hash(), '-o', PLAIN_LIB, g.HIP_SRC], cwd=ROOT)
    return PLAIN_LIB


ap = argparse.ArgumentParser()
ap.add_argument('--sizes', default='1,8,64,512'); ap.add_argument('--horizon', type=int, default=10); ap.add_argument('--passes', type=int, default=3)
ap.add_argument('--ndx', type=int, default=275); ap.add_argument('--nu', type=int, default=59)
ap.add_argument('--no-plain', action='store_true'); ap.add_argument('--no-host', action='store_true'); ap.add_argument('--build-only', action='store_true')
a = ap.parse_args()
if a.build_only:
    print(build_plain()); sys.exit(0)

import torch
from flybody_amd import engine, lqr
torch.cuda.set_device(0)
st = torch.cuda.current_stream()
T, ndx, nu = a.horizon, a.ndx, a.nu
model = engine.Model.from_asset('walk_imitation')
batches = {'device': engine.Batch(model, 1, precision=64)}
if not a.no_plain:
    batches['plain'] = engine.Batch(engine.Model(model.arrays, lib_path=build_plain()), 1, precision=64)


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st); r = f(); e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)*1e-3, r


def host(A, B, Q, R):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    K, _ = lqr.tvlqr(A.cpu().numpy(), B.cpu().numpy(), Q.cpu().numpy(), R.cpu().numpy())
    Kd = torch.from_numpy(K).cuda()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, Kd


flop = T*(2*(2*ndx**3 + 3*ndx*ndx*nu + ndx*nu*nu) + 2*nu*nu*ndx + nu**3/3)
out = dict(tool='lqr_bench', engine=engine.version(), horizon=T, ndx=ndx, nu=nu, passes=a.passes, flop_per_nominal=round(flop), results=[])
mean = lambda x: float(np.mean(x))
g = torch.Generator(device='cuda'); g.manual_seed(0)
rn = lambda *s: torch.randn(*s, generator=g, device='cuda', dtype=torch.float64)
G, H = rn(ndx, ndx), rn(nu, nu)
Q = (G.T @ G/ndx + 0.1*torch.eye(ndx, device='cuda', dtype=torch.float64)).contiguous()
R = (H.T @ H/nu + torch.eye(nu, device='cuda', dtype=torch.float64)).contiguous()
for size in a.sizes.split(','):
    n = int(size)
    A = (0.5*torch.eye(ndx, device='cuda', dtype=torch.float64) + 0.5/ndx**0.5*rn(n, T, ndx, ndx)).contiguous()
    B = rn(n, T, ndx, nu)
    calls = {name: (lambda b=b: b.lqr_backward(A, B, Q, R)) for name, b in batches.items()}
    res = {name: timed(f)[1] for name, f in calls.items()}                       # warm-up: grows the workspace
    times = {name: [] for name in calls}; hs = []; gap = None
    for _ in range(a.passes):
        for name, f in calls.items():
            t, res[name] = timed(f); times[name].append(t)
        if not a.no_host:
            t, Kh = host(A, B, Q, R); hs.append(t)
            gap = float(((res['device'].K - Kh).abs().max()/Kh.abs().max()).item())
    row = dict(n_nom=n, status_any=int(res['device'].status.max().item()), device_s=[round(x, 6) for x in times['device']],
               gflops=round(n*flop/mean(times['device'])*1e-9, 1), fp64_matrix_peak_fraction=round(n*flop/mean(times['device'])/PEAK, 4))
    if 'plain' in times:
        row.update(plain_s=[round(x, 6) for x in times['plain']], plain_over_device=round(mean(times['plain'])/mean(times['device']), 2),
                   plain_equals_device_bits=bool(torch.equal(res['plain'].K, res['device'].K)))
    if hs:
        row.update(host_s=[round(x, 5) for x in hs], host_over_device=round(mean(hs)/mean(times['device']), 2), max_rel_diff_K_to_host=float('%.1e' % gap))
    out['results'].append(row)
    print('lqr_bench:', json.dumps(row), file=sys.stderr, flush=True)
    del A, B, res
print(json.dumps(out))
