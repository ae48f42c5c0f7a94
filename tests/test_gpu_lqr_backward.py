"""fb_batch_lqr_backward (csrc/fb_riccati.hpp: k_riccati_gemm on v_mfma_f64_16x16x4_f64, k_riccati_gain) on the MI355X, on
both engine builds: the assertions of tests/lqr_cases.py that tests/test_lqr_backward_emulation.py runs on the emulation build.  The
exact-integer product test is the one that pins the f64 C/D lane map of the matrix core; the emulation build cannot.

Measured on the MI355X (both builds print the same figures), kernel against the longdouble reference (numpy FP64 against it), largest
shape (275, 59, 2, 2) with mu given: K 3.1e-15 (2.6e-15), k 2.3e-15 (1.9e-15), P 1.1e-15 (1.2e-15), p 2.3e-15 (1.5e-15), dV 2.2e-16
(4.4e-16); worst over the shapes (64, 64, 1, 1): K 8.5e-15 (7.4e-15).  Against lqr.tvlqr: K 5.7e-16, P 3.7e-16.  Stationary: P_0
against lqr.lqr 1.8e-10 (tol 1e-10), against P_1 4.3e-16.  The whole table: DESIGN.md 23.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lqr_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def sync():
    import torch
    torch.cuda.synchronize()


@pytest.fixture(scope='module', params=[False, True], ids=['default', 'dense'])
def ctx(request):
    from flybody_amd import engine
    model = engine.Model.from_asset('walk_imitation', dense=request.param)
    make_batch = lambda: engine.Batch(model, 4, precision=64)
    return lc.Ctx(make_batch(), make_batch, dev=dev, np_=lambda t: t.cpu().numpy(), sync=sync,
                  tag='MI355X, ' + ('dense' if request.param else 'default') + ' build')


def test_gemm_is_exact_on_small_integers(ctx):
    lc.gemm_is_exact_on_small_integers(ctx)


@pytest.mark.parametrize('i', range(len(lc.SHAPES)), ids=['x'.join(map(str, s)) for s in lc.SHAPES])
def test_shape_matches_the_reference(ctx, i):
    lc.shape_matches_the_reference(ctx, i)


def test_plain_tvlqr(ctx):
    lc.plain_tvlqr(ctx)


def test_regularisation_shrinks_the_gain(ctx):
    lc.regularisation_shrinks_the_gain(ctx)


def test_dV_predicts_the_line_search(ctx):
    lc.dV_predicts_the_line_search(ctx)


def test_stationary_mode_is_lqr(ctx):
    lc.stationary_mode_is_lqr(ctx)


def test_failure_is_data(ctx):
    lc.failure_is_data(ctx)


def test_determinism_and_regrowth(ctx):
    lc.determinism_and_regrowth(ctx)


def test_hand_over_without_a_copy(ctx):
    lc.hand_over_without_a_copy(ctx)


def test_refusals(ctx):
    lc.refusals(ctx)


def test_an_fp32_batch_serves_and_a_side_stream_orders_the_call():
    """The call reads no environment: an FP32 batch computes the bits of an FP64 one; on a stream of the caller's the result is that of
    the current stream."""
    import torch
    from flybody_amd import engine
    model = engine.Model.from_asset('walk_imitation')
    pr = lc.problem(33, 5, 2, 2, 41)
    cs = [lc.Ctx(engine.Batch(model, 4, precision=p), None, dev, lambda t: t.cpu().numpy(), sync) for p in (64, 32)]
    out = [lc.as_numpy(c, lc.run(c, pr)) for c in cs]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    side = lc.as_numpy(cs[0], lc.run(cs[0], pr, stream=s.cuda_stream))
    for f in lc.ARRAYS:
        assert np.array_equal(out[0][f], out[1][f]) and np.array_equal(out[0][f], side[f]), f
