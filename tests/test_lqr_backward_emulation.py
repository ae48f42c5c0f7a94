"""fb_batch_lqr_backward (csrc/fb_riccati.hpp: k_riccati_gemm, k_riccati_gain) through the kernel-source emulation build,
where the tile primitive is its plain C++ branch and everything else -- indexing, edges, the gain kernel, the host loop -- is the source
the GPU runs.  No GPU needed.  The assertions are those of tests/lqr_cases.py, which tests/test_gpu_lqr_backward.py runs on the MI355X.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lqr_cases as lc  # noqa: E402
from test_deriv_emulation import _load  # noqa: E402
from test_rollout_emulation import emu_lib  # noqa: E402,F401  (the emulation library's fixture)


@pytest.fixture(scope='module')
def ctx(emu_lib):  # noqa: F811
    import torch
    from flybody_amd import engine
    model, _, _ = _load('walk_imitation', emu_lib)
    make_batch = lambda: engine.Batch(model, 1, precision=64)
    return lc.Ctx(make_batch(), make_batch, dev=lambda x: torch.from_numpy(np.ascontiguousarray(x)), np_=lambda t: t.numpy(), tag='emulation')


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


def test_any_batch_serves(emu_lib):  # noqa: F811
    """The call reads no environment: an FP32 batch computes the same bits."""
    import torch
    from flybody_amd import engine
    model, _, _ = _load('walk_imitation', emu_lib)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    pr = lc.problem(5, 2, 2, 2, 41)
    cs = [lc.Ctx(engine.Batch(model, 1, precision=p), None, dev, lambda t: t.numpy()) for p in (64, 32)]
    out = [lc.as_numpy(c, lc.run(c, pr)) for c in cs]
    for f in lc.ARRAYS:
        assert np.array_equal(out[0][f], out[1][f]), f
