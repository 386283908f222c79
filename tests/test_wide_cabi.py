"""Host-side checks of SIGSVGD_FLAG_FP32_SWEEPS for RBF paths of 17 to 32 channels: with the bit, order 0,
the default stencil and 3 <= T <= 64 such a launch runs the register-resident kernel's 32-channel layout (csrc/gram_fast_wide.hip);
without it, and in every other case, every route and workspace figure is what it was.  What the workspace query answers with
and without the bit (tests/wide_plans.py restates the new plan, tests/plans.py the coverage kernel's), where the bit changes
nothing, what the partial solve decides before any device work, and -- on the C oracle alone -- that the inputs of
tests/test_gpu_wide.py would show a kernel that stops after its first 16 channels or drops its last one.  No device needed."""
import ctypes

import numpy as np
import pytest

from cabi import FAKE, lib, OK, UNSUPPORTED
from parity import rel_entry
from plans import device_cus, routed_generic_plan
from sigsvgd_amd import _lib, ops
from wide_plans import H, inputs, reference, wide_bytes, wide_shape

RBF, LINEAR, IMQ, RQ, M32, M52 = (_lib.STATIC_RBF, _lib.STATIC_LINEAR, _lib.STATIC_IMQ, _lib.STATIC_RQ, _lib.STATIC_MATERN32,
                                  _lib.STATIC_MATERN52)
FP32, YX, GENERIC, NAIVE = _lib.FLAG_FP32_SWEEPS, _lib.FLAG_Y_IS_X, _lib.FLAG_FORCE_GENERIC, _lib.FLAG_NAIVE_SOLVER
DS, TS = [17, 24, 31, 32], [3, 32, 33, 64]
# ordered with A != B, or Y_IS_X with A == B: a query that covers one plan (one tile and a ragged second one; past 256 workgroups)
SIZES = [(5, 6, 0), (9, 9, YX), (9, 100, 0), (70, 70, YX)]


def ws(A, B, T, d, n, kind, grad, flags):
    b = ctypes.c_size_t(12345)
    rc = lib().sigsvgd_gram_workspace_bytes(A, B, T, d, n, kind, grad, flags, ctypes.byref(b))
    return rc, b.value


@pytest.mark.parametrize("grad", [0, 1])
@pytest.mark.parametrize("A,B,yx", SIZES)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("d", DS)
def test_flagged_query_is_the_wide_plan_and_the_unflagged_one_the_coverage_kernel_s(d, T, A, B, yx, grad):
    cus = device_cus()
    assert wide_shape(T, d)
    got = ws(A, B, T, d, 0, RBF, grad, yx | FP32)
    assert got == (OK, wide_bytes(A, B, T, d, grad, bool(yx), cus))
    plain = ws(A, B, T, d, 0, RBF, grad, yx)
    route, pl = routed_generic_plan(A, B, T, d, 0, RBF, bool(grad), sym=bool(yx), cus=cus)
    assert route == "Generic" and plain == (OK, pl["bytes"] if grad else 512)
    assert got != plain


def test_the_geometry_has_a_ragged_tile_and_a_launch_past_the_grid():
    from wide_plans import wide_geometry

    assert wide_geometry(5, 6, False) == dict(rows_per_tile=4, items=12, grid=12, ntile=2)
    assert wide_geometry(9, 9, True) == dict(rows_per_tile=4, items=9 + 5 + 1, grid=15, ntile=3)
    g = wide_geometry(9, 100, False)
    assert g["items"] == 300 and g["grid"] == 256  # a workgroup takes more than one item


@pytest.mark.parametrize("grad", [0, 1])
def test_the_bit_still_changes_nothing_elsewhere(grad):
    cases = [(A, B, 64, 33, 0, RBF, f) for (A, B, f) in SIZES]                                  # d = 33
    cases += [(A, B, 65, 17, 0, RBF, f) for (A, B, f) in SIZES]                                 # T = 65
    cases += [(A, B, 20, 17, 1, RBF, f) for (A, B, f) in SIZES]                                 # dyadic order 1
    cases += [(A, B, 64, d, 0, RBF, f | NAIVE) for (A, B, f) in SIZES for d in (17, 32)]       # the first-order stencil
    cases += [(A, B, 64, d, 0, RBF, f | GENERIC) for (A, B, f) in SIZES for d in (17, 32)]
    cases += [(A, B, 64, 17, 0, k, f) for (A, B, f) in SIZES for k in (LINEAR, IMQ, RQ, M32, M52)]
    cases += [(A, B, 2, 17, 0, RBF, f) for (A, B, f) in SIZES]                                  # T = 2
    for A, B, T, d, n, kind, flags in cases:
        got = ws(A, B, T, d, n, kind, grad, flags | FP32)
        assert got[0] == OK and got == ws(A, B, T, d, n, kind, grad, flags), (A, B, T, d, n, kind, flags)
    # d = 16: RBF's own figure, with and without the bit; and not the 32-channel layout's formula by accident of the shape
    for (A, B, f) in SIZES:
        for T in TS:
            assert ws(A, B, T, 16, 0, RBF, grad, f | FP32) == ws(A, B, T, 16, 0, RBF, grad, f)


def test_takes_queries():
    for shape in [(5, 6, 64, 17), (9, 9, 3, 32), (9, 9, 65, 17), (9, 9, 64, 33)]:
        for grad in (False, True):
            assert ops.gram_takes(*shape, 0, RBF, grad, fp32_sweeps=True) is True


def test_the_partial_solve_keeps_refusing_more_than_16_channels():
    L = lib()
    for d in (17, 32):
        for flags in (0, FP32, FP32 | _lib.FLAG_FOLD_TILES):
            assert L.sigsvgd_gram_sym_partial(FAKE, 16, 64, d, _lib.F32, 1.0, RBF, flags, 0, 2, None, FAKE, FAKE, None, 0,
                                              None) == UNSUPPORTED
        for T in TS:
            assert L.sigsvgd_gram_sym_tile_rows(T, d) == 0
    assert L.sigsvgd_gram_sym_tile_rows(64, 17) == 0 and L.sigsvgd_gram_sym_tile_rows(64, 16) == 4
    # a Y_IS_X gradient query covers no partial plan at d > 16: the symmetric launch's bytes alone
    assert ws(9, 9, 64, 17, 0, RBF, 1, YX | FP32) == (OK, wide_bytes(9, 9, 64, 17, 1, True, device_cus()))


@pytest.mark.parametrize("d", [17, 31, 32])
def test_oracle_tells_a_kernel_that_loses_channels(d):
    """K of the first 16 channels alone, and K without the last channel (d = 32: channel 31, the one the kernel's d = 31
    instantiations leave out), are more than 1e-3 per entry from the full K on the inputs of the GPU parity test, whose
    tolerance is 1e-5: that test sees a kernel that stops after its first block of channels or treats d = 32 as d = 31"""
    from oracle import c_oracle

    A, B, T = 5, 6, 64
    K = reference(A, B, T, d)[0]
    assert 0.9 < K.min() and K.max() < 2.5
    X, Y = inputs(A, T, d, 0), inputs(B, T, d, 5)
    for keep in (16, d - 1):
        Kc = c_oracle.gram_fwd_bwd(np.ascontiguousarray(X[:, :, :keep]), np.ascontiguousarray(Y[:, :, :keep]), h=H, want_grad=False)[0]
        assert rel_entry(Kc, K, 1e-6) > 1e-3, (d, keep, rel_entry(Kc, K, 1e-6))
