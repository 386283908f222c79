"""Host-side checks of SIGSVGD_FLAG_FP32_SWEEPS (128; include/sigsvgd_hip.h): the opt-in that sends
the IMQ and rational-quadratic static kernels to the register-resident kernel at that kernel's shapes.  What the workspace
query answers with and without the bit, where the bit changes nothing, and what `sigsvgd_gram_sym_partial` decides before
any device work.  No device needed."""
import ctypes

import pytest

from cabi import FAKE, lib, OK, UNSUPPORTED
from sigsvgd_amd import _lib, ops

RBF, LINEAR, IMQ, RQ, M32, M52 = (_lib.STATIC_RBF, _lib.STATIC_LINEAR, _lib.STATIC_IMQ, _lib.STATIC_RQ, _lib.STATIC_MATERN32,
                                  _lib.STATIC_MATERN52)
FP32, YX, GENERIC, NAIVE = _lib.FLAG_FP32_SWEEPS, _lib.FLAG_Y_IS_X, _lib.FLAG_FORCE_GENERIC, _lib.FLAG_NAIVE_SOLVER
NEW = [IMQ, RQ]
SHAPES = [(9, 5, 3, 2), (17, 17, 64, 7), (5, 6, 50, 16)]


def ws(A, B, T, d, n, kind, grad, flags):
    b = ctypes.c_size_t(12345)
    rc = lib().sigsvgd_gram_workspace_bytes(A, B, T, d, n, kind, grad, flags, ctypes.byref(b))
    return rc, b.value


def test_the_flag_is_bit_128():
    assert FP32 == 128 and _lib.ABI_VERSION == 10 and lib().sigsvgd_abi_version() == 10
    assert ops._flags(False, False, False, False, fp32_sweeps=True) == 128 and ops._flags(False, True, True, False) == 6


@pytest.mark.parametrize("kind", NEW)
@pytest.mark.parametrize("yx", [0, YX])
@pytest.mark.parametrize("grad", [0, 1])
@pytest.mark.parametrize("A,B,T,d", SHAPES)
def test_workspace_is_the_rbf_launch_s_with_the_flag_and_the_coverage_kernel_s_without(A, B, T, d, grad, yx, kind):
    got = ws(A, B, T, d, 0, kind, grad, yx | FP32)
    assert got[0] == OK and got == ws(A, B, T, d, 0, RBF, grad, yx)
    plain = ws(A, B, T, d, 0, kind, grad, yx)
    assert plain[0] == OK and plain == ws(A, B, T, d, 0, kind, grad, yx | GENERIC)


@pytest.mark.parametrize("grad", [0, 1])
def test_the_flag_changes_nothing_elsewhere(grad):
    cases = [(17, 17, 64, 7, 0, k, f) for k in (RBF, LINEAR, M32, M52) for f in (0, YX)]
    cases += [(9, 9, 65, 7, 0, k, f) for k in NEW for f in (0, YX)]            # T = 65
    cases += [(9, 9, 20, 3, 1, k, f) for k in NEW for f in (0, YX)]            # dyadic order 1
    cases += [(9, 5, 20, 3, 0, k, NAIVE) for k in NEW]                          # the first-order stencil
    cases += [(17, 17, 64, 7, 0, k, GENERIC | f) for k in NEW for f in (0, YX)]
    for A, B, T, d, n, kind, flags in cases:
        got = ws(A, B, T, d, n, kind, grad, flags | FP32)
        assert got[0] == OK and got == ws(A, B, T, d, n, kind, grad, flags), (A, B, T, d, n, kind, flags)


@pytest.mark.parametrize("kind", NEW)
def test_one_channel_gradient_launches_stay_on_the_coverage_kernel(kind):
    for flags in (0, YX):
        assert ws(9, 9, 20, 1, 0, kind, 1, flags | FP32) == ws(9, 9, 20, 1, 0, kind, 1, flags)
    # forward only, one channel: the register-resident kernel, as for RBF
    assert ws(9, 5, 20, 1, 0, kind, 0, FP32) == ws(9, 5, 20, 1, 0, RBF, 0, 0)


@pytest.mark.parametrize("kind", NEW)
def test_takes_queries(kind):
    for shape in [(9, 5, 3, 2), (17, 17, 64, 7), (4, 4, 4000, 3), (9, 9, 65, 7)]:
        for grad in (False, True):
            assert ops.gram_takes(*shape, 0, kind, grad, fp32_sweeps=True) == ops.gram_takes(*shape, 0, kind, grad)


@pytest.mark.parametrize("kind", NEW)
def test_partial_solve_argument_rules(kind):
    """decided before any device work: without the flag and at 65 <= T <= 128 the kinds are refused as before; with it at
    T <= 64 the call gets past the route (and is then refused for its tile arguments, still before device work)"""
    L = lib()
    part = lambda T, flags, off=0, stride=2: L.sigsvgd_gram_sym_partial(FAKE, 16, T, 7, _lib.F32, 1.0, kind, flags, off, stride,
                                                                        None, FAKE, FAKE, None, 0, None)
    assert part(64, 0) == UNSUPPORTED and "FP32_SWEEPS" in _lib.last_error()
    assert part(65, FP32) == UNSUPPORTED and part(128, FP32) == UNSUPPORTED
    assert part(64, FP32 | GENERIC) == UNSUPPORTED
    assert part(64, FP32, off=2) == -1 and "tile_offset" in _lib.last_error()
    assert part(64, FP32, stride=0) == -1
    for other in (LINEAR, M32, M52):
        assert L.sigsvgd_gram_sym_partial(FAKE, 16, 64, 7, _lib.F32, 1.0, other, FP32, 0, 2, None, FAKE, FAKE, None, 0,
                                          None) == UNSUPPORTED
    assert L.sigsvgd_gram_sym_tile_rows(64, 7) == 8  # (the ownership unit does not depend on the kind)
