"""Host-side checks of the static-kernel kinds SIGSVGD_STATIC_IMQ (2) and SIGSVGD_STATIC_RQ (3) (include/sigsvgd_hip.h,
DESIGN.md section 5.15): which entry points accept them, what their queries answer, and what stays refused.  No device
needed: every call below returns before any device work."""
import ctypes

import pytest

from cabi import BADARG, FAKE, lib, OK, UNSUPPORTED
from sigsvgd_amd import _lib, ops

RBF, LINEAR, IMQ, RQ = _lib.STATIC_RBF, _lib.STATIC_LINEAR, _lib.STATIC_IMQ, _lib.STATIC_RQ
NAIVE = _lib.FLAG_NAIVE_SOLVER
NEW = [IMQ, RQ]


def query(name, *args):
    b = ctypes.c_size_t(12345)
    rc = getattr(lib(), "sigsvgd_" + name)(*args, ctypes.byref(b))
    return rc, b.value


def test_constants_and_abi():
    assert (IMQ, RQ) == (2, 3) and _lib.ABI_VERSION == 10 and lib().sigsvgd_abi_version() == 10


@pytest.mark.parametrize("kind", NEW)
def test_takes_queries_answer_as_for_the_linear_kernel(kind):
    assert ops.gram_takes(4, 4, 64, 7, 0, static_kind=kind) is True
    assert ops.gram_takes(4, 4, 4000, 3, 0, static_kind=kind) is False
    for shape in [(4, 4, 64, 7, 0), (4, 4, 4000, 3, 0), (5, 6, 20, 17, 0), (5, 6, 10, 3, 2), (3, 3, 300, 2, 0), (2, 2, 200, 4, 2),
                  (64, 64, 6, 2, 0)]:
        for grad in (False, True):
            assert ops.gram_takes(*shape, static_kind=kind, want_grad=grad) == ops.gram_takes(*shape, static_kind=LINEAR, want_grad=grad)
    for shape in [(3, 4, 70, 66, 3, 0), (2, 3, 9, 12, 17, 2), (2, 2, 9000, 9000, 2, 0), (2, 2, 300, 300, 2, 6)]:
        assert ops.gram_long2_takes(*shape, static_kind=kind) == ops.gram_long2_takes(*shape, static_kind=LINEAR)
        A, _, TX, TY, d, n = shape
        assert ops.pair_takes(A, TX, TY, d, n, static_kind=kind) == ops.pair_takes(A, TX, TY, d, n, static_kind=LINEAR)
    assert ops.gram_long2_takes(3, 4, 70, 66, 3, 0, static_kind=kind) and not ops.gram_long2_takes(2, 2, 9000, 9000, 2, 0, static_kind=kind)
    for shape in [(12, 70, 3, 0), (10, 20, 2, 2), (4, 9000, 2, 0)]:
        for world in (1, 2, 3):
            assert (ops.gram_long_partial_takes(*shape, static_kind=kind, tile_stride=world)
                    == ops.gram_long_partial_takes(*shape, static_kind=LINEAR, tile_stride=world))
    assert ops.gram_long_partial_takes(12, 70, 3, 0, static_kind=kind, tile_stride=2)


@pytest.mark.parametrize("kind", NEW)
def test_workspace_bytes(kind):
    """The plans do not depend on the kind: the long route's figures are RBF's, the coverage kernel's the linear kernel's
    (the two kinds take the plan FORCE_GENERIC selects, so that figure of the linear kernel too)."""
    for shape in [(3, 4, 70, 66, 3, 0), (2, 3, 9, 12, 17, 2), (5, 5, 300, 300, 2, 0)]:
        for grad in (0, 1):
            got = query("gram_long_workspace_bytes", *shape, kind, grad, 0)
            assert got[0] == OK and got == query("gram_long_workspace_bytes", *shape, RBF, grad, 0)
            A, _, TX, TY, d, n = shape
            got = query("pair_workspace_bytes", A, TX, TY, d, n, kind, grad, 0)
            assert got[0] == OK and got == query("pair_workspace_bytes", A, TX, TY, d, n, RBF, grad, 0)
        for wx, wy in [(1, 1), (1, 0), (0, 0)]:
            got = query("gram_long2_workspace_bytes", *shape, kind, wx, wy, 0)
            assert got[0] == OK and got == query("gram_long2_workspace_bytes", *shape, RBF, wx, wy, 0)
    for off in (0, 1):
        got = query("gram_long_partial_workspace_bytes", 12, 70, 3, 0, kind, _lib.FLAG_FOLD_TILES, off, 2)
        assert got[0] == OK and got == query("gram_long_partial_workspace_bytes", 12, 70, 3, 0, RBF, _lib.FLAG_FOLD_TILES, off, 2)
    for shape in [(5, 6, 4, 2, 3), (5, 6, 20, 17, 0), (5, 6, 128, 14, 0), (64, 64, 6, 2, 0), (4, 4, 64, 7, 0)]:
        for grad in (0, 1):
            for flags in (0, _lib.FLAG_Y_IS_X, NAIVE, _lib.FLAG_FORCE_GENERIC):
                got = query("gram_workspace_bytes", *shape, kind, grad, flags)
                assert got[0] == OK and got == query("gram_workspace_bytes", *shape, LINEAR, grad, flags)
                assert got == query("gram_workspace_bytes", *shape, LINEAR, grad, flags | _lib.FLAG_FORCE_GENERIC)


@pytest.mark.parametrize("kind", NEW)
def test_naive_solver_is_unsupported_on_the_long_route(kind):
    for name, args in [("gram_long_workspace_bytes", (3, 4, 70, 66, 3, 0, kind, 1, NAIVE)),
                       ("pair_workspace_bytes", (3, 70, 66, 3, 0, kind, 1, NAIVE)),
                       ("gram_long2_workspace_bytes", (3, 4, 70, 66, 3, 0, kind, 1, 1, NAIVE)),
                       ("gram_long_partial_workspace_bytes", (12, 70, 3, 0, kind, NAIVE, 0, 2))]:
        assert query(name, *args)[0] == UNSUPPORTED, name
        msg = _lib.last_error()
        assert "NAIVE_SOLVER" in msg and "default stencil" in msg, msg
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    assert lib().sigsvgd_gram_long_partial_plan(12, 70, 3, 0, kind, NAIVE, 2, ctypes.byref(r), ctypes.byref(c)) == UNSUPPORTED
    # the launches say the same (after their argument checks, before any device work)
    L = lib()
    assert L.sigsvgd_gram_long_fwd(FAKE, FAKE, 3, 4, 70, 66, 3, _lib.F64, 1.0, 0, kind, NAIVE, FAKE, None, 0, None) == UNSUPPORTED
    assert L.sigsvgd_gram_long_fwd_bwd(FAKE, FAKE, 3, 4, 70, 66, 3, _lib.F64, 1.0, 0, kind, NAIVE, None, FAKE, FAKE, None, 0,
                                       None) == UNSUPPORTED
    assert L.sigsvgd_pair_fwd(FAKE, FAKE, 3, 70, 66, 3, _lib.F64, 1.0, 0, kind, NAIVE, FAKE, None, 0, None) == UNSUPPORTED
    assert L.sigsvgd_gram_long_fwd_bwd2(FAKE, FAKE, 3, 4, 70, 66, 3, _lib.F64, 1.0, 0, kind, NAIVE, None, FAKE, FAKE, FAKE, None,
                                        0, None) == UNSUPPORTED
    assert L.sigsvgd_gram_long_sym_partial(FAKE, 12, 70, 3, _lib.F64, 1.0, 0, kind, NAIVE, 0, 2, None, FAKE, FAKE, None, 0,
                                           None) == UNSUPPORTED
    assert "default stencil" in _lib.last_error()
    # RBF and the linear kernel keep the first-order solver there
    for k in (RBF, LINEAR):
        assert query("gram_long_workspace_bytes", 3, 4, 70, 66, 3, 0, k, 1, NAIVE)[0] == OK
    # and the coverage kernel has it for every kind
    assert query("gram_workspace_bytes", 5, 6, 20, 3, 0, kind, 1, NAIVE)[0] == OK


@pytest.mark.parametrize("bad", [5, 9, 4, -1])
def test_other_kinds_stay_invalid(bad):
    assert query("gram_workspace_bytes", 4, 4, 64, 7, 0, bad, 1, 0)[0] == BADARG
    assert query("gram_long_workspace_bytes", 3, 4, 70, 66, 3, 0, bad, 1, 0)[0] == BADARG
    assert query("pair_workspace_bytes", 3, 70, 66, 3, 0, bad, 1, 0)[0] == BADARG
    assert query("gram_long2_workspace_bytes", 3, 4, 70, 66, 3, 0, bad, 1, 1, 0)[0] == BADARG
    assert query("gram_long_partial_workspace_bytes", 12, 70, 3, 0, bad, 0, 0, 2)[0] == BADARG
    L = lib()
    assert L.sigsvgd_gram_fwd(FAKE, FAKE, 4, 4, 64, 7, _lib.F64, 1.0, 0, bad, 0, FAKE, None, 0, None) == BADARG
    assert L.sigsvgd_gram_long_fwd(FAKE, FAKE, 3, 4, 70, 66, 3, _lib.F64, 1.0, 0, bad, 0, FAKE, None, 0, None) == BADARG


@pytest.mark.parametrize("kind", NEW)
@pytest.mark.parametrize("inv_h", [0.0, -1.0, float("nan")])
def test_bandwidth_must_be_positive(kind, inv_h):
    L = lib()
    assert L.sigsvgd_gram_fwd(FAKE, FAKE, 4, 4, 64, 7, _lib.F64, inv_h, 0, kind, 0, FAKE, None, 0, None) == BADARG
    assert "inv_h > 0" in _lib.last_error()
    assert L.sigsvgd_gram_fwd_bwd(FAKE, FAKE, 4, 4, 64, 7, _lib.F64, inv_h, 0, kind, 0, None, FAKE, FAKE, None, 0, None) == BADARG
    assert L.sigsvgd_gram_long_fwd(FAKE, FAKE, 3, 4, 70, 66, 3, _lib.F64, inv_h, 0, kind, 0, FAKE, None, 0, None) == BADARG
    assert "inv_h > 0" in _lib.last_error()
    assert L.sigsvgd_pair_fwd_bwd(FAKE, FAKE, 3, 70, 66, 3, _lib.F64, inv_h, 0, kind, 0, None, FAKE, FAKE, FAKE, None, 0,
                                  None) == BADARG
    assert L.sigsvgd_gram_long_fwd_bwd2(FAKE, FAKE, 3, 4, 70, 66, 3, _lib.F64, inv_h, 0, kind, 0, None, FAKE, FAKE, FAKE, None, 0,
                                        None) == BADARG
    assert L.sigsvgd_gram_long_sym_partial(FAKE, 12, 70, 3, _lib.F64, inv_h, 0, kind, 0, 0, 2, None, FAKE, FAKE, None, 0,
                                           None) == BADARG


@pytest.mark.parametrize("kind", NEW)
def test_fused_partial_solve_stays_rbf_only(kind):
    L = lib()
    rc = L.sigsvgd_gram_sym_partial(FAKE, 16, 64, 7, _lib.F32, 1.0, kind, 0, 0, 2, None, FAKE, FAKE, None, 0, None)
    assert rc == UNSUPPORTED and "RBF" in _lib.last_error()


def test_sharded_routes(monkeypatch):
    """ShardedSigSVGD's route for kinds 2 and 3 (host-only queries): never the fused partial solve; row-wise where the
    coverage kernel takes the rows, the long partial solve where it does not; and the row-wise solver of a shape only the
    long route takes is ops.gram_long_fwd_bwd."""
    import torch

    from sigsvgd_amd.distributed import ShardedSigSVGD

    for kind in NEW:
        sh = ShardedSigSVGD(1.0, 0.1, static_kind=kind)
        assert sh._route_of(8, torch.zeros(8, 64, 7), 1) == "rowwise"
        assert sh._route_of(8, torch.zeros(8, 300, 2), 1) == "long_partial"
        assert ShardedSigSVGD(1.0, 0.1, static_kind=kind, long_partial=False)._route_of(8, torch.zeros(8, 300, 2), 1) == "rowwise"
        calls = []
        monkeypatch.setattr(ops, "gram_fwd_bwd", lambda *a, **k: calls.append(("fused", a[3:])))
        monkeypatch.setattr(ops, "gram_long_fwd_bwd", lambda *a, **k: calls.append(("long", a[3:])))
        sh.rows_fn(torch.zeros(4, 64, 7), torch.zeros(8, 64, 7), 1.0)
        sh.rows_fn(torch.zeros(4, 300, 2), torch.zeros(8, 300, 2), 1.0)
        assert calls == [("fused", (0, kind)), ("long", (0, kind))]
