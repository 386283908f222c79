"""Host-side checks of the long-path Gram entry points (`sigsvgd_gram_long_*`, include/sigsvgd_hip.h) and of the routing
predicate `ops.gram_takes`; no device needed (every call below returns before any device work)."""
import ctypes

import pytest

from cabi import assert_exported, BADARG, FAKE, lib, UNSUPPORTED
from plans import device_cus, long_plan
from sigsvgd_amd import _lib, ops

NAMES = ("sigsvgd_gram_long_workspace_bytes", "sigsvgd_gram_long_fwd", "sigsvgd_gram_long_fwd_bwd")


def long_ws(A, B, TX, TY, d, n, kind=_lib.STATIC_RBF, want_grad=1, flags=0, out=True):
    b = ctypes.c_size_t(12345)
    rc = lib().sigsvgd_gram_long_workspace_bytes(A, B, TX, TY, d, n, kind, want_grad, flags, ctypes.byref(b) if out else None)
    return rc, b.value


def gram_ws_rc(A, B, T, d, n, want_grad=1):
    b = ctypes.c_size_t(0)
    return lib().sigsvgd_gram_workspace_bytes(A, B, T, d, n, _lib.STATIC_RBF, want_grad, 0, ctypes.byref(b))


def test_long_symbols_exported():
    assert_exported(NAMES, abi=10)


@pytest.mark.parametrize("A,B,TX,TY,d,n,old", [(4, 4, 400, 400, 3, 0, True), (2, 2, 200, 200, 4, 2, True),
                                               (2, 3, 1000, 150, 2, 0, False)])
def test_long_query_takes_what_the_fused_route_refuses(A, B, TX, TY, d, n, old):
    for kind in (_lib.STATIC_RBF, _lib.STATIC_LINEAR):
        rc, b = long_ws(A, B, TX, TY, d, n, kind)
        assert rc == 0 and b > 0, _lib.last_error()
    if old:  # the existing route keeps its contract at these shapes
        assert gram_ws_rc(A, B, TX, d, n, 1) == UNSUPPORTED
        assert gram_ws_rc(A, B, TX, d, n, 0) == UNSUPPORTED


def test_long_query_refuses_grids_past_8192():
    assert long_ws(1, 2, 129, 129, 2, 6)[0] == 0  # P = Q = 8192: the edge is taken
    for (TX, TY, n) in [(8194, 10, 0), (10, 8194, 0), (130, 129, 6), (129, 130, 6), (10, 1000, 4)]:
        rc, _ = long_ws(1, 2, TX, TY, 2, n)
        assert rc == UNSUPPORTED
        assert "8192" in _lib.last_error()


@pytest.mark.parametrize("case", ["A<1", "B<1", "TX<2", "TY<2", "d<1", "kind", "flags", "sym_AB", "sym_T", "order",
                                  "null_bytes"])
def test_long_bad_arguments(case):
    args = dict(A=3, B=3, TX=300, TY=300, d=2, n=0, kind=_lib.STATIC_RBF, flags=0)
    upd = {"A<1": dict(A=0), "B<1": dict(B=0), "TX<2": dict(TX=1), "TY<2": dict(TY=1), "d<1": dict(d=0), "kind": dict(kind=5),
           "flags": dict(flags=_lib.FLAG_FORCE_GENERIC), "sym_AB": dict(B=4, flags=_lib.FLAG_SYM),
           "sym_T": dict(TY=200, flags=_lib.FLAG_SYM), "order": dict(n=11), "null_bytes": {}}[case]
    a = {**args, **upd}
    rc, _ = long_ws(a["A"], a["B"], a["TX"], a["TY"], a["d"], a["n"], a["kind"], 1, a["flags"], out=case != "null_bytes")
    assert rc == BADARG, _lib.last_error()
    if case == "null_bytes":
        return
    L = lib()
    rc = L.sigsvgd_gram_long_fwd_bwd(FAKE, FAKE, a["A"], a["B"], a["TX"], a["TY"], a["d"], _lib.F32, 1.0, a["n"], a["kind"],
                                     a["flags"], None, FAKE, FAKE, FAKE, 1 << 30, None)
    assert rc == BADARG, _lib.last_error()
    if not case.startswith("sym"):  # (SYM is a backward weighting: the forward checks it too, as the Gram entry points do)
        rc = L.sigsvgd_gram_long_fwd(FAKE, FAKE, a["A"], a["B"], a["TX"], a["TY"], a["d"], _lib.F32, 1.0, a["n"], a["kind"],
                                     a["flags"], FAKE, FAKE, 1 << 30, None)
        assert rc == BADARG, _lib.last_error()


def test_long_launch_argument_checks():
    L = lib()
    base = (FAKE, FAKE, 3, 3, 300, 300, 2)
    # null pointers, bad dtype, RBF without a bandwidth, no gradient output: refused before any device work
    assert L.sigsvgd_gram_long_fwd(None, FAKE, 3, 3, 300, 300, 2, _lib.F32, 1.0, 0, 0, 0, FAKE, None, 0, None) == BADARG
    assert L.sigsvgd_gram_long_fwd(*base, 7, 1.0, 0, 0, 0, FAKE, None, 0, None) == BADARG
    assert L.sigsvgd_gram_long_fwd(*base, _lib.F32, 0.0, 0, _lib.STATIC_RBF, 0, FAKE, None, 0, None) == BADARG
    assert L.sigsvgd_gram_long_fwd_bwd(*base, _lib.F32, 1.0, 0, 0, 0, None, FAKE, None, FAKE, 1 << 30, None) == BADARG
    # accepted flags
    for f in (_lib.FLAG_NAIVE_SOLVER, _lib.FLAG_Y_IS_X, _lib.FLAG_SYM, _lib.FLAG_SYM | _lib.FLAG_NAIVE_SOLVER):
        assert long_ws(3, 3, 300, 300, 2, 0, flags=f)[0] == 0, _lib.last_error()


def test_long_forward_needs_no_scratch():
    for (A, B, TX, TY, d, n) in [(4, 4, 400, 400, 3, 0), (2, 2, 200, 200, 4, 2), (16, 16, 2048, 2048, 2, 0)]:
        assert long_ws(A, B, TX, TY, d, n, want_grad=0) == (0, 0)
        rc, b = long_ws(A, B, TX, TY, d, n, want_grad=1)
        assert rc == 0 and b > 0
    # Y_IS_X changes nothing
    assert long_ws(4, 4, 400, 400, 3, 0, flags=_lib.FLAG_Y_IS_X) == long_ws(4, 4, 400, 400, 3, 0)
    # the gradient scratch is bounded by the 1 GiB cap on per-wave scratch plus the slabs
    rc, b = long_ws(64, 64, 1025, 1025, 4, 0)
    assert rc == 0 and b < (1 << 30) + 64 * 64 * 1025 * 4 * 8 + 4096


def test_routing_predicate():
    assert ops.gram_takes(4, 4, 64, 7, 0) is True
    assert ops.gram_takes(4, 4, 400, 3, 0) is False
    assert ops.gram_takes(4, 4, 400, 3, 0, want_grad=False) is False
    assert ops.gram_takes(2, 2, 200, 4, 2) is False
    assert ops.gram_takes(2, 2, 20, 4, 2, want_grad=False, y_is_x=True) is True
    with pytest.raises(RuntimeError):  # a bad argument is an error, not a route
        ops.gram_takes(4, 4, 64, 7, 0, static_kind=9)


def test_plan_helper_matches_workspace_query():
    """tests/plans.long_plan mirrors long_make_plan: its bytes are the library's over shapes that reach every branch of
    the plan (ring wrap, nrow = 1, JC from 32 down to 1, the 1 GiB scratch cap, the LDS limit)."""
    cus = device_cus()
    shapes = [(1, 1, 2, 2), (3, 4, 300, 300), (1, 2, 129, 129), (2, 3, 129, 130), (2, 2, 257, 258), (2, 2, 513, 514),
              (2, 2, 9, 9), (2, 3, 5, 9), (1, 2, 9, 3), (3, 2, 150, 400), (2, 3, 66, 258), (1, 1, 300, 2), (1, 1, 2, 300),
              (64, 64, 40, 40), (40, 60, 40, 40), (500, 700, 20, 20), (64, 64, 1025, 1025), (16, 16, 2048, 2048)]
    seen = set()
    for (A, B, M, N) in shapes:
        for n in (0, 1, 2, 3, 6, 7, 8, 10):
            for d in (1, 2, 17, 183, 184):
                for want_grad in (0, 1):
                    rc, b = long_ws(A, B, M, N, d, n, want_grad=want_grad)
                    pl = long_plan(A, B, M, N, d, n, want_grad, cus)
                    assert (rc == UNSUPPORTED) == (pl is None), (A, B, M, N, d, n, want_grad, rc)
                    if pl is None:
                        continue
                    assert rc == 0 and b == pl["bytes"], (A, B, M, N, d, n, want_grad, b, pl)
                    seen.add(pl["JC"])
    assert {1, 2, 4, 32} <= seen


def test_channel_limit():
    """Up to 16 channels the ring fill keeps a point in registers, past 16 it reads global memory; the LDS holds the band's
    points of X, so at T = 300 and order 0 the limit is 183 channels."""
    assert long_ws(2, 2, 300, 300, 183, 0)[0] == 0
    assert long_ws(2, 2, 300, 300, 183, 0, want_grad=0)[0] == 0
    for want_grad in (0, 1):
        rc, _ = long_ws(2, 2, 300, 300, 184, 0, want_grad=want_grad)
        assert rc == UNSUPPORTED
        assert "LDS" in _lib.last_error()
    assert long_plan(2, 2, 300, 300, 183, 0) is not None and long_plan(2, 2, 300, 300, 184, 0) is None
    for d in (16, 17, 33):  # (what SigKernel(RBFKernel) sends to the long route)
        assert ops.gram_takes(4, 4, 300, d, 0) is False
        assert long_ws(4, 4, 300, 300, d, 0)[0] == 0


@pytest.mark.parametrize("n", [7, 8, 9, 10])
def test_high_orders(n):
    """Orders 7 to 10 (nrow = 1: a band of 64 rows is part of one coarse row): taken up to P = Q = 8192, refused past it."""
    edge = 8192 // (1 << n) + 1  # points giving 8192 cells
    for (TX, TY) in [(edge, edge), (edge, 3), (3, edge), (2, 2)]:
        for want_grad in (0, 1):
            assert long_ws(1, 2, TX, TY, 2, n, want_grad=want_grad)[0] == 0, _lib.last_error()
        assert long_plan(1, 2, TX, TY, 2, n)["nrow"] == 1
    for (TX, TY) in [(edge + 1, edge), (edge, edge + 1), (edge + 1, 2)]:
        rc, _ = long_ws(1, 2, TX, TY, 2, n)
        assert rc == UNSUPPORTED and "8192" in _lib.last_error()
