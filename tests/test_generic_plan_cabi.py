"""Host-side pin of `plans.generic_plan` and `plans.generic_route`, the restated launch plan of the coverage kernel
(csrc/gram_generic.hip) and of `gram_route`'s three ways into it, to the library's own workspace query; no device needed.

A gradient query's bytes are [256: work counter][A * nchunks slabs of T * d doubles][the column slab of an unordered
solve][grid * wsk_per_block floats] + 256: they fix JC and nchunks, the bands and steps, the doubling of the scratch in the
per-band layout and the column slab; at sizes with more items than workgroups grid = CUs * per_cu also fixes the LDS figure and
with it the increment table.  Queries are ordered with A != B, or Y_IS_X, so that they cover one plan."""
import ctypes

import pytest

from cabi import OK, UNSUPPORTED, lib
from plans import device_cus, generic_plan, generic_route
from sigsvgd_amd import _lib

RBF, LINEAR = _lib.STATIC_RBF, _lib.STATIC_LINEAR
NAIVE, Y_IS_X, FORCE = _lib.FLAG_NAIVE_SOLVER, _lib.FLAG_Y_IS_X, _lib.FLAG_FORCE_GENERIC


def query(A, B, T, d, n, kind, want_grad, flags):
    """(status, bytes) of sigsvgd_gram_workspace_bytes"""
    b = ctypes.c_size_t(0)
    rc = lib().sigsvgd_gram_workspace_bytes(A, B, T, d, n, kind, int(want_grad), flags, ctypes.byref(b))
    return rc, b.value


def restated(A, B, T, d, n, kind, want_grad, flags, cus):
    """(route, plan) of the same query"""
    sym = bool(flags & Y_IS_X) and A == B
    r = generic_route(A, B, T, d, n, kind, want_grad, bool(flags & NAIVE), bool(flags & FORCE), sym, cus)
    assert r is not None, (A, B, T, d, n, kind, flags)
    return r[0], generic_plan(A, B, T, d, n, want_grad, sym, r[1], r[2], cus)


# (T, d, n): both sides of the table switches, one band and several, T = 2, channel blocks, refined grids past the band kernels
SHAPES = [(5, 2, 0), (5, 2, 2), (33, 2, 0), (34, 2, 0), (47, 2, 0), (98, 2, 0), (99, 2, 0), (105, 2, 1), (113, 2, 0), (114, 2, 0),
          (276, 2, 0), (128, 14, 0), (89, 16, 0), (90, 16, 0), (2, 1, 0), (2, 2, 7), (3, 2, 7), (33, 17, 0), (9, 33, 1), (40, 3, 3),
          (65, 3, 0), (20, 7, 4)]
# ordered, A != B: one item, fewer items than workgroups, JC = 2, 8, 32 and items past the grid
SIZES = [(1, 2), (3, 2), (20, 21), (64, 65), (256, 70), (300, 8), (1024, 70), (2500, 7)]


def test_plan_matches_workspace_query_on_every_route():
    cus = device_cus()
    seen, past_grid = set(), 0
    for (kind, flags) in [(RBF, FORCE), (LINEAR, 0), (RBF, NAIVE), (LINEAR, FORCE | NAIVE)]:
        for (T, d, n) in SHAPES:
            for (A, B) in SIZES:
                route, pl = restated(A, B, T, d, n, kind, True, flags, cus)
                rc, b = query(A, B, T, d, n, kind, True, flags)
                assert route == ("GenericPrecise" if flags & FORCE else "Generic")
                assert (rc, b) == ((OK, pl["bytes"]) if pl else (UNSUPPORTED, 0)), (kind, flags, A, B, T, d, n, rc, b, pl)
                if pl:
                    seen.add((route, pl["table"], pl["JC"]))
                    past_grid += pl["items"] > pl["grid"]
                    # forward only: no slabs, no scratch
                    _, pf = restated(A, B, T, d, n, kind, False, flags, cus)
                    assert query(A, B, T, d, n, kind, False, flags) == ((OK, 512) if pf else (UNSUPPORTED, 0))
    assert {(r, t, jc) for r in ("Generic", "GenericPrecise") for t in ("f64", "f32", "big") for jc in (1, 2, 8, 32)} <= seen
    assert past_grid > 100
    # the fp32-sweep kinds fall through to the default route where no family holds the shape
    for (T, d, n) in [(40, 3, 3), (2, 2, 0), (2, 2, 5), (9, 17, 1), (200, 3, 0), (33, 17, 0)]:
        route, pl = restated(300, 8, T, d, n, RBF, True, 0, cus)
        assert route == "Generic" and query(300, 8, T, d, n, RBF, True, 0) == (OK, pl["bytes"]), (T, d, n)
    assert generic_route(300, 8, 20, 3, 0, RBF, True) is None and generic_route(300, 8, 100, 3, 0, RBF, True) is None
    assert generic_route(300, 8, 20, 3, 0, _lib.STATIC_IMQ, True)[0] == "GenericPrecise"
    assert generic_route(300, 8, 20, 3, 0, _lib.STATIC_MATERN52, False)[0] == "GenericPrecise"


def test_one_channel_route_solves_unordered_at_any_size():
    """d = 1, order 0, gradient, 3 <= T <= 128: precise, and with Y_IS_X each unordered pair once whatever the pair count --
    the column slab [N][N][T] doubles is in the bytes from N = 2 on.  (T = 2 and T = 129 are not one-channel launches.)"""
    cus = device_cus()
    for T in (3, 5, 64, 100, 128):
        for (A, B) in SIZES:
            route, pl = restated(A, B, T, 1, 0, RBF, True, 0, cus)
            assert route == "GenericOneChannel" and not pl["yx"] and pl["table"] in ("f64", "big")
            assert query(A, B, T, 1, 0, RBF, True, 0) == (OK, pl["bytes"]), (A, B, T)
        for N in (2, 5, 63, 64, 300):
            route, pl = restated(N, N, T, 1, 0, RBF, True, Y_IS_X, cus)
            ordered = generic_plan(N, N, T, 1, 0, True, False, True, True, cus)
            assert route == "GenericOneChannel" and pl["yx"] and pl["bytes"] > ordered["bytes"]
            # (a Y_IS_X gradient query also covers the symmetric partial solve of the shape, which keeps the fp32-sweep
            #  kernels: from T = 65 on the quadrant kernel's fixed scratch is the larger plan up to a few hundred paths)
            rc, b = query(N, N, T, 1, 0, RBF, True, Y_IS_X)
            assert rc == OK and b >= pl["bytes"] and (b == pl["bytes"] or T > 64), (N, T, b, pl)
        N = 600
        assert query(N, N, T, 1, 0, RBF, True, Y_IS_X) == (OK, restated(N, N, T, 1, 0, RBF, True, Y_IS_X, cus)[1]["bytes"]), T
    assert generic_route(5, 5, 2, 1, 0, RBF, True, sym=True)[0] == "Generic"
    assert generic_route(5, 5, 129, 1, 0, RBF, True, sym=True)[0] == "Generic"
    assert generic_route(5, 5, 20, 1, 0, RBF, False, sym=True) is None  # forward only: the fp32 route


def test_unordered_solve_thresholds():
    """Y is X on the other two routes: ordered pairs below 4096 of them (N = 63), each unordered pair once from N = 64 on,
    and ordered again where the column slab N * N * T * d doubles would pass 1 GiB.  Queries only: nothing runs at these sizes."""
    cus = device_cus()
    for (kind, flags) in [(RBF, FORCE | Y_IS_X), (LINEAR, Y_IS_X)]:
        for (N, T, d, n, yx) in [(63, 5, 2, 0, False), (64, 5, 2, 0, True), (63, 5, 2, 2, False), (64, 5, 2, 2, True), (190, 5, 2, 0, True),
                                 (3663, 5, 2, 0, True), (3664, 5, 2, 0, False), (1024, 128, 1, 0, True), (1025, 128, 1, 0, False)]:
            _, pl = restated(N, N, T, d, n, kind, True, flags, cus)
            assert pl["yx"] == yx, (N, T, d, pl)
            assert query(N, N, T, d, n, kind, True, flags) == (OK, pl["bytes"]), (N, T, d, n, pl)
            if yx:  # forward only: unordered too (no slab to outgrow)
                assert generic_plan(N, N, T, d, n, False, True, bool(flags & FORCE), False, cus)["yx"]
    assert 3664 * 3664 * 5 * 2 * 8 > 1 << 30 >= 3663 * 3663 * 5 * 2 * 8 and 1025 * 1025 * 128 * 8 > 1 << 30 == 1024 * 1024 * 128 * 8
    assert generic_plan(190, 190, 5, 2, 0, True, True, True, False, cus)["JC"] == 2
    assert generic_plan(181, 181, 5, 2, 0, True, True, True, False, cus)["JC"] == 2  # (Y is X: 181 * 91 >= 16384 items)
    assert generic_plan(180, 180, 5, 2, 0, True, True, True, False, cus)["JC"] == 1
    assert generic_plan(64, 32, 5, 2, 0, True, False, True, False, cus)["JC"] == 1   # (ordered: A * ceil(B / 2) >= 2048)
    assert generic_plan(64, 63, 5, 2, 0, True, False, True, False, cus)["JC"] == 2


# route flags, kind, d, gradient, order, (T, table) at T = 2 and at every switch, first refused T (A = B + 1 = 3)
REFUSALS = [
    (FORCE, RBF, 2, True, 0, [(2, "f64"), (99, "big")], 277),
    (FORCE, RBF, 2, True, 1, [(2, "f64"), (99, "f32")], 114),
    (FORCE, RBF, 2, False, 0, [(2, "f64"), (139, "big")], 277),
    (FORCE, RBF, 2, False, 1, [(2, "f64"), (139, "f32")], 193),
    (FORCE, RBF, 16, True, 0, [(2, "f64"), (90, "big")], 201),
    (0, LINEAR, 2, True, 0, [(2, "f64"), (34, "f32"), (114, "big")], 277),
    (0, LINEAR, 2, False, 0, [(2, "f64"), (47, "f32"), (195, "big")], 277),
    (NAIVE, RBF, 2, True, 1, [(2, "f64"), (33, "f32")], 114),
]


@pytest.mark.parametrize("flags,kind,d,want_grad,n,switches,refused_from", REFUSALS)
def test_table_switches_and_the_lds_refusal(flags, kind, d, want_grad, n, switches, refused_from):
    """The increment table at every T up to past the refusal: the restated plan changes table exactly where the rows say, the
    library refuses (E_UNSUPPORTED, no bytes) from `refused_from` on and accepts the T before it, and where both accept
    the bytes agree -- at 2500 x 7, past the grid, where they carry the LDS figure."""
    cus = device_cus()
    found, prev = [], None
    for T in range(2, refused_from + 3):
        _, pl = restated(2500, 7, T, d, n, kind, want_grad, flags, cus)
        rc, b = query(2500, 7, T, d, n, kind, want_grad, flags)
        assert (pl is None) == (T >= refused_from) and rc == (UNSUPPORTED if T >= refused_from else OK), (T, rc, pl)
        if pl:
            assert b == pl["bytes"], (T, b, pl)
            if pl["table"] != prev:
                found.append((T, pl["table"]))
                prev = pl["table"]
    assert found == switches
