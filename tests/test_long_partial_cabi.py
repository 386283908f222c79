"""Host-side checks of the long route's partial solve (`sigsvgd_gram_long_partial_plan`,
`sigsvgd_gram_long_partial_workspace_bytes`, `sigsvgd_gram_long_sym_partial`, include/sigsvgd_hip.h):
exports, argument checks, the Python mirror of the item rule (tests/plans.py) pinned to the two queries, and the four
conditions the plan has to meet (partition, balance, schedule, memory).  No device needed: every call below returns before
any device work."""
import ctypes
import re

import pytest

from cabi import assert_exported, BADARG, FAKE, lib, UNSUPPORTED, WORKSPACE
from plans import device_cus, item_pairs, item_size, part_items, part_pick, part_plan, part_share, ring_plan, tiles
from sigsvgd_amd import _lib, ops

NAMES = ("sigsvgd_gram_long_partial_plan", "sigsvgd_gram_long_partial_workspace_bytes", "sigsvgd_gram_long_sym_partial")
GRID_N, GRID_G, GRID_RES = (64, 128, 200, 256, 512, 1024), (2, 4, 8), (256, 512, 1024, 2048)


# ---- the library's own answers (the Python mirror of the plan is plans.part_plan) ---------------------------------------
def q_plan(N, T, d, n=0, kind=_lib.STATIC_RBF, flags=0, stride=1, out=True):
    R, JC = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = lib().sigsvgd_gram_long_partial_plan(N, T, d, n, kind, flags, stride, ctypes.byref(R) if out else None,
                                              ctypes.byref(JC) if out else None)
    return rc, R.value, JC.value


def q_ws(N, T, d, n=0, kind=_lib.STATIC_RBF, flags=0, off=0, stride=1, out=True):
    b = ctypes.c_size_t(12345)
    rc = lib().sigsvgd_gram_long_partial_workspace_bytes(N, T, d, n, kind, flags, off, stride, ctypes.byref(b) if out else None)
    return rc, b.value


def _launch(a, X=FAKE, K=FAKE, g=FAKE, dtype=_lib.F32, inv_h=1.0, ws_bytes=1 << 40):
    return lib().sigsvgd_gram_long_sym_partial(X, a["N"], a["T"], a["d"], dtype, inv_h, a["n"], a["kind"], a["flags"], a["off"],
                                               a["stride"], None, K, g, FAKE, ws_bytes, None)


# ---- exports and argument checks ----------------------------------------------------------------------------------------
def test_symbols_exported_and_declared():
    import os

    assert_exported(NAMES, abi=10)
    header = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "..", "include", "sigsvgd_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header)


@pytest.mark.parametrize("case", ["N<1", "T<2", "d<1", "kind", "order", "force_generic", "unknown_flag", "stride<1", "off<0",
                                  "off>=stride"])
def test_bad_shapes_flags_and_tiles(case):
    args = dict(N=6, T=300, d=2, n=0, kind=_lib.STATIC_RBF, flags=_lib.FLAG_FOLD_TILES, off=1, stride=2)
    upd = {"N<1": dict(N=0), "T<2": dict(T=1), "d<1": dict(d=0), "kind": dict(kind=5), "order": dict(n=11),
           "force_generic": dict(flags=_lib.FLAG_FORCE_GENERIC), "unknown_flag": dict(flags=_lib.FLAG_WS_CLEAN),
           "stride<1": dict(stride=0, off=0), "off<0": dict(off=-1), "off>=stride": dict(off=2)}[case]
    a = {**args, **upd}
    if not case.startswith("off"):  # (the plan query has no tile_offset)
        assert q_plan(a["N"], a["T"], a["d"], a["n"], a["kind"], a["flags"], a["stride"])[0] == BADARG, _lib.last_error()
        assert _lib.last_error()
    assert q_ws(a["N"], a["T"], a["d"], a["n"], a["kind"], a["flags"], a["off"], a["stride"])[0] == BADARG
    assert _lib.last_error()
    assert _launch(a) == BADARG and _lib.last_error()


def test_launch_argument_checks():
    a = dict(N=6, T=300, d=2, n=0, kind=_lib.STATIC_RBF, flags=0, off=0, stride=2)
    assert q_plan(6, 300, 2, out=False)[0] == BADARG and q_ws(6, 300, 2, out=False)[0] == BADARG
    assert _launch(a, X=None) == BADARG and _launch(a, K=None) == BADARG and _launch(a, g=None) == BADARG
    assert _launch(a, dtype=7) == BADARG
    assert _launch(a, inv_h=0.0) == BADARG  # RBF without a bandwidth
    for f in (0, _lib.FLAG_NAIVE_SOLVER, _lib.FLAG_SYM, _lib.FLAG_Y_IS_X, _lib.FLAG_FOLD_TILES,
              _lib.FLAG_FOLD_TILES | _lib.FLAG_SYM | _lib.FLAG_NAIVE_SOLVER | _lib.FLAG_Y_IS_X):
        assert q_ws(6, 300, 2, flags=f, off=1, stride=2)[0] == 0, _lib.last_error()
        assert q_plan(6, 300, 2, flags=f, stride=2)[0] == 0, _lib.last_error()
    # the two-sided entry point still refuses the fold flag
    b = ctypes.c_size_t(0)
    assert lib().sigsvgd_gram_long2_workspace_bytes(3, 3, 300, 300, 2, 0, 0, 1, 0, _lib.FLAG_FOLD_TILES | _lib.FLAG_Y_IS_X,
                                                    ctypes.byref(b)) == BADARG


def test_workspace_too_small_is_refused_before_device_work():
    a = dict(N=6, T=300, d=2, n=0, kind=_lib.STATIC_RBF, flags=_lib.FLAG_FOLD_TILES, off=0, stride=2)
    rc, need = q_ws(6, 300, 2, flags=a["flags"], off=0, stride=2)
    assert rc == 0 and need > 0
    assert _launch(a, ws_bytes=need - 1) == WORKSPACE
    assert "required %d" % need in _lib.last_error()


def test_refusals_are_the_long_routes():
    assert q_plan(4, 129, 2, n=6)[0] == 0  # P = Q = 8192: the edge is taken
    for (T, n) in [(8194, 0), (130, 6)]:
        assert q_plan(4, T, 2, n=n)[0] == UNSUPPORTED and "8192" in _lib.last_error()
        assert q_ws(4, T, 2, n=n)[0] == UNSUPPORTED and "8192" in _lib.last_error()
    assert q_plan(4, 300, 184)[0] == UNSUPPORTED and "LDS" in _lib.last_error()
    assert ops.gram_long_partial_takes(4, 300, 183) is True
    assert ops.gram_long_partial_takes(4, 300, 184) is False
    assert ops.gram_long_partial_takes(4, 8194, 2, tile_stride=4) is False
    with pytest.raises(RuntimeError):  # a bad argument is an error, not a route
        ops.gram_long_partial_takes(4, 300, 2, static_kind=9)
    assert ops.gram_long_partial_tiles(6, 300, 2, 0, _lib.STATIC_RBF, 2) == q_plan(6, 300, 2, stride=2)[1:]


def test_a_rank_without_tiles_is_a_valid_launch_without_workspace():
    R, _ = ops.gram_long_partial_tiles(5, 300, 2, 0, _lib.STATIC_RBF, 8)
    assert R == 1
    for fold in (0, _lib.FLAG_FOLD_TILES):
        sizes = [q_ws(5, 300, 2, flags=fold, off=off, stride=8) for off in range(8)]
        assert all(rc == 0 for rc, _ in sizes)
        for off in range(8):
            assert (sizes[off][1] == 0) == (not ops.owned_tiles(5, off, 8, bool(fold)))


# ---- the mirror is the library's rule -------------------------------------------------------------------------------------
def test_plan_mirror_matches_the_queries():
    """`plans.part_plan` against sigsvgd_gram_long_partial_plan and ..._workspace_bytes: shapes with 1, 2, 4 and 8 resident
    waves per CU, orders 0 and 2, d = 3 and 20, strides 1 .. 8 and more ranks than tiles, folded and cyclic, and refusals."""
    cus = device_cus()
    shapes = [(20, 300, 0), (33, 200, 2), (9, 257, 0), (5, 300, 0), (70, 140, 0), (64, 300, 0), (128, 300, 0), (256, 130, 0),
              (300, 16, 0), (200, 40, 2), (256, 1025, 0), (131, 2, 0), (1, 300, 0), (2, 9, 2), (512, 64, 0), (16, 2049, 0),
              (4, 8193, 0), (4, 8194, 0), (4, 2050, 2)]
    seen, res_seen = set(), set()
    for (N, T, n) in shapes:
        for d in (3, 20, 184):
            for stride in (1, 2, 3, 4, 8):
                rc, R, JC = q_plan(N, T, d, n, stride=stride)
                ref = part_plan(N, T, d, n, 0, stride, True, cus)
                assert (rc == UNSUPPORTED) == (ref is None), (N, T, d, n, stride, rc)
                if ref is None:
                    assert q_ws(N, T, d, n, off=0, stride=stride)[0] == UNSUPPORTED
                    continue
                assert rc == 0 and (R, JC) == (ref["R"], ref["JC"]), (N, T, d, n, stride, R, JC, ref["R"], ref["JC"])
                seen.add((R, JC))
                res_seen.add(ref["resident"] // cus)
                for fold in (False, True):
                    for off in range(stride):
                        pl = part_plan(N, T, d, n, off, stride, fold, cus)
                        rc, b = q_ws(N, T, d, n, flags=_lib.FLAG_FOLD_TILES if fold else 0, off=off, stride=stride)
                        assert rc == 0 and b == pl["bytes"], (N, T, d, n, stride, off, fold, b, pl["bytes"])
    assert {1, 2, 4, 8} <= res_seen, res_seen
    assert (1, 1) in seen and any(JC & (JC - 1) for (_, JC) in seen) and any(R > 1 and JC != R for (R, JC) in seen), seen
    assert q_plan(4, 8193, 3)[0] == 0 and q_plan(4, 8194, 3)[0] == UNSUPPORTED  # T = 8193 at order 0 is the edge
    # the fp32 and fp64 launches share one plan: the queries take no dtype


# ---- the four plan conditions ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [True, False])
def test_condition_partition(fold):
    """Every unordered pair belongs to exactly one rank's items, enumerated by the mirror of the kernel's item decode."""
    for N in (1, 2, 7, 33, 64, 131, 256):
        for stride in (1, 2, 3, 4, 8):
            for res in (256, 2048):
                R, JC = part_pick(N, stride, res)
                seen = {}
                for off in range(stride):
                    owned = ops.owned_tiles(tiles(N, R), off, stride, fold)
                    items = part_items(N, R, JC, owned)
                    assert len(set(items)) == len(items)
                    for (k, c) in items:
                        assert 0 <= c < tiles(N - owned[k] * R, JC)
                        assert item_size(N, R, JC, owned[k], c) == len(item_pairs(N, R, JC, owned[k], c))
                        for p in item_pairs(N, R, JC, owned[k], c):
                            assert p not in seen, (N, stride, res, p, seen[p], off)
                            seen[p] = off
                assert len(seen) == N * (N + 1) // 2 and all(i <= j for (i, j) in seen), (N, stride, res, R, JC)


def _grid():
    for res in GRID_RES:
        for N in GRID_N:
            for G in GRID_G:
                R, JC = part_pick(N, G, res)
                yield res, N, G, R, JC, [part_share(N, R, JC, off, G, True, res) for off in range(G)]


def test_conditions_balance_schedule_memory():
    """Folded ownership over N x G x resident waves (72 combinations): the fullest rank holds <= 1.05 x the mean; every
    rank's eff = ceil(pairs / resident) / makespan >= 0.9 in the kernel's own item order; a share's slabs are <= N^2 / 4
    (units of T d doubles) where it holds more than 16 pairs per resident wave, else <= 2 pairs + N; and per rank the slabs
    at 8 ranks are fewer than at 2 for N >= 256."""
    slabs = {}
    for res, N, G, R, JC, shares in _grid():
        total = N * (N + 1) // 2
        assert sum(s["pairs"] for s in shares) == total
        assert max(s["pairs"] for s in shares) * G <= 1.05 * total, (res, N, G, R, JC)
        for s in shares:
            eff = -(-s["pairs"] // res) / s["makespan"]
            assert eff >= 0.9, (res, N, G, R, JC, eff)
            bound = N * N // 4 if s["pairs"] > 16 * res else 2 * s["pairs"] + N
            assert s["slabs"] <= bound, (res, N, G, R, JC, s["slabs"], bound)
        slabs[(res, N, G)] = max(s["slabs"] for s in shares)
    for res in GRID_RES:
        for N in GRID_N:
            if N >= 256:
                assert slabs[(res, N, 8)] < slabs[(res, N, 2)], (res, N)


def test_the_grid_of_the_conditions_is_the_librarys_plan():
    """The (R, JC) the conditions above were checked on are the library's: its plan query at every N and rank count of the
    grid, on shapes that leave a CU 1, 2, 4 and 8 resident waves (256 CUs: the grid's 256 .. 2048)."""
    cus = device_cus()
    for (T, d, per_cu) in [(2049, 2, 1), (300, 4, 2), (60, 3, 4), (30, 3, 8)]:
        res = ring_plan(T, T, 0, True, d, cus)["resident"]
        assert res == per_cu * cus
        for N in GRID_N:
            for G in GRID_G:
                assert q_plan(N, T, d, stride=G) == (0,) + part_pick(N, G, res), (N, G, T, d)


def test_workspace_falls_with_the_rank_count():
    """The library's own bytes (T = 300, d = 4: two resident waves per CU): a share's workspace at 8 ranks is smaller than
    at 2 for each N >= 256."""
    for N in (256, 512, 1024):
        by = {G: max(q_ws(N, 300, 4, flags=_lib.FLAG_FOLD_TILES, off=off, stride=G)[1] for off in range(G)) for G in (2, 8)}
        assert 0 < by[8] < by[2], (N, by)
