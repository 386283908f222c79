"""Host-side checks behind tests/test_gpu_partition.py; no device needed.  `plans.gram_geometry` restates how a Gram launch
of the fp32-sweep kernels is split into items and workgroups: pinned here to the library's own queries.  Every case of the
partition file's matrix is in the multi-item regime it claims on 256 compute units.  And, on the fp64 oracle alone, the
gradient metric of that file (largest error over the launch's largest entry, below 1e-5) would notice a single lost or
misfiled pair."""
import ctypes

import numpy as np
import pytest

from cabi import lib
from oracle import c_oracle as C
from parity import signed_weights, walks
from plans import (claim_regime, device_cus, gram_geometry, gram_item_ranges, gram_multi_item_regime,
                   gram_ordered_grad_bytes, PARTITION_CASES, probes, set_band_mode, step_scale)
from sigsvgd_amd import _lib

MODES = (None, "serial", "parallel")


def test_rows_per_tile_match_sym_tile_rows():
    """the ownership unit of the partial solve is the tile height of the symmetric gradient launch (order 0, T <= 128)"""
    for T in range(3, 129):
        for d in range(2, 17):
            g = gram_geometry(37, 37, T, d, 0, True, True, device_cus())
            assert lib().sigsvgd_gram_sym_tile_rows(T, d) == g["rows_per_tile"], (T, d, g)


def test_geometry_matches_workspace_query(monkeypatch):
    """Ordered gradient queries with A != B reach one launch, whose plan is [flag bytes][row segments of (tiles + grid)
    workgroup-tile meetings][the family's scratch]: the bytes fix rows_per_tile and grid, and the family through its scratch.
    Shapes of every family, both band schedules and the launcher's own rule, from one item to far past the resident grid."""
    cus = device_cus()
    shapes = [(c.T, c.d, c.n) for c in PARTITION_CASES]
    shapes += [(3, 2, 0), (32, 8, 0), (33, 8, 0), (64, 4, 0), (64, 5, 0), (64, 9, 0), (65, 2, 0), (112, 15, 0), (113, 14, 0),
               (128, 16, 0), (3, 7, 6), (33, 5, 2), (9, 3, 3), (17, 14, 2), (33, 3, 3), (3, 2, 7), (5, 16, 6), (27, 2, 3), (17, 9, 4)]
    sizes = [(1, 2), (2, 1), (5, 9), (9, 113), (33, 77), (43, 97), (67, 263), (300, 8), (8, 300), (301, 517)]
    families = set()
    for mode in MODES:
        set_band_mode(monkeypatch, mode)
        for (T, d, n) in shapes:
            for (A, B) in sizes:
                g = gram_geometry(A, B, T, d, n, True, False, cus)
                assert g is not None and g["grid"] == min(g["items"], g["resident"])
                b = ctypes.c_size_t(0)
                assert lib().sigsvgd_gram_workspace_bytes(A, B, T, d, n, _lib.STATIC_RBF, 1, 0, ctypes.byref(b)) == 0
                assert b.value == gram_ordered_grad_bytes(A, B, T, d, n, cus), (mode, A, B, T, d, n, g, b.value)
                families.add((g["family"], g["rows_per_tile"]))
    assert {("fast", 4), ("fast", 8), ("quad", 8), ("dyad", 4), ("dyad", 8), ("band serial", 8), ("band parallel", 1)} <= families


def test_one_channel_gradients_leave_the_families():
    assert gram_geometry(9, 9, 20, 1, 0, True, True) is None
    assert gram_geometry(9, 9, 20, 1, 0, False, True)["family"] == "fast"
    assert gram_geometry(9, 9, 40, 3, 3, True, False) is None  # 312 cells: the coverage kernel


def test_item_ranges():
    """the split by hand: 3 tiles of 8 rows over 20 columns, ordered and from the diagonal on"""
    g = dict(rows_per_tile=8, items=60, grid=7)
    bounds, starts = gram_item_ranges(20, 20, g, False)
    assert list(starts) == [0, 20, 40, 60] and list(bounds) == [0, 8, 17, 25, 34, 42, 51, 60]
    assert gram_multi_item_regime(20, 20, g, False) == dict(multi=True, inside=True, crosses=True, shared=True)
    g = dict(rows_per_tile=8, items=36, grid=3)
    bounds, starts = gram_item_ranges(20, 20, g, True)
    assert list(starts) == [0, 20, 32, 36] and list(bounds) == [0, 12, 24, 36]
    assert gram_multi_item_regime(20, 20, g, True) == dict(multi=True, inside=True, crosses=True, shared=True)
    # one item per workgroup: no range holds a second item, let alone a tile boundary; ranges that are whole tiles
    assert gram_multi_item_regime(20, 20, dict(rows_per_tile=8, items=60, grid=60), False) == dict(
        multi=False, inside=True, crosses=False, shared=True)
    assert gram_multi_item_regime(20, 20, dict(rows_per_tile=8, items=60, grid=3), False) == dict(
        multi=True, inside=False, crosses=False, shared=False)


def test_partition_cases_are_in_their_regime(monkeypatch):
    """every case of tests/test_gpu_partition.py on 256 compute units: the family and tile height the table names, and the
    regime conditions of the gradient and of the forward-only launch, ordered and Y is X (the GPU tests assert the same with
    the device's CU count)"""
    seen = set()
    for c in PARTITION_CASES:
        set_band_mode(monkeypatch, c.mode)
        for (A, B, sym) in [(*c.AB, False), (c.N, c.N, True)]:
            g = claim_regime(A, B, c.T, c.d, c.n, True, sym, c.regime, cus=256)
            assert (g["family"], g["rows_per_tile"]) == (c.family, c.rows), (c, g)
            if c.rows > 1 and not (sym and c.regime == "two"):  # (N = 44 is the one Y-is-X size of 4-row tiles past the grid)
                assert A % c.rows and B % c.rows, "sizes ragged against the tile height"
            gf = gram_geometry(A, B, c.T, c.d, c.n, False, sym, 256)
            same = (gf["rows_per_tile"], gf["grid"]) == (g["rows_per_tile"], g["grid"])
            assert same == (c.ABf is None), (c, g, gf)
            seen.add((g["family"], g["rows_per_tile"], g["resident"]))
        if c.ABf:
            for (A, B, sym) in [(*c.ABf, False), (c.Nf, c.Nf, True)]:
                gf = claim_regime(A, B, c.T, c.d, c.n, False, sym, c.regime, cus=256)
                seen.add((gf["family"] + " forward", gf["rows_per_tile"], gf["resident"]))
    set_band_mode(monkeypatch, None)
    claim_regime(67, 263, 16, 3, 0, True, False, "full", cus=256)
    claim_regime(257, 257, 12, 2, 0, True, True, "full", cus=256)
    assert {("fast", 8, 768), ("fast", 8, 256), ("fast", 4, 256), ("fast forward", 4, 768), ("fast forward", 4, 512),
            ("quad", 8, 256), ("dyad", 8, 256), ("dyad", 4, 256), ("band serial", 8, 512), ("band serial", 8, 256),
            ("band parallel", 1, 1280), ("band parallel", 1, 1024)} <= seen, seen
    # the 4-row tiles of gram_dyad.hip exist up to 4 * CUs pairs: with two tiles or more such a launch never reaches
    # 2 * grid + 1 items, and none of its two-item ranges holds a tile boundary -- regime "two" claims the rest
    monkeypatch.setenv("SIGSVGD_BAND_MODE", "serial")
    past_grid = 0
    for A in range(5, 300):
        for (B, sym) in [(B, False) for B in range(1, 1024 // A + 2)] + [(A, True)]:
            g = gram_geometry(A, B, 20, 7, 2, True, sym, 256)
            if g["rows_per_tile"] == 4 and g["items"] > g["grid"]:
                past_grid += 1
                assert g["items"] < 2 * g["grid"] + 1 and not gram_multi_item_regime(A, B, g, sym)["crosses"], (A, B, sym, g)
    assert past_grid > 100


# one small case per launch form of the partition file: (form, T, d, size): the ordered launch and the three weightings
# of the Y-is-X launch
FORMS = [("ordered", 16, 3, (67, 263)), ("signed", 16, 3, 155), ("signed-sym", 64, 7, 93), ("ones", 33, 9, 67)]


@pytest.mark.parametrize("form,T,d,size", FORMS, ids=[f[0] for f in FORMS])
def test_gradient_metric_notices_one_pair(form, T, d, size):
    """Losing pair (i, j) -- w_ij = 0 in the oracle -- moves row i of the reference gradient by more than 1e-4 of the
    launch's largest entry, ten times the tolerance of the parity tests, for 32 pairs at the ends of workgroup ranges and at
    random; so does filing a pair under its mirror image's weight (w_ij and w_ji swapped: asymmetric weights), and losing
    the column side of a symmetric item (pair (j, i) of row j).  No row hides behind the launch's maximum: every row's
    largest entry is at least 1e-2 of it.  Seeds, shapes and weights are those of tests/test_gpu_partition.py."""
    sym = form != "ordered"
    (A, B), h = ((size, size), 1.1) if sym else (size, 0.9)
    X = walks(A, T, d, 21 if sym else 11, step_scale(0))
    Y = X if sym else walks(B, T, d, 12, step_scale(0))
    w = np.ones((A, B)) if form == "ones" else signed_weights(A, B, 23 if sym else 13)

    def effective(w):
        return w + w.T if form == "signed-sym" else w

    _, gref = C.gram_fwd_bwd(X, Y, h, 0, grad_out=effective(w))
    top = np.abs(gref).max()
    row_top = np.abs(gref).reshape(A, -1).max(axis=1)
    print(f"{form}: smallest row maximum {row_top.min() / top:.3f} of the launch's")
    assert row_top.min() >= 1e-2 * top

    def row(i, w2):
        return C.gram_fwd_bwd(X, Y, h, 0, grad_out=effective(w2)[i:i + 1], rows=(i, i + 1))[1][0]

    geom = gram_geometry(A, B, T, d, 0, True, sym, 256)
    assert all(gram_multi_item_regime(A, B, geom, sym).values())
    pairs = probes(A, B, geom, sym, 5)
    assert len(pairs) == 32
    least = np.inf
    for (i, j) in pairs:
        assert np.abs(row(i, w) - gref[i]).max() <= 1e-12 * top  # (the row query is the full run's row)
        lost = w.copy()
        lost[i, j] = 0.0
        moves = [np.abs(row(i, lost) - gref[i]).max()]
        if sym and i != j:
            lost = w.copy()
            lost[j, i] = 0.0
            moves.append(np.abs(row(j, lost) - gref[j]).max())  # the column side of item (tile of i, column j)
        if form == "signed" and i != j:
            swapped = w.copy()
            swapped[i, j], swapped[j, i] = w[j, i], w[i, j]
            moves.append(np.abs(row(i, swapped) - gref[i]).max())
        least = min(least, min(moves))
        assert min(moves) > 1e-4 * top, (form, i, j, [m / top for m in moves])
    print(f"{form}: a lost or misfiled pair moves its row by at least {least / top:.2e} of the launch's largest entry")
