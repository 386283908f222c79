"""The checker of the vector kernels, checked on the CPU (tests/vec_reference.py; the device tests are
tests/test_gpu_vec_edges.py).

`fused_order` and `kgrad_order` restate the kernels' arithmetic in fp32 numpy.  They pass `assert_vec` in both input forms at
every shape the device file runs (the two 4097-row shapes on their first two and last two row tiles, with the split geometry
of the whole launch), and each of the nine fused and four two-launch mistakes fails it in both forms at every shape tried where
the mistake can happen.  That rests on the integer form's exactness (the 2^24 condition, asserted) and the float form's margin
(asserted: the smallest channel term, 0.25, is worth at least 2 sq bounds at every shape; 3.6 fused and 5.9 direct at D = 512,
above 50 at D <= 129).  The restatements' own largest error / bound is 0.34.
With an `assert_vec` that always passes, 27 of the tests here fail: the 26 mutation tests and the hand-computed gate (tried
once)."""
import ctypes

import numpy as np
import pytest

import vec_reference as V
from oracle import vector_oracle as VO
from vec_reference import SEED, U32

FUSED_SHAPES = V.FUSED_D_SHAPES + V.FUSED_AB_SHAPES + V.FUSED_BIG_SHAPES + V.FUSED_GUARDED_SHAPES + V.FUSED_ALIGN_SHAPES
# the shapes the mutation tests walk: every D edge, the tile edges in B, and the launches with several tiles per workgroup
MUTATION_SHAPES = [(65, 70, D) for D in (1, 3, 33, 64, 65, 129, 257, 512)] + [(17, 65, 5), (64, 65, 68), (129, 193, 68), (1, 63, 5)] + V.FUSED_BIG_SHAPES


def capped(inp):
    """at most the first two and the last two row tiles of a launch"""
    if inp.A <= 4 * V.FM:
        return inp
    return inp.take_rows(np.r_[0:2 * V.FM, inp.A - V.FM - 1:inp.A])


def check_fused(inp, kind, K, dK, where, path="fused"):
    e = V.expected(inp, kind, path)
    per = V.fused_geometry(inp.launch_A, inp.B)["per"]
    worst = V.assert_vec(K, e.K, e.e_K, where, "K", per)
    return max(worst, V.assert_vec(dK, e.dK, e.e_dK, where, "dK"))


_INPUTS = {}


def inputs(A, B, D, form, metric):
    key = (A, B, D, form, metric)
    if key not in _INPUTS:
        _INPUTS[key] = capped(V.vec_inputs(A, B, D, SEED, form, metric))
    return _INPUTS[key]


def test_inputs_are_as_described():
    for form in V.FORMS:
        a, b = V.vec_inputs(33, 70, 68, SEED, form, True), V.vec_inputs(33, 70, 68, SEED, form, False)
        assert a.X.shape == (33, 68) and a.Y.shape == (70, 68) and a.go.shape == (33, 70) and a.XM.shape == a.X.shape
        assert all(t.dtype == np.float32 for t in (a.X, a.Y, a.go, a.XM, a.YM))
        assert np.array_equal(a.X, b.X) and np.array_equal(a.Y, b.Y) and b.XM is None and a.grad_scale in (-2, -1, 1, 2)
        assert not np.array_equal(a.X, V.vec_inputs(33, 70, 68, SEED + 1, form).X)
        assert (a.X[-1] != a.X[-2]).any() and (a.Y[-1] != a.Y[-2]).any() and (a.X[:, -1] != a.X[:, -2]).any() and a.Y[0, -1] != 0
    i = V.vec_inputs(129, 193, 68, SEED, "integer", True)
    assert set(np.unique(i.X)) == set(range(-3, 4)) == set(np.unique(i.Y)) and set(np.unique(i.go)) == {1, 2, 3}
    M = V.metric_matrix(68)
    assert M[0, 0] == 2 and M[0, 1] == 1 and M[1, 0] == 0 and np.array_equal(i.XM, i.X.astype(np.float64) @ M)
    f = V.vec_inputs(129, 193, 68, SEED, "float")
    assert 1 <= np.abs(f.X).min() and np.abs(f.X).max() <= 2 and 0.25 <= np.abs(f.Y).min() and np.abs(f.Y).max() <= 0.5
    assert 0.5 <= f.go.min() and f.go.max() <= 1.5 and (f.X > 0).any() and (f.X < 0).any()


def test_integer_inputs_keep_every_partial_sum_below_2_to_24():
    top = {m: max(V.assert_exact_sums(V.vec_inputs(A, B, D, SEED, "integer", m)) for A, B, D in [(300, 300, 512), (129, 193, 68), (65, 70, 512)])
           for m in (False, True)}
    print("largest sum of absolute values:", top)
    assert top[False] < 2 ** 16 and top[True] < 2 ** 20  # orders of magnitude of headroom below 2^24
    big = V.vec_inputs(*V.FUSED_BIG_SHAPES[1], SEED, "integer", True)
    assert V.assert_exact_sums(big) < 2 ** 24
    bad = V.vec_inputs(5, 5, 3, SEED, "integer")
    bad.X[0, 0] = 0.5
    with pytest.raises(AssertionError):
        V.assert_exact_sums(bad)
    bad.X[0, 0] = 2.0 ** 24
    with pytest.raises(AssertionError):
        V.assert_exact_sums(bad)


def test_geometry_restated_equals_the_library_query():
    """`fused_geometry` against `sigsvgd_vec_fused_workspace_bytes` (host only) at every fused shape, and the geometry the
    several-tiles shapes are there for"""
    from sigsvgd_amd import _lib

    L = _lib.load()
    for A, B, D in FUSED_SHAPES + [(2048, 2048, 40), (1024, 1024, 448)]:
        n = ctypes.c_size_t(0)
        assert L.sigsvgd_vec_fused_workspace_bytes(A, B, D, ctypes.byref(n)) == 0
        assert n.value == V.fused_workspace_bytes(A, B, D), (A, B, D)
    g = V.fused_geometry(4097, 641)
    assert g == {"rows": 65, "ntile": 11, "splits": 6, "per": 2}  # 8 splits wanted, 2 tiles each, the sixth owns one
    assert V.fused_geometry(64, 65) == {"rows": 1, "ntile": 2, "splits": 2, "per": 1}
    assert V.fused_geometry(4097, 641, grad=False)["splits"] == 11


def test_references_agree_with_the_oracle_classes():
    inp = V.vec_inputs(9, 12, 7, SEED, "float", True)
    X, Y, M = inp.X.astype(np.float64), inp.Y.astype(np.float64), V.metric_matrix(7)
    hh = V.half_inv_h2(7, True)
    h = float(np.sqrt(0.5 / hh))
    XM, YM = X @ M, Y @ M  # (unrounded: the oracle's own operands)
    sq = V.sq_reference(X, Y, XM, YM)
    assert np.allclose(sq, VO.scaled_pw_dist_sq(X, Y, M)[0], rtol=1e-14)
    K, dK, _ = VO.scaled_imq(X, Y, M, h)
    assert np.allclose(V.kernel_reference(sq, "imq", hh)[0], K, rtol=1e-14)
    assert np.allclose(V.dk_reference(sq, XM, YM, None, "imq", hh, -0.5 / h ** 2), dK, rtol=1e-13)
    K, dK, _ = VO.gaussian(X, Y, h)
    sq = V.sq_reference(X, Y)
    assert np.allclose(V.kernel_reference(sq, "gaussian", hh)[0], K, rtol=1e-14)
    assert np.allclose(V.dk_reference(sq, X, Y, None, "gaussian", hh, -1 / h ** 2), dK, rtol=1e-13)
    assert np.array_equal(V.sq_reference(X, Y, X, Y, absolute=True), sq)


def test_bounds_and_gate_on_hand_computed_values():
    X, Y = np.array([[3.0, 1.0]], np.float32), np.array([[1.0, 1.0], [0.0, 2.0]], np.float32)
    inp = V.VecInputs(X, Y, np.array([[1.0, 2.0]], np.float32), None, None, 2.0, "float")
    assert np.array_equal(V.sq_reference(X, Y), [[4.0, 10.0]])
    g = V.gamma(5)
    assert np.allclose(V.sq_bound_direct(inp), [[4 * g, 10 * g]], rtol=1e-15)
    # centred on Y[0] = (1, 1): x~ = (2, 0), y~ = (0, 0), (-1, 1): a = 4, b = 0, 2; cross = 0, 2 * 2
    assert np.allclose(V.sq_bound_fused(inp), [[4 * g, (4 + 2 + 4) * g]], rtol=1e-15)
    assert np.array_equal(V.dk_reference([[4.0, 10.0]], X, Y, inp.go, "unit", 0.25, 2.0), [[2 * (2 + 2 * 3), 2 * (0 + 2 * -1)]])
    eK, ew = V.kernel_bounds(np.array([[4.0]]), np.array([[0.0]]), "gaussian", 0.25, U32, 1)
    assert np.allclose(eK, 2 * U32 * np.exp(-1.0), rtol=1e-15) and np.array_equal(eK, ew)
    eK, _ = V.kernel_bounds(np.array([[4.0]]), np.array([[0.0]]), "imq", 0.25, U32, 0)
    assert 0.9 * 0.5 * 2 ** -1.5 * 2 * U32 < eK[0, 0] < 1.1 * 0.5 * 2 ** -1.5 * 2 * U32  # |f'(den)| u den at den = 2
    with pytest.raises(AssertionError):
        V.kernel_bounds(np.array([[4.0]]), np.array([[0.0]]), "imq", 0.25, U32, V.F_MAX + 1)
    assert all(0 < f <= V.F_MAX for f in V.F_ULPS.values())
    # the gate: a zero bound demands equality, one unit in the last place is beyond it, so is a non-finite entry
    ref, zero = np.array([[4.0, 10.0]]), np.zeros((1, 2))
    assert V.assert_vec(ref.astype(np.float32), ref, zero, "exact") == 0.0
    for bad in (np.nextafter(ref.astype(np.float32), np.float32(11)), ref * np.nan):
        with pytest.raises(AssertionError):
            V.assert_vec(bad, ref, zero, "gate")
    assert V.assert_vec(ref + 0.5e-6, ref, np.full((1, 2), 1e-6), "inside") == pytest.approx(0.5, rel=1e-6)
    with pytest.raises(AssertionError, match="beyond their bound"):
        V.assert_vec(ref + 2e-6, ref, np.full((1, 2), 1e-6), "outside")
    assert V.function_error_ulps(np.exp(-1.0) * (1 + 3 * 2 * U32), np.array([[4.0]]), "gaussian", 0.25) == pytest.approx(3, rel=1e-6)


@pytest.mark.parametrize("metric", [False, True])
@pytest.mark.parametrize("form", V.FORMS)
def test_fused_order_passes_at_every_shape(form, metric):
    worst = 0.0
    for A, B, D in FUSED_SHAPES:
        inp = inputs(A, B, D, form, metric)
        for kind in (("unit", "imq") if form == "integer" else ("gaussian",)):
            K, dK = V.fused_order(inp, kind, V.half_inv_h2(D, metric))
            r = check_fused(inp, kind, K, dK, f"fused order ({A}, {B}, {D}) {form} {kind}")
            assert r == 0.0 or kind != "unit"
            worst = max(worst, r)
        K0, none = V.fused_order(inp, "gaussian", V.half_inv_h2(D, metric), grad=False)  # the K-only geometry
        e = V.expected(inp, "gaussian", "fused")
        assert none is None and V.assert_vec(K0, e.K, e.e_K, "K only") <= 1.0
    print(f"{form}, metric {metric}: largest error / bound over the shapes = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("form", V.FORMS)
def test_kgrad_order_passes_at_every_shape(form):
    worst = 0.0
    for A, B, D in V.KGRAD_SHAPES:
        inp = V.vec_inputs(A, B, D, SEED, form, metric=(D % 2 == 1))
        for kind, dtype in (("unit", np.float32), ("gaussian", np.float32), ("imq", np.float64)):
            e = V.expected(inp, kind, "two_launch", fp64=dtype is np.float64)
            K, dK = V.kgrad_order(e.sq.astype(dtype), inp, kind, e.hh)
            V.assert_vec(K, e.K, e.e_K, f"kgrad order ({A}, {B}, {D})", "K")  # (fl(sq) is within e_sq of sq)
            worst = max(worst, V.assert_vec(dK, e.dK, e.e_dK, f"kgrad order ({A}, {B}, {D}) {form} {kind}", "dK", stage=V.GC))
    assert worst <= 1.0


def test_float_inputs_keep_every_channel_far_above_the_bound():
    margins = {}
    for A, B, D in FUSED_SHAPES:
        margins[(A, B, D)] = V.float_margin(inputs(A, B, D, "float", False), "fused")
    for A, B, D in V.SQDIST_SHAPES + V.KGRAD_SHAPES + [(65, 70, 512)]:
        margins[("direct", A, B, D)] = V.float_margin(V.vec_inputs(A, B, D, SEED, "float"), "two_launch")
    low = min(margins, key=margins.get)
    print(f"smallest 0.25 / max(sq bound): {margins[low]:.2f} at {low}; fused at D = 512: {margins[(65, 70, 512)]:.2f}, "
          f"direct at D = 512: {margins[('direct', 65, 70, 512)]:.2f}")
    assert margins[low] >= 2
    assert margins[(65, 70, 512)] >= 3.5 and margins[("direct", 65, 70, 512)] >= 5.9
    assert all(m > 50 for k, m in margins.items() if k[-1] <= 129)


@pytest.mark.parametrize("form", V.FORMS)
@pytest.mark.parametrize("mutation", V.FUSED_MUTATIONS)
def test_each_fused_mistake_fails_the_checker(mutation, form):
    tried = 0
    for metric in ((False, True) if form == "integer" else (False,)):  # (float form with a metric: see vec_reference)
        for A, B, D in MUTATION_SHAPES:
            if not V.fused_applies(mutation, A, B, D, metric):
                continue
            inp = inputs(A, B, D, form, metric)
            kind, hh = ("unit" if form == "integer" else "gaussian"), V.half_inv_h2(D, metric)
            good, bad = V.fused_order(inp, kind, hh), V.fused_order(inp, kind, hh, mutation=mutation)
            assert not all(np.array_equal(a, b) for a, b in zip(good, bad)), (mutation, A, B, D, "changed nothing")
            with pytest.raises(AssertionError, match="beyond their bound"):
                check_fused(inp, kind, *bad, mutation)
            tried += 1
    assert tried >= 2, (mutation, tried)


@pytest.mark.parametrize("form", V.FORMS)
@pytest.mark.parametrize("mutation", V.KGRAD_MUTATIONS)
def test_each_two_launch_mistake_fails_the_checker(mutation, form):
    tried = 0
    for A, B, D in V.KGRAD_SHAPES:
        if not V.kgrad_applies(mutation, A, B, D):
            continue
        inp = V.vec_inputs(A, B, D, SEED, form)
        kind = "unit" if form == "integer" else "gaussian"
        e = V.expected(inp, kind, "two_launch")
        _, good = V.kgrad_order(e.sq.astype(np.float32), inp, kind, e.hh)
        _, bad = V.kgrad_order(e.sq.astype(np.float32), inp, kind, e.hh, mutation)
        if np.array_equal(good, bad):  # (two neighbours of a small integer draw can coincide)
            assert form == "integer" and A * B <= 33, (mutation, A, B, D, "changed nothing")
            continue
        with pytest.raises(AssertionError, match="beyond their bound"):
            V.assert_vec(bad, e.dK, e.e_dK, mutation, "dK", stage=V.GC)
        tried += 1
    assert tried >= 20, (mutation, tried)


def test_mutations_apply_where_the_code_has_the_edge():
    assert not V.fused_applies("stale_last_S_stage", 65, 70, 64) and V.fused_applies("stale_last_S_stage", 65, 70, 65)
    assert V.fused_applies("stale_last_S_stage", 65, 70, 33, metric=True)
    assert not V.fused_applies("stale_b_from_previous_tile", 129, 193, 68) and V.fused_applies("stale_b_from_previous_tile", 4097, 641, 5)
    assert not V.fused_applies("last_split_left_out_of_join", 65, 63, 5) and V.fused_applies("last_split_left_out_of_join", 64, 65, 5)
    assert not V.fused_applies("tail_column_of_K_from_its_neighbour", 65, 1, 5)
    assert all(V.fused_applies(m, 4097, 641, 68) for m in V.FUSED_MUTATIONS)
