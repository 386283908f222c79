"""The checker of the velocity kernel, checked on the CPU (tests/phi_reference.py; the device tests are tests/test_gpu_phi.py).

`kernel_order` restates svgd_phi_kernel's arithmetic in fp32 numpy.  It passes `assert_phi` in both input forms at every
shape the device file runs, and each of seven mistakes a kernel of that shape can make -- a lost k, a lost quarter, a stale
stage, a neighbour's column, row or float, a wrong 1/N -- fails it in both forms at every shape where the mistake can happen.
That rests on the float inputs' margin, asserted here: the smallest term of a dot product, 0.1/N, is worth at least 8 bounds
(36 and more at these shapes).  With an `assert_phi` that always passes, 15 of the 21 tests here fail: the 14 mutation tests
and the hand-computed gate (tried once).  `kernel_order`'s own largest error / bound is 0.954 in the integer form (two
roundings against a bound of two) and 0.178 in the float form."""
import numpy as np
import pytest

import phi_reference as P
from phi_reference import BENCH_SHAPE, SEED, SHAPES, U


@pytest.fixture(scope="module")
def emulated():
    """(N, D, form) -> (inputs, kernel_order's result), computed once"""
    out = {}
    for N, D in SHAPES:
        for form in P.FORMS:
            I = P.phi_inputs(N, D, SEED, form)
            out[(N, D, form)] = (I, P.kernel_order(*I[:3]))
    return out


def test_inputs_are_as_described():
    for form in P.FORMS:
        K, s, gk, mask, X = P.phi_inputs(33, 70, SEED, form)
        assert K.shape == (33, 33) and all(a.shape == (33, 70) and a.dtype == np.float32 for a in (s, gk, mask, X))
        assert set(np.unique(mask)) == {0.0, 1.0}
        again = P.phi_inputs(33, 70, SEED, form)
        assert all(np.array_equal(a, b) for a, b in zip((K, s, gk, mask, X), again))
        assert not np.array_equal(K, P.phi_inputs(33, 70, SEED + 1, form)[0])
    K, s, gk = P.phi_inputs(260, 132, SEED, "integer")[:3]
    assert set(np.unique(K)) == {1, 2, 3} and set(np.unique(s)) == {-4, -3, -2, -1, 1, 2, 3, 4}
    assert set(np.unique(gk)) == set(range(-8, 9))
    K, s, gk = P.phi_inputs(260, 132, SEED, "float")[:3]
    assert 0.2 <= K.min() and K.max() <= 1.0
    for a in (s, gk):
        assert 0.5 <= np.abs(a).min() and np.abs(a).max() <= 1.5 and (a > 0).any() and (a < 0).any()


def test_reference_and_bound_on_hand_computed_values():
    K, s, gk = np.array([[1.0, 2.0], [3.0, 1.0]]), np.array([[1.0], [-2.0]]), np.array([[4.0], [1.0]])
    assert np.array_equal(P.phi_reference(K, s, gk), [[3.5], [0.0]])  # -((1 - 4 - 4)/2), -((3 - 2 - 1)/2)
    assert np.array_equal(P.phi_bound(K, s, gk, "integer"), [[0.0], [0.0]])  # N = 2: exact
    g = 5 * U / (1 - 5 * U)
    assert np.allclose(P.phi_bound(K, s, gk, "float"), [[g * 4.5], [g * 3.0]], rtol=1e-15, atol=0)
    K3, s3, gk3 = np.ones((3, 3)), np.array([[1.0], [2.0], [4.0]]), np.array([[1.0], [7.0], [8.0]])
    assert np.allclose(P.phi_bound(K3, s3, gk3, "integer"), 2 * U * (1 + U) * np.array([[2.0], [0.0], [1 / 3]]), rtol=1e-15)
    # the gate: one unit in the last place of an exact entry, a non-zero at a zero reference, a non-finite entry
    v = P.phi_reference(K, s, gk).astype(np.float32)
    assert P.assert_phi(v, K, s, gk, "integer", "exact") == 0.0
    assert P.assert_phi(np.array([[3.5], [-0.0]], np.float32), K, s, gk, "integer", "a zero of either sign") == 0.0
    for bad in (np.nextafter(v, np.float32(4)), v + np.array([[0], [1e-30]], np.float32), v * np.float32("nan")):
        with pytest.raises(AssertionError):
            P.assert_phi(bad, K, s, gk, "integer", "gate")
    # a 0/1 mask scales reference and bound; a fractional one adds its rounding
    m = np.array([[0.0], [1.0]])
    assert P.assert_phi(v * m.astype(np.float32), K, s, gk, "integer", "mask", mask=m) == 0.0
    with pytest.raises(AssertionError):
        P.assert_phi(v, K, s, gk, "integer", "mask not applied", mask=m)


@pytest.mark.parametrize("form", P.FORMS)
def test_kernel_order_passes_at_every_shape(emulated, form):
    worst = 0.0
    for N, D in SHAPES:
        (K, s, gk, _, _), v = emulated[(N, D, form)]
        worst = max(worst, P.assert_phi(v, K, s, gk, form, "kernel order"))
    print(f"{form}: largest error / bound over the shapes = {worst:.3f}")
    # derived, not tuned: the integer form's two roundings can reach the bound, a sequential float chain stays far inside
    assert worst <= 1.0


def test_kernel_order_passes_at_the_benchmark_shape():
    K, s, gk, _, _ = P.phi_inputs(*BENCH_SHAPE, SEED, "integer")
    v = P.kernel_order(K, s, gk)
    assert P.assert_phi(v, K, s, gk, "integer", "kernel order") == 0.0  # N = 1024 is a power of two: exact
    assert np.array_equal(v, (-((K.astype(np.float64) @ s - gk) / 1024)).astype(np.float32))


def test_float_inputs_keep_every_term_far_above_the_bound():
    smallest = min(P.float_margin(*P.phi_inputs(N, D, SEED, "float")[:3]) for N, D in SHAPES)
    print(f"smallest (0.1/N) / max(bound) over the shapes: {smallest:.1f}")
    assert smallest >= 8
    for N, D in SHAPES:
        K, s = P.phi_inputs(N, D, SEED, "float")[:2]
        assert (np.abs(K[:, :, None] * s[None, :, :]) >= 0.1 * (1 - 2 * U)).all()


@pytest.mark.parametrize("form", P.FORMS)
@pytest.mark.parametrize("mutation", P.MUTATIONS)
def test_each_mistake_fails_the_checker(emulated, mutation, form):
    tried = 0
    for N, D in SHAPES:
        if not P.applies(mutation, N, D):
            continue
        (K, s, gk, _, _), good = emulated[(N, D, form)]
        v = P.kernel_order(K, s, gk, mutation)
        assert not np.array_equal(v, good), (mutation, N, D, "changed nothing")
        with pytest.raises(AssertionError, match="beyond their bound"):
            P.assert_phi(v, K, s, gk, form, mutation)
        tried += 1
    assert tried >= 10, (mutation, tried)


def test_mutations_apply_where_the_code_has_the_edge():
    assert not P.applies("stale_last_stage", 64, 64) and P.applies("stale_last_stage", 65, 65)
    assert not P.applies("last_column_from_its_neighbour", 15, 1) and not P.applies("last_row_from_its_neighbour", 1, 1)
    assert all(P.applies(m, 68, 68) for m in P.MUTATIONS)
