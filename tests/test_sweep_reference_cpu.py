"""The inputs, point classes, reference and checker of the per-point Gram tests, checked on the CPU (tests/sweep_reference.py;
the device tests are tests/test_gpu_every_length.py).

The generator and the classes are pinned to literal values; the plain solve is the oracle; the three conditions on the inputs
hold on the oracle over the whole case matrix; the restatement of the kernels' fp32 arithmetic meets the contract with the
margin applied (4 E < 1e-5 over the whole tensor, every case and launch form) and passes its own class assertion; each of seven
wrong kernels restated on top of it fails the class assertion at every length where the mistake can happen.  Each mistake test
also prints, at every eighth of those lengths, whether the earlier metric -- rel_max < 1e-5 and K per entry, on `walks(.., 0.05)`
(refined grids: 0.3) -- would have passed the wrong kernel; over all of them it passes 1 of 928 (mistake, length) combinations,
the skipped last group at T = 3, order 7: the mistakes as restated are whole steps and whole points, which any metric sees --
what the earlier files lacked is the lengths.  With an `assert_classes` that always passes, 16 of the 25 tests here fail: the 16
mistake tests."""
import numpy as np
import pytest

import sweep_reference as S
from oracle import sigkernel_oracle as O
from parity import rel_entry, rel_max, signed_weights, sized_walks

FAMILY_CASES = {"fast": [c for c in S.ORDER0_CASES if c[0] <= 64], "quad": [c for c in S.ORDER0_CASES if c[0] > 64],
                "refined": S.REFINED_CASES}


def test_generator_and_weights_are_pinned():
    X, Y, w, wyx = S.inputs(5, 2)
    assert X.dtype == Y.dtype == np.float32 and X.shape == (3, 5, 2) and Y.shape == (2, 5, 2) and w.shape == (3, 2) and wyx.shape == (3, 3)
    assert np.array_equal(X, sized_walks(np.random.default_rng(1005), 3, 5, 2, 0.9 / np.sqrt(2.0)))
    assert np.array_equal(Y, sized_walks(np.random.default_rng(2005), 2, 5, 2, 0.9 / np.sqrt(2.0)))
    np.testing.assert_allclose(X[0, :2], [[-0.2023845, -0.051663626], [-0.3667762, -0.09635926]], rtol=0, atol=1e-7)
    np.testing.assert_allclose(Y[1, -1], [1.3668834, -1.1311306], rtol=0, atol=1e-7)
    np.testing.assert_allclose(w[0], [1.214926004, -1.32221818], rtol=0, atol=1e-7)
    assert np.array_equal(w, signed_weights(3, 2, 3005).astype(np.float32)) and np.array_equal(wyx, signed_weights(3, 3, 4005).astype(np.float32))
    for (T, d, n) in S.ALL_CASES[::37]:
        _, _, w, wyx = S.inputs(T, d)
        for a in (w, wyx):
            assert 0.5 <= np.abs(a).min() and np.abs(a).max() <= 1.5 and (a > 0).any() and (a < 0).any()
        assert np.abs(wyx - wyx.T).max() > 0.1  # (asymmetric: w_ji for w_ij is a different gradient)


def test_point_classes_are_pinned():
    assert S.classes(3, 0) == dict(ends=[0, 2], next=[1])
    assert S.classes(4, 0) == dict(ends=[0, 3], next=[1, 2])
    assert S.classes(5, 0) == dict(ends=[0, 4], next=[1, 3], interior=[2])
    assert S.classes(64, 0) == dict(ends=[0, 63], next=[1, 62], interior=list(range(2, 62)))
    assert "handover" not in S.classes(65, 0) and S.seam_points(65, 0) == []
    assert S.classes(66, 0)["handover"] == [63] and S.seam_points(66, 0) == [64]
    assert S.classes(67, 0)["handover"] == [63, 64]
    assert S.classes(128, 0)["handover"] == [63, 64, 65] and S.classes(128, 0)["interior"] == list(range(2, 126))
    assert "handover" not in S.classes(33, 1) and S.seam_points(33, 1) == []  # (64 cells: one band, no seam)


def test_refined_point_classes_are_pinned():
    assert S.seam_points(5, 5) == [2] and S.classes(5, 5) == dict(ends=[0, 4], next=[1, 3], interior=[2], handover=[1, 2, 3])
    assert S.seam_points(3, 7) == [1] and S.seam_points(3, 6) == [1]
    assert S.classes(3, 6) == dict(ends=[0, 2], next=[1], handover=[0, 1, 2])
    assert S.seam_points(10, 4) == [4, 8] and S.classes(10, 4)["handover"] == [3, 4, 5, 7, 8, 9]
    assert S.seam_points(30, 3) == [8, 16, 24] and S.seam_points(17, 2) == []
    tn = S.refined_tn()
    assert len(tn) == 67 and len(set(tn)) == 67 and (33, 1) in tn and (3, 7) in tn and (3, 5) in tn and (2, 7) not in tn
    assert len(S.ORDER0_CASES) == 62 * 4 + 6 * 3 + 64 * 4 and len(S.REFINED_CASES) == 67 * 3


def test_plain_solve_is_the_oracle():
    for (T, d, n) in [(7, 3, 0), (5, 2, 2), (66, 2, 0)]:
        X, Y, w, wyx = S.inputs(T, d)
        K, g, _ = S.plain(T, d, n, "ordered")
        Kr, gr = O.gram_backward(X, Y, w, O.RBF, S.H, n)
        assert rel_entry(K, Kr, 0) < 1e-12 and rel_max(g, gr) < 1e-11
        for form, sym in (("yx", False), ("yx-sym", True)):
            K, g, _ = S.plain(T, d, n, form)
            Kr, gr = O.gram_backward(X, X, wyx, O.RBF, S.H, n, False, sym)
            assert rel_entry(K, Kr, 0) < 1e-12 and rel_max(g, gr) < 1e-11
    # the unordered form of the restatement in fp64 arithmetic is the ordered one: row side + column side of a pair once
    X, _, _, wyx = S.inputs(9, 3)
    X = X.astype(np.float64)
    Kp, row, col, _ = S._pairs(X[[0, 0, 1]], X[[1, 2, 2]], S.H, 1, False, None)
    Kq, rowq, _, _ = S._pairs(X[[1, 2, 2]], X[[0, 0, 1]], S.H, 1, False, None)
    assert S.kernel_of("fast") is None and S.kernel_of("band serial") == S.kernel_of("band parallel") == "band"
    assert S.refined_kernels(33, 1) == ["dyad"] and S.refined_kernels(5, 5) == ["dyad", "band"] and S.refined_kernels(10, 4) == ["band"]
    assert rel_entry(Kp, Kq, 0) < 1e-12 and rel_max(col, rowq) < 1e-11


def test_input_conditions_hold_on_the_oracle():
    """the three conditions of the module docstring over the whole case matrix: the last-cell weights on the X x Y pairs, the K
    range over every K the device tests compare with -- the X x Y pairs and the Y-is-X batch, k(x_i, x_i) included"""
    for name, cases in (("order0", S.ORDER0_CASES), ("refined", S.REFINED_CASES)):
        below = pairs = 0
        best, klo, khi = np.inf, np.inf, 0.0
        for (T, d, n) in cases:
            K, _, L = S.plain(T, d, n, "ordered")
            assert L.max() >= S.LAST_CELL_MIN, (T, d, n, L.max())
            below, pairs, best = below + int((L < S.LAST_CELL_MIN).sum()), pairs + L.size, min(best, L.max())
            for Kc in (K, S.plain(T, d, n, "yx")[0]):
                klo, khi = min(klo, np.abs(Kc).min()), max(khi, np.abs(Kc).max())
        print(f"{name}: {below} of {pairs} pairs below 1e-4 ({100.0 * below / pairs:.1f} %), every case's best pair >= {best:.1e}, "
              f"K in [{klo:.3f}, {khi:.3f}]")
        assert below <= 0.10 * pairs
        assert S.K_RANGE[0] <= klo and khi <= S.K_RANGE[1]
        fb, fp, fbest, flo, fhi = S.LAST_CELL_FIGURES[name]
        assert (below, pairs) == (fb, fp) and abs(best / fbest - 1) < 0.06 and abs(klo - flo) < 6e-3 and abs(khi - fhi) < 6e-2


@pytest.mark.parametrize("family", list(FAMILY_CASES))
def test_restatement_meets_the_contract_with_the_margin(family):
    """4 E < 1e-5 over the whole tensor, E_K < 1e-5 per entry, and the restatement passes its own class assertion, at every
    case and launch form; prints the largest E_c per class"""
    worst = {}
    for (T, d, n) in FAMILY_CASES[family]:
        for form, kern in [(f, k) for f in S.FORMS for k in (S.refined_kernels(T, n) if n else [None])]:
            EK, Eg, E = S.restatement_error(T, d, n, form, kern)
            assert S.MARGIN * Eg < S.CONTRACT and EK < S.CONTRACT, (T, d, n, form, kern, EK, Eg)
            Kp, gp, _ = S.plain(T, d, n, form)
            Kr, gr = S.restated(T, d, n, form, kernel=kern)
            S.assert_contract(Kr, Kp, gr, gp)
            tol = S.tolerances(T, d, n, form, "f64", kern)
            m = S.class_metrics(gr, gp, T, n)
            top = np.abs(gp).max()
            for k, (e, _, den) in m.items():
                assert e < tol[k] <= S.CONTRACT * top / den * (1 + 1e-12), (T, d, n, form, kern, k, e, tol[k])
                if E[k] > worst.get((kern, k), (0,))[0]:
                    worst[kern, k] = (E[k], T, d, n, form)
    for (kern, k), v in sorted(worst.items(), key=str):
        print(f"ECLASS {kern or family} {k}: largest E_c {v[0]:.2e} at T={v[1]} d={v[2]} n={v[3]} {v[4]}")


# ---- seven wrong kernels ------------------------------------------------------------------------------------------------------
MISTAKE_FORM = dict(seam_one_side="ordered", last_group_skipped="ordered", early_cut="ordered", ring_wrap_early="ordered",
                    column_sum_missing_first="yx", column_sum_missing_last="yx", wji_for_wij="yx")


def _lengths(family, mistake):
    """one case per (T, n) of the family that the mistake touches: the smallest d of the case matrix there"""
    seen, out = set(), []
    for (T, d, n) in FAMILY_CASES[family]:
        if (T, n) not in seen and S.touches(mistake, T, d, n, MISTAKE_FORM[mistake]):
            seen.add((T, n))
            out.append((T, d, n))
    return out


MISTAKE_TESTS = [(m, f) for m in S.MISTAKES for f in FAMILY_CASES if _lengths(f, m)]


def test_mistakes_touch_what_they_name():
    assert len(MISTAKE_TESTS) == 16, MISTAKE_TESTS
    assert [c[0] for c in _lengths("fast", "ring_wrap_early")] == [33]
    assert _lengths("fast", "seam_one_side") == [] and _lengths("fast", "early_cut") == [] == _lengths("refined", "early_cut")
    assert [c[0] for c in _lengths("quad", "seam_one_side")] == list(range(66, 129))
    early = [c[0] for c in _lengths("quad", "early_cut")]
    assert max(early) <= 112 and 73 in early and 112 in early and len(early) >= 40, early
    assert len(_lengths("refined", "seam_one_side")) == len([tn for tn in S.refined_tn() if S.seam_points(*tn)]) >= 50
    assert not S.touches("early_cut", 100, 16, 0, "ordered") and S.touches("early_cut", 100, 14, 0, "ordered")
    assert not S.touches("wji_for_wij", 20, 2, 0, "yx-sym") and not S.touches("column_sum_missing_last", 20, 2, 0, "ordered")


@pytest.mark.parametrize("mistake,family", MISTAKE_TESTS, ids=[f"{m}-{f}" for m, f in MISTAKE_TESTS])
def test_mistake_fails_the_class_assertion(mistake, family):
    form = MISTAKE_FORM[mistake]
    missed = []
    cases = _lengths(family, mistake)
    for (T, d, n) in cases:
        Kp, gp, _ = S.plain(T, d, n, form)
        _, g = S.restated(T, d, n, form, mistake)
        for io in ("f32", "f64"):
            with pytest.raises(AssertionError):
                S.assert_classes(T, d, n, form, io, g, gp, where=mistake)
    survey = cases[::8]  # (printed, not asserted: a sample keeps the file quick)
    for (T, d, n) in survey:
        Ko, go, _ = S.plain(T, d, n, form, True)
        Kw, gw = S.restated(T, d, n, form, mistake, True)
        if rel_max(gw, go) < S.CONTRACT and rel_entry(Kw, Ko, 1e-6) < S.CONTRACT:
            missed.append((T, n))
    print(f"OLDMETRIC {mistake} {family}: the earlier metric on the earlier inputs passes the wrong kernel at {len(missed)} of "
          f"{len(survey)} sampled lengths: {missed}")
