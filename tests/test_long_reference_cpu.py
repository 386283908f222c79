"""tests/long_reference.py checked on the host: the input conditions on the fp64 reference over every case, the reference against
the oracle, the restatement's class errors E_c (printed), every MISTAKE failing the class assertion at every case it touches,
and (printed, not asserted; `python tests/test_long_reference_cpu.py` prints it alone, for profiles/long_points.txt) which
mistakes pass rel_max < 1e-5 on rough walks as tests/test_gpu_exact_adjoint.py, test_gpu_log_k.py, test_gpu_normalized.py and
test_gpu_nan_tails.py draw them, at the same shapes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import exact_adjoint_reference as EA  # noqa: E402
import log_k_reference as LK  # noqa: E402
import long_reference as L  # noqa: E402
from oracle import sigkernel_oracle as O  # noqa: E402
from parity import bounded_points, rel_max  # noqa: E402

CASE_FAMILIES = [(c, "close") for c in L.CLOSE_CASES] + [(c, "bounded") for c in L.BOUNDED_CASES]
FLAG_CASES = [(c, f) for f in ("gg", "exact", "log", "norm") for c in L.cases_of(f)]


def _diag_logs(Z, n):
    return np.array([LK.log_gram(Z[i:i + 1], Z[i:i + 1], EA.RBF, L.H, n)[0, 0] for i in range(len(Z))])


# ---- the input conditions --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,family", CASE_FAMILIES, ids=[f"{c}-{f}" for c, f in CASE_FAMILIES])
def test_every_K_is_positive_and_every_cell_is_live(case, family):
    X, Y, _, _ = L.inputs(case, family)
    n = L.CASES[case][3]
    assert X.astype(np.float32).astype(np.float64).tobytes() == X.tobytes()  # fp32-valued
    for P_, Q_ in ((X, Y), (X, X), (Y, Y)):
        assert np.isfinite(LK.log_gram(P_, Q_, EA.RBF, L.H, n)).all(), "a pair has K <= 0"  # (ln K is NaN there)
        D = np.abs(O.increments(EA.static_gram(P_, Q_, EA.RBF, L.H)))
        live = (D > L.LIVE * D.max(axis=(2, 3), keepdims=True)).mean(axis=(2, 3))
        print(f"    {case} {family}: live cells of the worst pair {live.min():.4f}")
        assert live.min() >= L.LIVE_SHARE


def test_bounded_paths_grow_past_the_drift_threshold_and_past_fp32():
    X, Y, _, _ = L.inputs("T131", "bounded")
    a = np.concatenate([_diag_logs(X, 0), _diag_logs(Y, 0)])
    print("    ln K(x, x) at 131 points:", np.round(a, 2))
    assert a.min() > 40
    X, Y, _, _ = L.inputs("past_fp32", "bounded")
    a = np.concatenate([_diag_logs(X, 0), _diag_logs(Y, 0)])
    print(f"    ln K(x, x) at {L.PAST_FP32_T} points:", np.round(a, 2))
    assert a.min() > 88.8
    # the smallest such T of these seeds: one point fewer, and a path stays inside fp32
    T, d = L.PAST_FP32_T - 1, L.CASES["past_fp32"][2]
    s, sd = 100 * list(L.CASES).index("past_fp32") + L.SEED_BUMP.get(("past_fp32", "bounded"), 0), L.BOUNDED_SIZE / np.sqrt(d)
    Z = np.concatenate([bounded_points(1000 + s, L.A, T, d, sd), bounded_points(2000 + s, L.B, T, d, sd)]).astype(np.float64)
    assert _diag_logs(Z, 0).min() <= 88.8


@pytest.mark.parametrize("case,flag", FLAG_CASES, ids=[f"{c}-{f}" for c, f in FLAG_CASES])
def test_every_point_has_a_gradient(case, flag):
    """above 1e-4 of the tensor's largest entry, in both gradients of the two-sided launch and in the Y_IS_X launch's"""
    for form in ("long2", "yx"):
        _, gX, gY = L.plain(case, flag, form)
        for name, g in (("gX", gX), ("gY", gY)):
            if g is not None:
                pt = np.abs(g).max(axis=2)
                print(f"    {case} {flag} {form} {name}: weakest point {float(pt.min() / pt.max()):.2e} of the largest entry")
                assert (pt > L.WEAKEST_POINT * pt.max()).all()


@pytest.mark.parametrize("case,flag", FLAG_CASES, ids=[f"{c}-{f}" for c, f in FLAG_CASES])
def test_a_dropped_S_entry_on_a_seam_row_shows(case, flag):
    """rows 63, 64, 127, 128 (those the case has), every column: zeroing that S entry in every pair moves gX or gY by more than
    1e-5 of its largest entry.  (The gradients are linear in S: the change is the entry's own contribution, at four points.
    NORMALIZED: the cross pairs' S = d ln K / dD under their weights w K^.)"""
    X, Y, w, _ = L.inputs(case, L.FAMILY[flag])
    ref = L.plain(case, flag, "long2")
    hidden, counted = hidden_S_entries(X, Y, w * ref[0] if flag == "norm" else w, L.CASES[case][3], flag, ref)
    print(f"    {case} {flag}: hidden {hidden} of {counted}")
    assert hidden == {r: 0 for r in hidden}


def hidden_S_entries(X, Y, w, n, flag, ref):
    """{row: columns at which a zeroed S[row][column] of every pair stays within 1e-5 of the largest entry of both gradients}"""
    _, S = L.pair_S(EA.static_gram(X, Y, EA.RBF, L.H), n, flag)
    _, gX, gY = ref
    sign = np.array([[1.0, -1.0], [-1.0, 1.0]])
    hidden, counted = {}, S.shape[3]
    for a in L.SEAM_ROWS:
        if a >= S.shape[2]:
            continue
        hidden[a] = 0
        for b in range(S.shape[3]):
            wR = (w * S[:, :, a, b])[:, :, None, None] * sign
            dx, dy = LK._chain(X[:, a:a + 2], Y[:, b:b + 2], wR, EA.RBF, L.H)
            hidden[a] += not (np.abs(dx).max() > L.CONTRACT * np.abs(gX).max() or np.abs(dy).max() > L.CONTRACT * np.abs(gY).max())
    return hidden, counted


# ---- the reference against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["P65_Q8", "n1_T66", "n2_T33"])
def test_gg_reference_is_the_oracles(case):
    X, Y, w, _ = L.inputs(case, "close")
    n = L.CASES[case][3]
    K, gX, gY = L.plain(case, "gg", "long2")
    Ko, gXo = O.gram_backward(X, Y, w, O.RBF, L.H, n)
    _, gYo = O.gram_backward(Y, X, w.T, O.RBF, L.H, n)
    assert np.abs(K / Ko - 1).max() < 1e-12 and rel_max(gX, gXo) < 1e-12 and rel_max(gY, gYo) < 1e-12
    # the forms: first slot only, Y_IS_X (each ordered pair), SYM, pairs
    assert rel_max(L.plain(case, "gg", "long")[1], gXo) < 1e-12
    _, _, _, wyx = L.inputs(case, "close")
    for form, sym in (("yx", False), ("yx_sym", True)):
        assert rel_max(L.plain(case, "gg", form)[1], O.gram_backward(X, X, wyx, O.RBF, L.H, n, sym=sym)[1]) < 1e-12
    Kp, gXp, gYp = L.plain(case, "gg", "pair")
    for i in range(L.B):
        _, gi = O.gram_backward(X[i:i + 1], Y[i:i + 1], w[0, i].reshape(1, 1), O.RBF, L.H, n)
        assert rel_max(gXp[i:i + 1], gi) < 1e-12


def test_references_of_the_flags_are_the_existing_helpers():
    X, Y, w, _ = L.inputs("n1_T66", "close")
    _, gX, gY = EA.gram_backward(X, Y, w, EA.RBF, L.H, 1)
    ref = L.plain("n1_T66", "exact", "long2")
    assert rel_max(ref[1], gX) < 1e-12 and rel_max(ref[2], gY) < 1e-12
    X, Y, w, wyx = L.inputs("n1_T66", "bounded")
    l, gX, gY = LK.log_gram_backward(X, Y, w, EA.RBF, L.H, 1)
    ref = L.plain("n1_T66", "log", "long2")
    assert np.abs(ref[0] - l).max() < 1e-12 and rel_max(ref[1], gX) < 1e-12 and rel_max(ref[2], gY) < 1e-12
    Kh, gX, gY = LK.normalized_gram_and_grads(X, Y, w, EA.RBF, L.H, 1)
    ref = L.plain("n1_T66", "norm", "long2")
    assert rel_max(ref[0], Kh) < 1e-12 and rel_max(ref[1], gX) < 1e-12 and rel_max(ref[2], gY) < 1e-12
    Kh, gX, _ = LK.normalized_gram_and_grads(X, X.copy(), wyx - np.diag(np.diag(wyx)), EA.RBF, L.H, 1)
    ref = L.plain("n1_T66", "norm", "yx")
    assert rel_max(ref[0], Kh) < 1e-12 and rel_max(ref[1], gX) < 1e-12


def test_restatement_without_its_roundings_is_the_reference():
    """the restatement's own sweeps (powers of two under LOG_K, lambda and c apart under EXACT_ADJOINT) give the helpers' S"""
    for flag in ("exact", "log"):
        X, Y, _, _ = L.inputs("n1_T66", L.FAMILY[flag])
        G = EA.static_gram(X, Y, EA.RBF, L.H)
        val, stored, other, _ = L._factors(G, 1, flag, False)
        S = EA.block_sum(stored * other, 1)
        v0, S0 = L.pair_S(G, 1, flag)
        assert np.abs(val - v0).max() < 1e-11 * np.abs(v0).max() and rel_max(S, S0) < 1e-10


def test_classes_sit_on_the_seams_of_the_code():
    cl = L.classes(131, 0, True)
    assert cl["band"] == [63, 64, 65, 127, 128, 129] and cl["pass"] == [62, 63, 64, 125, 126, 127] and cl["wrap"] == [127, 128, 129]
    assert "wrap" not in L.classes(131, 0) and "wrap" not in L.classes(129, 0, True)  # (N - 1 = 128 columns fit the ring)
    assert L.classes(33, 2)["band"] == [15, 16, 17] and L.classes(66, 1)["band"] == [31, 32, 33, 63, 64]  # (65 is an end)
    assert "band" not in L.classes(9, 0) and "pass" not in L.classes(40, 1)
    assert L.ring_W(131, 0) == 128 and L.ring_W(40, 1) == 64


# ---- the restatement's error, and the mistakes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,flag", FLAG_CASES + [("T131", "nan")], ids=[f"{c}-{f}" for c, f in FLAG_CASES] + ["T131-nan"])
def test_restatement_error_per_class(case, flag):
    """E_c, printed; the restatement itself passes the class assertion (MARGIN > 1) and the contract"""
    for (side, k), e in sorted(L.class_error(case, flag).items()):
        print(f"    E case={case} flag={flag} {side} class={k}: {e:.3e}")
    for form in L.forms_of(flag):
        _, failed = L.check_launch(case, flag, form, "f64", L.restated(case, flag, form), printer=None)
        assert not failed, failed
    if flag in ("gg", "exact"):
        for k, e in sorted(L.pde_class_error(case, flag).items()):
            print(f"    E case={case} flag={flag} dG class={k}: {e:.3e}")


@pytest.mark.parametrize("kind", EA.KINDS)
def test_restatement_error_of_the_static_kinds(kind):
    for flag in ("gg", "exact"):
        K = L.plain("T131", flag, "long2", kind)[0]
        assert (K > 0).all()
        E = L.class_error("T131", flag, kind)
        print(f"    kind {kind} {flag}: largest E_c {max(E.values()):.3e}")


MISTAKE_CASES = [(m, c, f, form) for m in L.MISTAKES for (c, f) in FLAG_CASES for form in L.forms_of(f) if L.touches(m, c, f, form)]


@pytest.mark.parametrize("mistake,case,flag,form", MISTAKE_CASES, ids=["-".join(t) for t in MISTAKE_CASES])
def test_every_mistake_fails_the_class_assertion(mistake, case, flag, form):
    """in every form of every (case, flag) that `touches` names"""
    got = L.restated(case, flag, form, EA.RBF, mistake)
    worst, failed = L.check_launch(case, flag, form, "f64", got, printer=None)
    print(f"    {mistake} {case} {flag} {form}: worst err / tol {max(worst.values()):.3g}")
    assert [f for f in failed if f[1] != "contract"], (mistake, case, flag, form)


@pytest.mark.parametrize("mistake", ["band_seam_one_side", "partial_dropped", "stale_forward_cell", "ring_wrap", "pass_seam"])
def test_pde_mistakes_fail_the_cell_assertion(mistake):
    for case in ("T131", "n1_T66"):
        if L.touches(mistake, case, "gg", "long2"):
            _, failed = L.check_pde(case, "gg", "f64", L.pde_restated(case, "gg", mistake)[1], printer=None)
            assert [f for f in failed if f[1] != "contract"], (mistake, case)


# ---- what the old inputs let through (printed, not asserted) -------------------------------------------------------------------------
ROUGH = [("T131", 0.5), ("T131", 2.0), ("P65_Q8", 0.5), ("Q130", 0.5), ("d17", 0.5), ("n1_T66", 0.5), ("n2_T33", 0.5)]


def rough_table():
    """lines: per shape of long_reference.CASES on rough walks as tests/test_gpu_exact_adjoint.py, test_gpu_log_k.py,
    test_gpu_normalized.py and test_gpu_nan_tails.py draw them (cumulative steps of 0.5 per channel, and 2.0 at T131), and on this
    file's inputs at the same shape: (a) the live cells, (b) per seam row the columns at which a zeroed S entry stays hidden,
    (c) the strongest interior and the weakest point, (d) per mistake whether rel_max < 1e-5 still passes"""
    lines = []
    for case, step in ROUGH + [(c, None) for c in L.CLOSE_CASES]:
        label = f"rough walks, steps of {step}" if step else "close (this file)"
        X, Y, w, _ = L.rough_inputs(case, step) if step else L.inputs(case, "close")
        n = L.CASES[case][3]
        D = np.abs(O.increments(EA.static_gram(X, Y, EA.RBF, L.H)))
        live = (D > L.LIVE * D.max(axis=(2, 3), keepdims=True)).mean(axis=(2, 3))
        ref = L.plain(case, "gg", "long2", EA.RBF, step)
        hidden, counted = hidden_S_entries(X, Y, w, n, "gg", ref)
        lines.append(f"{case} {label}: live cells per pair {live.min():.3f} .. {live.max():.3f}; hidden columns of {counted} per row "
                     f"{hidden}")
        pt = np.abs(ref[1]).max(axis=2)
        lines.append(f"    gX: strongest interior point {pt[:, 2:-2].max() / pt.max():.3f} of the strongest point, "
                     f"weakest {pt.min() / pt.max():.1e}")
        for m in L.MISTAKES:
            if L.touches(m, case, "gg", "long2"):
                got = L.restated(case, "gg", "long2", EA.RBF, m, step)
                e = max(rel_max(got[1], ref[1]), rel_max(got[2], ref[2]))
                lines.append(f"    {m}: rel_max {e:.2e} -> {'PASSES' if e < L.CONTRACT else 'fails'} rel_max < 1e-5")
    return lines


def test_rough_inputs_table():
    print("\n".join(rough_table()))


if __name__ == "__main__":
    print("\n".join(rough_table()))
