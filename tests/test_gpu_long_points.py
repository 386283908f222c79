"""The long route's gradients per point class on the device (ring_sweep.h, gram_long_kernels.h, long_static.h), on inputs that
keep every cell of the grid live: tests/long_reference.py has the inputs, the classes, the fp64 reference, the restatement of the
kernels' two fp32 roundings and the tolerance rule, and tests/test_long_reference_cpu.py checks that checker on the host (every
wrong kernel of long_reference.MISTAKES fails these assertions at every case it touches).

The shapes are the smallest at which each mechanism exists (long_reference.CASES).  A = 3, B = 2 with signed weights; the Y_IS_X
launches run A = 3 with asymmetric weights.  Launch forms: ops.gram_long_fwd_bwd ("long"), ops.gram_long_fwd_bwd2 with both sides
("long2"), Y_IS_X ("yx") and Y_IS_X | SYM ("yx_sym"), ops.pair_fwd_bwd under SIGSVGD_PAIR_MODE=serial ("pair"; the band-parallel
schedule must give the same bits where ops.pair_schedule has more than one wave), and ops.pde_fwd_bwd ("pde", dG per cell class
on the cases' own static-kernel grids).  Unflagged (GG) and exact_adjoint launches run every case and form on the `close` inputs;
log_k and normalized run T131, n1_T66 and the past-fp32 case on the `bounded` inputs, two-sided forms; nan_tails runs T131 with
lengths 63, 64, 65, 127 and 131 against the truncated pairs, the rows past a path's end exact zeros; the six static kinds run
T131 two-sided; fp32 I/O runs T131, P65_Q8 and n2_T33.

Every launch asserts the existing contract (K per entry and rel_max < 1e-5 of each gradient; ln K and K^ as tests/test_gpu_log_k.py
and tests/test_gpu_normalized.py bound them), the class tolerances, and the same bits from a second call.  One PERPOINT line per
(family, case, form, io, flag, class) with err, tol, E and the worst point is printed before anything is asserted."""
import numpy as np
import pytest
import torch

import exact_adjoint_reference as EA
import log_k_reference as LK
import long_reference as L
from parity import np64, rel_entry

pytestmark = pytest.mark.gpu

IO = {"f64": torch.float64, "f32": torch.float32}
INV_H = 1.0 / L.H
WORST = {}  # (family, flag, class) -> the largest err / tol of the file, for test_worst_ratio_summary


def dev(a, io, gpu):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=IO[io], device=gpu)


def same_bits(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def numpy_out(out):
    return tuple(None if t is None else np64(t) for t in out)


def keep(family, flag, worst):
    for k, v in worst.items():
        key = (family, flag, k[1] if isinstance(k, tuple) else k)
        WORST[key] = max(WORST.get(key, 0.0), v)


def check_value(case, flag, form, io, got, ref):
    """the existing contract of a launch's first result: K per entry; ln K within (1e-12, fp32 I/O 2 * 2^-24) max(1, |ln K|) times
    the pair's cancellation; K^ within the sum of its three logarithms' bounds, relatively"""
    if flag in ("gg", "exact", "nan"):
        e = rel_entry(got, ref, 0.0)
        print(f"    K per entry {e:.2e}")
        assert e < L.CONTRACT
        return
    X, Y, _, _ = L.inputs(case, "bounded")
    Y = X if form in ("yx", "yx_sym") else Y
    n = L.CASES[case][3]
    unit = lambda v: (1e-12 if io == "f64" else 2 * 2.0 ** -24) * np.maximum(1.0, np.abs(v))
    c = LK.cancellation(X, Y, EA.RBF, L.H, n)
    if flag == "log":
        worst = float((np.abs(got - ref) / (unit(ref) * c)).max())
    else:
        l = LK.log_gram(X, Y, EA.RBF, L.H, n)
        a = LK.log_pair_backward(X, X, None, EA.RBF, L.H, n)[0]
        b = a if Y is X else LK.log_pair_backward(Y, Y, None, EA.RBF, L.H, n)[0]
        u = lambda v: 1e-12 * np.maximum(1.0, np.abs(v))
        tol = u(l) * c + 0.5 * u(a)[:, None] + 0.5 * u(b)[None, :] + (3 * 2.0 ** -24 if io == "f32" else 0.0)
        worst = float((np.abs(got - ref) / (np.abs(ref) * tol)).max())
    print(f"    first result: {worst:.2e} of its bound")
    assert worst <= 1.0


def launch(gpu, case, flag, form, io, kind=EA.RBF):
    """-> a function of no arguments that runs the launch and returns (K, gX, gY) as device tensors"""
    from sigsvgd_amd import ops

    X, Y, w, wyx = L.inputs(case, L.FAMILY[flag])
    n = L.CASES[case][3]
    kw = dict(exact_adjoint=True) if flag == "exact" else {}
    if flag == "nan":
        lx, ly = L.nan_lengths(form)
        X, Y = X.copy(), Y.copy()
        for Z, lens in ((X, lx),) if form == "yx" else ((X, lx), (Y, ly)):
            for i, l in enumerate(lens):
                Z[i, l:] = np.nan
        kw = dict(nan_tails=True)
    if flag in ("log", "norm"):
        kw = dict(log_k=True) if flag == "log" else dict(normalized=True)
    Xt, Yt, wt, wyxt = dev(X, io, gpu), dev(Y, io, gpu), dev(w, io, gpu), dev(wyx, io, gpu)
    if form == "long":
        return lambda: (*ops.gram_long_fwd_bwd(Xt, Yt, INV_H, n, kind, wt, **kw), None)
    if form == "long2":
        return lambda: ops.gram_long_fwd_bwd2(Xt, Yt, INV_H, n, kind, wt, **kw)
    if form in ("yx", "yx_sym"):
        return lambda: ops.gram_long_fwd_bwd2(Xt, Xt, INV_H, n, kind, wyxt, sym=form == "yx_sym", y_is_x=True, **kw)
    assert form == "pair"
    Xp, wp = Xt[:L.B].contiguous(), wt[0].contiguous()
    return lambda: ops.pair_fwd_bwd(Xp, Yt, INV_H, n, kind, wp, **kw)


def run(gpu, case, flag, form, io, kind=EA.RBF):
    """the three assertions of a gradient launch"""
    go = launch(gpu, case, flag, form, io, kind)
    out = go()
    got = numpy_out(out)
    ref = L.plain(case, flag, form, kind)
    assert all(np.isfinite(g).all() for g in got if g is not None)
    worst, failed = L.check_launch(case, flag, form, io, got, kind, where=f"family={L.FAMILY[flag]}")
    keep(L.FAMILY[flag], flag, worst)
    check_value(case, flag, form, io, got[0], ref[0])
    assert (got[2] is None) == (ref[2] is None)
    assert not failed, failed
    assert same_bits(out, go())
    return out


GRAD_CASES = [(c, io) for c in L.CLOSE_CASES for io in (("f64", "f32") if c in L.F32_CASES else ("f64",))]
LOG_CASES = [(c, io) for c in L.BOUNDED_CASES for io in (("f64", "f32") if c == "T131" else ("f64",))]
ids = lambda cases: [f"{c}-{io}" for c, io in cases]


@pytest.mark.parametrize("form", ["long", "long2", "yx", "yx_sym"])
@pytest.mark.parametrize("flag", ["gg", "exact"])
@pytest.mark.parametrize("case,io", GRAD_CASES, ids=ids(GRAD_CASES))
def test_gram_launches(gpu, case, io, flag, form):
    run(gpu, case, flag, form, io)


@pytest.mark.parametrize("flag", ["gg", "exact"])
@pytest.mark.parametrize("case,io", GRAD_CASES, ids=ids(GRAD_CASES))
def test_pair_launch(gpu, monkeypatch, case, io, flag):
    from sigsvgd_amd import ops

    TX, TY, d, n = L.CASES[case]
    monkeypatch.setenv("SIGSVGD_PAIR_MODE", "serial")
    assert ops.pair_schedule(L.B, TX, TY, d, n, exact_adjoint=flag == "exact")[0] == 1
    out = run(gpu, case, flag, "pair", io)
    monkeypatch.setenv("SIGSVGD_PAIR_MODE", "bands")
    if ops.pair_schedule(L.B, TX, TY, d, n, exact_adjoint=flag == "exact")[0] > 1:
        assert same_bits(out, launch(gpu, case, flag, "pair", io)())


@pytest.mark.parametrize("flag", ["gg", "exact"])
@pytest.mark.parametrize("case,io", GRAD_CASES, ids=ids(GRAD_CASES))
def test_pde_launch(gpu, case, io, flag):
    from sigsvgd_amd import ops

    G, w = L.pde_grids(case)
    n = L.CASES[case][3]
    Gt, wt = dev(G, io, gpu), dev(w, io, gpu)
    go = lambda: ops.pde_fwd_bwd(Gt, n, wt, False, exact_adjoint=flag == "exact")
    out = go()
    K, dG = numpy_out(out)
    Kref, _ = L.pde_plain(case, flag)
    worst, failed = L.check_pde(case, flag, io, dG, where="family=close")
    keep("close", flag + " pde", worst)
    assert rel_entry(K, Kref, 0.0) < L.CONTRACT
    assert not failed, failed
    assert same_bits(out, go())


@pytest.mark.parametrize("form", L.TWO_SIDED)
@pytest.mark.parametrize("flag", ["log", "norm"])
@pytest.mark.parametrize("case,io", LOG_CASES, ids=ids(LOG_CASES))
def test_log_domain_launches(gpu, case, io, flag, form):
    out = run(gpu, case, flag, form, io)
    if flag == "norm" and form != "long2":
        assert torch.equal(out[0].diagonal(), torch.ones(L.A, dtype=IO[io], device=gpu)) and torch.equal(out[0], out[0].T)


@pytest.mark.parametrize("form", ["long2", "yx"])
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_nan_tails(gpu, io, form):
    """T131 with lengths 63, 64, 127 (X) and 65, 131 (Y): per class against the truncated pairs, exact zeros past each end"""
    out = run(gpu, "T131", "nan", form, io)
    lx, ly = L.nan_lengths(form)
    for g, lens in ((out[1], lx), (out[2], ly)):
        if g is not None:
            assert all(not g[i, l:].any() for i, l in enumerate(lens))


@pytest.mark.parametrize("flag", ["gg", "exact"])
@pytest.mark.parametrize("kind", EA.KINDS)
def test_static_kinds(gpu, kind, flag):
    run(gpu, "T131", flag, "long2", "f64", kind)


def test_worst_ratio_summary():
    """a reporter, not a check (every launch above asserts its own classes): the largest err / tol per input family, flag and
    class over the launches that ran before it in this process, for profiles/long_points.txt"""
    for (family, flag, k), v in sorted(WORST.items()):
        print(f"    WORST family={family} flag={flag} class={k}: err / tol {v:.3f}")
