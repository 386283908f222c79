"""Host-side checks of the paired entry points (`sigsvgd_pair_*`, include/sigsvgd_hip.h), of their plan, of the predicate
`ops.pair_takes` and of the routing of `SigKernel.compute_kernel`; no device needed (every library call below returns before
any device work, and the routing tests run on oracle-backed doubles of the ops)."""
import ctypes

import numpy as np
import pytest
import torch

from cabi import assert_exported, BADARG, FAKE, lib, UNSUPPORTED
from oracle import sigkernel_oracle as O
from plans import device_cus, pair_plan
from sigsvgd_amd import _lib, ops

NAMES = ("sigsvgd_pair_workspace_bytes", "sigsvgd_pair_fwd", "sigsvgd_pair_fwd_bwd")


def pair_ws(A, TX, TY, d, n, kind=_lib.STATIC_RBF, want_grad=1, flags=0, out=True):
    b = ctypes.c_size_t(12345)
    rc = lib().sigsvgd_pair_workspace_bytes(A, TX, TY, d, n, kind, want_grad, flags, ctypes.byref(b) if out else None)
    return rc, b.value


def test_pair_symbols_exported():
    assert_exported(NAMES, abi=10)


@pytest.mark.parametrize("case", ["A<1", "TX<2", "TY<2", "d<1", "kind", "order", "order<0", "sym", "y_is_x", "generic",
                                  "null_bytes"])
def test_pair_bad_arguments(case):
    args = dict(A=3, TX=300, TY=200, d=2, n=0, kind=_lib.STATIC_RBF, flags=0)
    upd = {"A<1": dict(A=0), "TX<2": dict(TX=1), "TY<2": dict(TY=1), "d<1": dict(d=0), "kind": dict(kind=5),
           "order": dict(n=11), "order<0": dict(n=-1), "sym": dict(flags=_lib.FLAG_SYM), "y_is_x": dict(flags=_lib.FLAG_Y_IS_X),
           "generic": dict(flags=_lib.FLAG_FORCE_GENERIC | _lib.FLAG_NAIVE_SOLVER), "null_bytes": {}}[case]
    a = {**args, **upd}
    rc, _ = pair_ws(a["A"], a["TX"], a["TY"], a["d"], a["n"], a["kind"], 1, a["flags"], out=case != "null_bytes")
    assert rc == BADARG, _lib.last_error()
    if case == "null_bytes":
        return
    L = lib()
    geo = (a["A"], a["TX"], a["TY"], a["d"], _lib.F32, 1.0, a["n"], a["kind"], a["flags"])
    assert L.sigsvgd_pair_fwd(FAKE, FAKE, *geo, FAKE, FAKE, 1 << 30, None) == BADARG, _lib.last_error()
    assert L.sigsvgd_pair_fwd_bwd(FAKE, FAKE, *geo, None, FAKE, FAKE, FAKE, FAKE, 1 << 30, None) == BADARG, _lib.last_error()


def test_pair_launch_argument_checks():
    L = lib()
    geo = (3, 300, 200, 2)
    fwd = lambda X, Y, dtype, inv_h, kind, K: L.sigsvgd_pair_fwd(X, Y, *geo, dtype, inv_h, 0, kind, 0, K, None, 0, None)
    # null pointers, bad dtype, RBF without a bandwidth: refused before any device work
    assert fwd(None, FAKE, _lib.F32, 1.0, 0, FAKE) == BADARG
    assert fwd(FAKE, None, _lib.F32, 1.0, 0, FAKE) == BADARG
    assert fwd(FAKE, FAKE, _lib.F32, 1.0, 0, None) == BADARG
    assert fwd(FAKE, FAKE, 7, 1.0, 0, FAKE) == BADARG
    assert fwd(FAKE, FAKE, _lib.F64, 0.0, _lib.STATIC_RBF, FAKE) == BADARG
    assert fwd(FAKE, FAKE, _lib.F64, -1.0, _lib.STATIC_RBF, FAKE) == BADARG
    # both gradient outputs NULL
    rc = L.sigsvgd_pair_fwd_bwd(FAKE, FAKE, *geo, _lib.F32, 1.0, 0, 0, 0, None, FAKE, None, None, FAKE, 1 << 30, None)
    assert rc == BADARG and "NULL" in _lib.last_error()
    rc = L.sigsvgd_pair_fwd_bwd(None, FAKE, *geo, _lib.F32, 1.0, 0, 0, 0, None, FAKE, FAKE, FAKE, FAKE, 1 << 30, None)
    assert rc == BADARG
    # the one flag taken
    assert pair_ws(3, 300, 200, 2, 0, flags=_lib.FLAG_NAIVE_SOLVER)[0] == 0, _lib.last_error()
    for kind in (_lib.STATIC_RBF, _lib.STATIC_LINEAR):
        assert pair_ws(3, 300, 200, 2, 0, kind)[0] == 0


@pytest.mark.parametrize("n", range(11))
def test_pair_refuses_grids_past_8192(n):
    edge = 8192 // (1 << n) + 1  # points giving 8192 cells
    for want_grad in (0, 1):
        for (TX, TY) in [(edge, edge), (edge, 3), (3, edge)]:
            assert pair_ws(2, TX, TY, 2, n, want_grad=want_grad)[0] == 0, _lib.last_error()
        for (TX, TY) in [(edge + 1, edge), (edge, edge + 1), (edge + 1, 2), (2, edge + 1)]:
            rc, _ = pair_ws(2, TX, TY, 2, n, want_grad=want_grad)
            assert rc == UNSUPPORTED and "8192" in _lib.last_error()
            assert ops.pair_takes(2, TX, TY, 2, n, want_grad=bool(want_grad)) is False


def test_pair_channel_limit():
    """The band's points of X sit in LDS: at T = 300 and order 0 the limit is 183 channels, as on the Gram long route."""
    lds184 = (64 * 128 + 299 + 2 + 64 + 65 * 184) * 8  # ring of 64 rows x 128 columns, boundary row, dump cells, points
    assert lds184 > 160 * 1024 >= lds184 - 65 * 8
    for want_grad in (0, 1):
        assert pair_ws(2, 300, 300, 183, 0, want_grad=want_grad)[0] == 0
        rc, _ = pair_ws(2, 300, 300, 184, 0, want_grad=want_grad)
        assert rc == UNSUPPORTED
        assert "LDS" in _lib.last_error() and str(lds184) in _lib.last_error()
    assert pair_plan(2, 300, 300, 183, 0) is not None and pair_plan(2, 300, 300, 184, 0) is None


def test_pair_plan_matches_workspace_query():
    """pair_plan mirrors pair_make_plan: its bytes are the library's over shapes that reach every branch of the plan (ring
    wrap, nrow = 1, more pairs than resident waves, the 1 GiB scratch cap, the LDS limit), with TX != TY."""
    cus = device_cus()
    shapes = [(1, 2, 2), (3, 300, 200), (2, 129, 129), (2, 129, 130), (5, 257, 258), (2, 9, 9), (3, 5, 9), (1, 9, 3),
              (7, 150, 400), (1, 300, 2), (1, 2, 300), (64, 40, 60), (1000, 64, 64), (5000, 20, 20), (100000, 10, 10),
              (64, 1025, 1025), (300, 1025, 700), (16, 2048, 2048)]
    seen = set()
    for (A, M, N) in shapes:
        for n in (0, 1, 2, 3, 6, 7, 10):
            for d in (1, 2, 17, 183, 184):
                for want_grad in (0, 1):
                    rc, b = pair_ws(A, M, N, d, n, want_grad=want_grad)
                    pl = pair_plan(A, M, N, d, n, want_grad, cus)
                    assert (rc == UNSUPPORTED) == (pl is None), (A, M, N, d, n, want_grad, rc)
                    if pl is None:
                        continue
                    assert rc == 0 and b == pl["bytes"], (A, M, N, d, n, want_grad, b, pl)
                    if want_grad == 0:
                        assert b == 0
                    per_wave = (2 * -(-pl["P"] // 64) * (pl["Q"] + 63) * 64 + 64) * 4
                    if want_grad and pl["grid"] < min(A, pl["resident"]):
                        seen.add("cap")
                        assert per_wave * pl["grid"] <= (1 << 30) or pl["grid"] == 1
                    if A > pl["resident"]:
                        seen.add("more_pairs")
                    if pl["nrow"] == 1 and pl["P"] > 64:
                        seen.add("nrow1")
                    if N - 1 > pl["W"]:
                        seen.add("wrap")
    assert {"cap", "more_pairs", "nrow1", "wrap"} <= seen, seen


def test_pair_takes_predicate():
    assert ops.pair_takes(1024, 64, 64, 7, 0) is True
    assert ops.pair_takes(4, 300, 200, 3, 0, want_grad=False) is True
    assert ops.pair_takes(2, 8194, 10, 2, 0) is False
    assert ops.pair_takes(2, 10, 10, 300, 0) is False  # LDS: the band's 65 points of X in 300 channels
    with pytest.raises(RuntimeError):  # a bad argument is an error, not a route
        ops.pair_takes(4, 64, 64, 7, 0, static_kind=9)


# ---- routing of SigKernel.compute_kernel on oracle-backed doubles (CPU tensors) ---------------------------------------------
def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _pair_oracle(X, Y, inv_h, n, kind, naive, go=None):
    """(K [A], gX [A,TX,d], gY [A,TY,d]) per pair from the numpy oracle: gX the first slot of (X_i, Y_i), gY the first slot
    of the swapped pair (Y_i, X_i)."""
    Xn, Yn = _np(X), _np(Y)
    A = Xn.shape[0]
    w = np.ones(A) if go is None else _np(go)
    K, gX, gY = np.empty(A), np.empty_like(Xn), np.empty_like(Yn)
    for i in range(A):
        Ki, gXi = O.gram_backward(Xn[i:i + 1], Yn[i:i + 1], w[i:i + 1, None], kind, 1.0 / inv_h, n, naive)
        _, gYi = O.gram_backward(Yn[i:i + 1], Xn[i:i + 1], w[i:i + 1, None], kind, 1.0 / inv_h, n, naive)
        K[i], gX[i], gY[i] = Ki[0, 0], gXi[0], gYi[0]
    return K, gX, gY


def _patch(monkeypatch, calls):
    def pair_fwd(X, Y, inv_h, dyadic_order=0, static_kind=0, naive=False):
        calls.append("pair_fwd")
        return torch.as_tensor(_pair_oracle(X, Y, inv_h, dyadic_order, static_kind, naive)[0], dtype=X.dtype)

    def pair_fwd_bwd(X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, want_x=True, want_y=True):
        calls.append(("pair_fwd_bwd", want_x, want_y))
        K, gX, gY = _pair_oracle(X, Y, inv_h, dyadic_order, static_kind, naive, grad_out)
        t = lambda a: torch.as_tensor(a, dtype=X.dtype)
        return t(K), t(gX) if want_x else None, t(gY) if want_y else None

    def refuse(name):
        def fn(*a, **k):
            calls.append(name)
            raise AssertionError(f"compute_kernel called {name}")
        return fn

    monkeypatch.setattr(ops, "pair_fwd", pair_fwd)
    monkeypatch.setattr(ops, "pair_fwd_bwd", pair_fwd_bwd)
    for name in ("gram_fwd", "gram_fwd_bwd", "gram_long_fwd", "gram_long_fwd_bwd", "gram_sym_partial"):
        monkeypatch.setattr(ops, name, refuse(name))


@pytest.mark.parametrize("static", ["rbf", "linear"])
def test_compute_kernel_routes_to_pairs(monkeypatch, static):
    import sigsvgd_amd.sigkernel as sk

    calls = []
    _patch(monkeypatch, calls)
    k = sk.SigKernel(sk.RBFKernel(0.7) if static == "rbf" else sk.LinearKernel(), 1)
    g = torch.Generator().manual_seed(3)
    X = (0.3 * torch.randn(3, 5, 2, generator=g, dtype=torch.float64)).cumsum(1)
    Y = (0.3 * torch.randn(3, 4, 2, generator=g, dtype=torch.float64)).cumsum(1)
    kind = _lib.STATIC_RBF if static == "rbf" else _lib.STATIC_LINEAR
    inv_h = 1.0 / 0.7 if static == "rbf" else 1.0
    Kr, gXr, gYr = _pair_oracle(X, Y, inv_h, 1, kind, False)

    Xb = (0.3 * torch.randn(20, 5, 2, generator=g, dtype=torch.float64)).cumsum(1)
    Yb = (0.3 * torch.randn(20, 4, 2, generator=g, dtype=torch.float64)).cumsum(1)
    K = k.compute_kernel(Xb, Yb)  # no gradient, 400 > 256 pairs in the Gram launch: the paired forward
    assert calls == ["pair_fwd"] and np.allclose(_np(K), _pair_oracle(Xb, Yb, inv_h, 1, kind, False)[0], rtol=1e-12)

    for (rx, ry) in [(True, True), (True, False), (False, True)]:
        calls.clear()
        Xg, Yg = X.clone().requires_grad_(rx), Y.clone().requires_grad_(ry)
        w = torch.tensor([0.5, -1.25, 2.0], dtype=torch.float64)
        (k.compute_kernel(Xg, Yg) * w).sum().backward()
        assert calls == [("pair_fwd_bwd", rx, ry)]  # one launch, unit weights, only the outputs needed
        w_ = _np(w)[:, None, None]
        if rx:
            assert np.allclose(_np(Xg.grad), gXr * w_, rtol=1e-10, atol=1e-14)
        else:
            assert Xg.grad is None
        if ry:
            assert np.allclose(_np(Yg.grad), gYr * w_, rtol=1e-10, atol=1e-14)
        else:
            assert Yg.grad is None

    # the same tensor in both slots: the sum of both derivatives
    calls.clear()
    Xs = (0.3 * torch.randn(3, 5, 2, generator=g, dtype=torch.float64)).cumsum(1).requires_grad_(True)
    k.compute_kernel(Xs, Xs).sum().backward()
    _, g1, g2 = _pair_oracle(Xs, Xs, inv_h, 1, kind, False)
    assert calls == [("pair_fwd_bwd", True, True)]
    assert np.allclose(_np(Xs.grad), g1 + g2, rtol=1e-10, atol=1e-14)

    # compute_distance: three paired launches, no Gram launch
    calls.clear()
    k.compute_distance(Xb[:, :4], Yb)
    assert calls == ["pair_fwd"] * 3
    calls.clear()
    k.compute_distance(Xb[:, :4].clone().requires_grad_(True), Yb)
    assert calls == [("pair_fwd_bwd", True, True), "pair_fwd", ("pair_fwd_bwd", True, False)]


def test_compute_kernel_gradient_dtypes(monkeypatch):
    import sigsvgd_amd.sigkernel as sk

    calls = []
    _patch(monkeypatch, calls)
    X = (0.3 * torch.randn(2, 4, 2, dtype=torch.float32)).cumsum(1).requires_grad_(True)
    Y = (0.3 * torch.randn(2, 6, 2, dtype=torch.float64)).cumsum(1).requires_grad_(True)
    K = sk.SigKernel(sk.RBFKernel(1.0), 0).compute_kernel(X, Y)
    assert K.dtype == torch.float32  # computed in X's dtype
    K.sum().backward()
    assert X.grad.dtype == torch.float32 and Y.grad.dtype == torch.float64


def test_compute_kernel_falls_back_where_pairs_refuse(monkeypatch):
    """T = 10 with d = 300 at order 0: the paired plan's LDS overflows, the fused Gram route takes the launch; compute_kernel
    keeps today's Gram diagonal there."""
    import sigsvgd_amd.sigkernel as sk
    from helpers import gram_fwd, gram_fwd_bwd

    calls = []
    _patch(monkeypatch, calls)
    assert ops.pair_takes(2, 10, 10, 300, 0) is False and ops.gram_takes(2, 2, 10, 300, 0) is True

    def spy(name, fn):
        def wrapped(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(ops, "gram_fwd", spy("gram_fwd", gram_fwd))
    monkeypatch.setattr(ops, "gram_fwd_bwd", spy("gram_fwd_bwd", gram_fwd_bwd))
    g = torch.Generator().manual_seed(4)
    X = (0.02 * torch.randn(2, 10, 300, generator=g, dtype=torch.float64)).cumsum(1)
    Y = (0.02 * torch.randn(2, 10, 300, generator=g, dtype=torch.float64)).cumsum(1)
    k = sk.SigKernel(sk.RBFKernel(4.0), 0)
    K = k.compute_kernel(X, Y)
    assert calls == ["gram_fwd"]
    Kr = O.gram(_np(X), _np(Y), O.RBF, 4.0, 0)
    assert np.allclose(_np(K), np.diag(Kr), rtol=1e-12)
    calls.clear()
    Xg = X.clone().requires_grad_(True)
    k.compute_kernel(Xg, Y).sum()
    assert calls == ["gram_fwd_bwd"] and "pair_fwd" not in calls


def test_small_forward_rule(monkeypatch):
    """Forward-only calls of A^2 <= CUs pairs that the fused Gram kernels take stay on the Gram diagonal (DESIGN.md section
    5.11); with a gradient, with more pairs, or where the fused kernels refuse, the paired route takes them."""
    import sigsvgd_amd.sigkernel as sk

    R = lambda A, T, d, n, g, cus=256: sk._pair_route(A, T, T, d, _lib.STATIC_RBF, n, g, False, cus)
    assert R(6, 100, 3, 3, False) is False       # the reference's arm-spline example, forward: Gram diagonal
    assert R(6, 100, 3, 3, True) is True         # with a gradient: paired
    assert R(16, 100, 3, 3, False) is False      # 256 pairs: one round of 256 CUs
    assert R(17, 100, 3, 3, False) is True       # 289 pairs: paired
    assert R(16, 100, 3, 3, False, cus=128) is True
    assert R(100, 10, 2, 4, False) is True       # notebook
    assert R(1024, 64, 7, 0, False) is True      # SVGD's C4 batch
    assert R(4, 300, 3, 0, False) is True        # the fused kernels refuse T = 300: paired
    assert R(2, 10, 300, 0, True) is False       # the paired plan refuses: Gram diagonal

    calls = []
    _patch(monkeypatch, calls)
    from helpers import gram_fwd

    monkeypatch.setattr(ops, "gram_fwd", lambda *a, **k: (calls.append("gram_fwd"), gram_fwd(*a, **k))[1])
    X = (0.3 * torch.randn(3, 6, 2, dtype=torch.float64)).cumsum(1)
    k = sk.SigKernel(sk.RBFKernel(0.7), 1)
    K = k.compute_kernel(X, X.flip(0))
    assert calls == ["gram_fwd"]
    assert np.allclose(_np(K), np.diag(O.gram(_np(X), _np(X.flip(0)), O.RBF, 0.7, 1)), rtol=1e-12)
