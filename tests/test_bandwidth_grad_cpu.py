"""The gradient of a static-kernel sigma, the parts that need no GPU: the reference expression of
tests/test_gpu_bandwidth_grad.py tied to the oracle, the host side of the four C entry points, and which launches
`sigsvgd_amd.sigkernel` makes for a sigma that requires grad.

Reference.  dK/dh = sum_{m,n} R[m][n] (-phi'(s)) s / h with R the 4-corner scatter of the block sums of GG (`RR._solve`): the
reference's GG convention chained exactly through the static kernel.  GG is the exact adjoint of the first-order stencil, so
with that stencil the expression is the derivative of K and a central difference of the oracle's K in h must reproduce it: to
1e-6 of the largest entry at a relative step of 1e-5 (truncation ~ step^2, rounding ~ 1e-16 / step; measured 1e-9 to 5e-8).
With the default stencil the two differ by per cents, which is why the reference is the contraction and not a difference."""
import ctypes

import numpy as np
import pytest
import torch

import radial_reference as RR
from bandwidth_reference import dK_dh, dK_dinvh
import sigsvgd_amd.sigkernel as sk
from cabi import BADARG, FAKE, OK, UNSUPPORTED, WORKSPACE, assert_exported, lib
from oracle import sigkernel_oracle as O
from parity import rel_max
from plans import device_cus, long2_plan, pair_plan
from sigsvgd_amd import _lib, ops

RBF, LINEAR, IMQ, RQ = 0, 1, 2, 3
NAIVE, SYM, Y_IS_X = 1, 2, 4


# ---- 1. the reference expression against the oracle ----------------------------------------------------------------------
@pytest.mark.parametrize("A,B,TX,TY,d,n", [(2, 3, 9, 12, 3, 0), (2, 2, 6, 5, 2, 2)])
@pytest.mark.parametrize("h", [0.5, 1.0, 4.0])
def test_contraction_is_the_derivative_under_the_first_order_stencil(A, B, TX, TY, d, n, h):
    X = O.synthetic_inputs(A, TX, d, seed_x=0)[0].double().numpy()
    Y = O.synthetic_inputs(B, TY, d, seed_x=5)[0].double().numpy()
    ref = dK_dh(X, Y, RBF, h, n, naive=True)
    e = 1e-5 * h
    fd = (O.gram(X, Y, RBF, h + e, n, naive=True) - O.gram(X, Y, RBF, h - e, n, naive=True)) / (2.0 * e)
    print("contraction vs central difference", (A, B, TX, TY, d, n, h), rel_max(ref, fd))
    assert rel_max(ref, fd) < 1e-6


def test_reference_helper():
    """the shared helper is the issue's expression on `RR._solve`, and d/d(1/h) = -h^2 d/dh"""
    X = O.synthetic_inputs(2, 9, 3, seed_x=0)[0].double().numpy()
    Y = O.synthetic_inputs(3, 12, 3, seed_x=5)[0].double().numpy()
    for kind in (RR.RBF, RR.IMQ, RR.RQ):
        _, R, _, s = RR._solve(X, Y, kind, 0.5, 1)
        ref = (R * RR.neg_dphi(kind, s) * s).sum((2, 3)) / 0.5
        assert np.array_equal(dK_dh(X, Y, kind, 0.5, 1), ref) and np.array_equal(dK_dinvh(X, Y, kind, 0.5, 1), -0.25 * ref)


# ---- 2. the C ABI, host only ---------------------------------------------------------------------------------------------
def gram_h_ws(A, B, TX, TY, d, n, kind, wx, wy, flags):
    b = ctypes.c_size_t(12345)
    return lib().sigsvgd_gram_long_h_workspace_bytes(A, B, TX, TY, d, n, kind, wx, wy, flags, ctypes.byref(b)), b.value


def pair_h_ws(A, TX, TY, d, n, kind, flags):
    b = ctypes.c_size_t(12345)
    return lib().sigsvgd_pair_h_workspace_bytes(A, TX, TY, d, n, kind, flags, ctypes.byref(b)), b.value


def gram_h(kind=RBF, inv_h=1.0, flags=0, dk=FAKE, ws_bytes=1 << 40, T=10, n=0, gX=FAKE, gY=None, X=FAKE, dtype=1):
    return lib().sigsvgd_gram_long_fwd_bwd_h(X, FAKE, 3, 3, T, T, 2, dtype, inv_h, n, kind, flags, None, FAKE, gX, gY, dk, FAKE,
                                             ws_bytes, None)


def pair_h(kind=RBF, inv_h=1.0, flags=0, dk=FAKE, ws_bytes=1 << 40, T=10, n=0, gX=FAKE, gY=None, X=FAKE, dtype=1):
    return lib().sigsvgd_pair_fwd_bwd_h(X, FAKE, 3, T, T, 2, dtype, inv_h, n, kind, flags, None, FAKE, gX, gY, dk, FAKE, ws_bytes,
                                        None)


def test_entry_points_are_exported_and_the_abi_is_10():
    assert_exported(["sigsvgd_gram_long_h_workspace_bytes", "sigsvgd_gram_long_fwd_bwd_h", "sigsvgd_pair_h_workspace_bytes",
                     "sigsvgd_pair_fwd_bwd_h"], abi=10)


@pytest.mark.parametrize("launch", [gram_h, pair_h], ids=["gram", "pair"])
def test_bad_arguments(launch):
    assert launch(kind=LINEAR) == BADARG and "no bandwidth" in _lib.last_error()
    assert launch(dk=None) == BADARG and "dK_dinvh_out" in _lib.last_error()
    for kind in (RBF, IMQ, RQ):
        assert launch(kind=kind, inv_h=0.0) == BADARG and launch(kind=kind, inv_h=-1.0) == BADARG
        assert launch(kind=kind, inv_h=float("nan")) == BADARG
    assert launch(flags=8) == BADARG and launch(flags=64) == BADARG and "flag" in _lib.last_error()
    assert launch(X=None) == BADARG and launch(dtype=2) == BADARG and launch(kind=4) == BADARG and launch(n=11) == BADARG
    assert launch(kind=IMQ, flags=NAIVE) == UNSUPPORTED and launch(kind=RQ, flags=NAIVE) == UNSUPPORTED


def test_bad_arguments_of_each_mode():
    assert pair_h(flags=SYM) == BADARG and pair_h(flags=Y_IS_X) == BADARG  # the paired mode takes NAIVE_SOLVER only
    assert gram_h(flags=Y_IS_X, gY=FAKE) == BADARG and gram_h(flags=SYM, gY=FAKE) == BADARG
    assert gram_h_ws(3, 4, 10, 10, 2, 0, RBF, 1, 0, Y_IS_X)[0] == BADARG  # Y_IS_X needs one shape
    assert gram_h_ws(3, 3, 10, 10, 2, 0, LINEAR, 1, 0, 0)[0] == BADARG and pair_h_ws(3, 10, 10, 2, 0, LINEAR, 0)[0] == BADARG
    assert lib().sigsvgd_gram_long_h_workspace_bytes(3, 3, 10, 10, 2, 0, RBF, 1, 0, 0, None) == BADARG
    assert lib().sigsvgd_pair_h_workspace_bytes(3, 10, 10, 2, 0, RBF, 0, None) == BADARG


def test_limits_are_the_long_routes():
    # 8192 refined cells on a side are taken, one more is refused; so is the first-order stencil with IMQ / RQ
    assert gram_h_ws(1, 1, 8193, 3, 2, 0, RBF, 0, 0, 0)[0] == OK and pair_h_ws(1, 3, 8193, 2, 0, RBF, 0)[0] == OK
    assert gram_h_ws(1, 1, 8194, 3, 2, 0, RBF, 0, 0, 0)[0] == UNSUPPORTED and "8192" in _lib.last_error()
    assert pair_h_ws(1, 3, 8194, 2, 0, IMQ, 0)[0] == UNSUPPORTED
    assert gram_h_ws(2, 2, 4098, 5, 2, 1, RQ, 1, 1, 0)[0] == UNSUPPORTED
    assert gram_h(T=8194) == UNSUPPORTED and pair_h(T=8194) == UNSUPPORTED
    assert gram_h_ws(2, 2, 9, 9, 2, 0, IMQ, 1, 1, NAIVE)[0] == UNSUPPORTED and pair_h_ws(2, 9, 9, 2, 0, RQ, NAIVE)[0] == UNSUPPORTED
    assert gram_h_ws(2, 2, 9, 9, 2, 0, RBF, 1, 1, NAIVE)[0] == OK


@pytest.mark.parametrize("kind", [RBF, IMQ, RQ])
def test_workspace(kind):
    """With a gradient wanted the two-sided launch's own workspace; with none the per-wave scratch alone (the launch still
    runs the reverse sweep), where the launch without the bandwidth output needs nothing.  One byte short is refused."""
    A, B, TX, TY, d, n = 5, 7, 40, 33, 3, 1
    cus = device_cus()
    for (wx, wy, flags, yx) in [(1, 1, 0, False), (1, 0, 0, False), (0, 1, 0, False)]:
        rc, nbytes = gram_h_ws(A, B, TX, TY, d, n, kind, wx, wy, flags)
        assert rc == OK and nbytes == long2_plan(A, B, TX, TY, d, n, bool(wx), bool(wy), yx, cus)["bytes"]
    rc, nbytes = gram_h_ws(A, A, TX, TX, d, n, kind, 1, 0, SYM)
    assert rc == OK and nbytes == long2_plan(A, A, TX, TX, d, n, True, False, False, cus)["bytes"]
    rc, nbytes = gram_h_ws(A, A, TX, TX, d, n, kind, 1, 0, Y_IS_X)
    assert rc == OK and nbytes == long2_plan(A, A, TX, TX, d, n, True, False, True, cus)["bytes"]
    for (b, ty, flags, yx) in [(B, TY, 0, False), (A, TX, Y_IS_X, True)]:
        full = long2_plan(A, b, TX, ty, d, n, True, not yx, yx, cus)
        rc, nbytes = gram_h_ws(A, b, TX, ty, d, n, kind, 0, 0, flags)
        assert rc == OK and nbytes == full["bytes"] - full["slab_bytes"] > 0  # the scratch alone
        assert long2_plan(A, b, TX, ty, d, n, False, False, yx, cus)["bytes"] == 0
    rc, nbytes = pair_h_ws(A, TX, TY, d, n, kind, 0)
    assert rc == OK and nbytes == pair_plan(A, TX, TY, d, n, True, cus)["bytes"] > 0
    # one byte short (argument checks pass, the plan refuses before anything is launched)
    need = gram_h_ws(3, 3, 10, 10, 2, 0, kind, 1, 0, 0)[1]
    assert gram_h(kind=kind, ws_bytes=need - 1) == WORKSPACE and "required" in _lib.last_error()
    need = gram_h_ws(3, 3, 10, 10, 2, 0, kind, 0, 0, 0)[1]
    assert gram_h(kind=kind, gX=None, ws_bytes=need - 1) == WORKSPACE
    need = pair_h_ws(3, 10, 10, 2, 0, kind, 0)[1]
    assert pair_h(kind=kind, ws_bytes=need - 1) == WORKSPACE and pair_h(kind=kind, gX=None, ws_bytes=need - 1) == WORKSPACE


def test_takes_queries():
    assert ops.gram_long_h_takes(3, 4, 10, 12, 2) and ops.pair_h_takes(3, 10, 12, 2, 1, IMQ)
    assert not ops.gram_long_h_takes(3, 4, 8194, 12, 2) and not ops.pair_h_takes(3, 10, 4098, 2, 1)
    assert not ops.gram_long_h_takes(3, 4, 10, 12, 2, 0, IMQ, naive=True) and not ops.pair_h_takes(3, 10, 12, 2, 0, RQ, True)
    with pytest.raises(RuntimeError):
        ops.gram_long_h_takes(3, 4, 10, 12, 2, 0, LINEAR)


# ---- 3. routing ----------------------------------------------------------------------------------------------------------
class Recorder:
    """every launch function of `ops` a request with a built-in static kernel can reach, recording (name, flags) and
    returning zero tensors of the right shapes (as tests/test_gram_routing_cpu.py does)"""

    def __init__(self, takes=True):
        self.launches, self.takes = [], takes

    def _note(self, name, X, Y, paired=False, **flags):
        self.launches.append((name, tuple(X.shape[:2]), tuple(Y.shape[:2]), " ".join(k for k, v in flags.items() if v)))
        return torch.zeros((X.shape[0],) if paired else (X.shape[0], Y.shape[0]), dtype=X.dtype)

    def gram_takes(self, *a, **k):
        return True

    def pair_takes(self, *a, **k):
        return True

    def gram_long_h_takes(self, *a, **k):
        return self.takes

    def pair_h_takes(self, *a, **k):
        return self.takes

    def gram_fwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, naive=False, force_generic=False, y_is_x=False,
                 stored_forward=False):
        return self._note("gram_fwd", X, Y, yx=y_is_x)

    def gram_fwd_bwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False, y_is_x=False,
                     force_generic=False, check_regime=True, stored_forward=False):
        return self._note("gram_fwd_bwd", X, Y, sym=sym, yx=y_is_x, w=grad_out is not None), torch.zeros_like(X)

    def gram_long_fwd_bwd2(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False,
                           y_is_x=False, want_gradX=True, want_gradY=True):
        K = self._note("gram_long_fwd_bwd2", X, Y, sym=sym, yx=y_is_x, gx=want_gradX, gy=want_gradY, w=grad_out is not None)
        return K, (torch.zeros_like(X) if want_gradX else None), (torch.zeros_like(Y) if want_gradY else None)

    def gram_long_fwd_bwd_h(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False,
                            y_is_x=False, want_gradX=True, want_gradY=True):
        K = self._note("gram_long_fwd_bwd_h", X, Y, sym=sym, yx=y_is_x, gx=want_gradX, gy=want_gradY, w=grad_out is not None)
        return K, (torch.zeros_like(X) if want_gradX else None), (torch.zeros_like(Y) if want_gradY else None), K + 1.0

    def pair_fwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, naive=False):
        return self._note("pair_fwd", X, Y, True)

    def pair_fwd_bwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, want_x=True, want_y=True):
        K = self._note("pair_fwd_bwd", X, Y, True, gx=want_x, gy=want_y)
        return K, (torch.zeros_like(X) if want_x else None), (torch.zeros_like(Y) if want_y else None)

    def pair_fwd_bwd_h(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, want_x=True, want_y=True):
        K = self._note("pair_fwd_bwd_h", X, Y, True, gx=want_x, gy=want_y, w=grad_out is not None)
        return K, (torch.zeros_like(X) if want_x else None), (torch.zeros_like(Y) if want_y else None), K + 1.0


NAMES = ("gram_takes", "pair_takes", "gram_long_h_takes", "pair_h_takes", "gram_fwd", "gram_fwd_bwd", "gram_long_fwd_bwd2",
         "gram_long_fwd_bwd_h", "pair_fwd", "pair_fwd_bwd", "pair_fwd_bwd_h")


def record(monkeypatch, takes=True):
    rec = Recorder(takes)
    for name in NAMES:
        monkeypatch.setattr(ops, name, getattr(rec, name))
    monkeypatch.setattr(sk, "_device_cus", lambda X: 256)
    return rec


def paths(n, t, d, grad):
    return torch.linspace(0.0, 1.0, n * t * d, dtype=torch.float64).reshape(n, t, d).requires_grad_(grad)


STATICS = [sk.RBFKernel, sk.IMQStaticKernel, sk.RationalQuadraticKernel]
SHAPES = [(8, 16, 3), (3, 300, 2)]  # a shape the fused kernels take; a long-route shape


@pytest.mark.parametrize("static", STATICS)
@pytest.mark.parametrize("A,T,d", SHAPES)
def test_learned_sigma_takes_the_bandwidth_launches(monkeypatch, static, A, T, d):
    rec = record(monkeypatch)
    sigma = torch.tensor(1.3, dtype=torch.float32, requires_grad=True)
    k = sk.SigKernel(static(sigma), 1)
    X, Y = paths(A, T, d, True), paths(A + 1, T - 1, d, False)
    K = k.compute_Gram(X, Y)
    assert rec.launches == [("gram_long_fwd_bwd_h", (A, T), (A + 1, T - 1), "gx")]
    W = torch.arange(1.0, K.numel() + 1.0, dtype=K.dtype).reshape(K.shape)
    (W * K).sum().backward()  # non-uniform weights: the coordinate gradient relaunches, sigma's does not
    assert rec.launches[1:] == [("gram_long_fwd_bwd2", (A, T), (A + 1, T - 1), "gx w")]
    # grad_sigma = -inv_h^2 sum(W dK_dinvh), the recorder's dK_dinvh being all ones; in sigma's dtype, shape and device
    assert sigma.grad.dtype == torch.float32 and sigma.grad.shape == sigma.shape
    assert abs(float(sigma.grad) + float(W.sum()) / 1.3**2) < 1e-4 * float(W.sum())
    # sigma alone requires grad: a sigma-only launch, and nothing in backward
    rec.launches.clear()
    sigma.grad = None
    k.compute_Gram(X.detach(), Y).sum().backward()
    assert rec.launches == [("gram_long_fwd_bwd_h", (A, T), (A + 1, T - 1), "")] and sigma.grad is not None
    # one tensor in both slots, sym; grad_Y
    rec.launches.clear()
    k.compute_Gram(X, X, sym=True).sum().backward()
    Yg = paths(A + 1, T - 1, d, True)
    k.compute_Gram(X, Yg, grad_Y=True).sum().backward()
    assert rec.launches == [("gram_long_fwd_bwd_h", (A, T), (A, T), "sym yx gx"),
                            ("gram_long_fwd_bwd_h", (A, T), (A + 1, T - 1), "gx gy")]
    # the paired launch, with and without path gradients
    rec.launches.clear()
    Yp = paths(A, T - 1, d, True)
    k.compute_kernel(X, Yp).sum().backward()
    k.compute_kernel(X.detach(), Yp.detach()).sum().backward()
    assert rec.launches == [("pair_fwd_bwd_h", (A, T), (A, T - 1), "gx gy"), ("pair_fwd_bwd_h", (A, T), (A, T - 1), "")]
    # compute_distance and compute_mmd go through them
    rec.launches.clear()
    k.compute_distance(X, Yp.detach()).backward()
    assert [l[0] for l in rec.launches] == ["pair_fwd_bwd_h"] * 3
    rec.launches.clear()
    k.compute_mmd(X, Yg).backward()
    assert [(l[0], l[3]) for l in rec.launches] == [("gram_long_fwd_bwd_h", "sym yx gx"), ("gram_long_fwd_bwd_h", "sym yx gx"),
                                                    ("gram_long_fwd_bwd_h", "gx")]


def calls_of(monkeypatch, sigma, no_grad=False):
    rec = record(monkeypatch)
    k = sk.SigKernel(sk.RBFKernel(sigma), 0)
    for (A, T, d) in SHAPES:
        X, Y = paths(A, T, d, True), paths(A, T, d, False) + 0.5
        with torch.no_grad() if no_grad else torch.enable_grad():
            K = k.compute_Gram(X, Y)
            Kp = k.compute_kernel(X, Y)
            if not no_grad:
                (K.sum() + Kp.sum()).backward()
    return rec.launches


def test_other_sigmas_make_the_calls_they_always_made(monkeypatch):
    """a float, a plain tensor, and a sigma that requires grad under no_grad: the launches of the float, none of them new"""
    base = calls_of(monkeypatch, 1.3)
    assert base and not any(name.endswith("_h") for name, *_ in base)
    assert calls_of(monkeypatch, torch.tensor(1.3)) == base
    assert calls_of(monkeypatch, torch.tensor(1.3, dtype=torch.float64)) == base
    learned = torch.tensor(1.3, requires_grad=True)
    forward_only = calls_of(monkeypatch, 1.3, no_grad=True)
    assert calls_of(monkeypatch, learned, no_grad=True) == forward_only
    assert not any(name.endswith("_h") for name, *_ in forward_only)
    # a user static kernel keeps the user route: nothing of `ops` above is called
    rec = record(monkeypatch)
    with pytest.raises(RuntimeError):  # (ops.PDESolve wants a device; what matters is that no recorded launch ran)
        sk.SigKernel(type("U", (), {"Gram_matrix": sk.RBFKernel(learned).Gram_matrix})(), 0).compute_Gram(
            paths(3, 5, 2, True), paths(3, 5, 2, False))
    assert rec.launches == []


@pytest.mark.parametrize("static", STATICS)
def test_refused_shapes_raise(monkeypatch, static):
    rec = record(monkeypatch, takes=False)
    k = sk.SigKernel(static(torch.tensor(1.3, requires_grad=True)), 0)
    X = paths(3, 5, 2, True)
    with pytest.raises(NotImplementedError, match="long route"):
        k.compute_Gram(X, X)
    with pytest.raises(NotImplementedError, match="long route"):
        k.compute_kernel(X, X)
    assert rec.launches == []
    with pytest.raises(ValueError, match="one element"):
        sk.SigKernel(static(torch.ones(2, requires_grad=True)), 0).compute_Gram(X, X)


@pytest.mark.parametrize("static", [sk.IMQStaticKernel, sk.RationalQuadraticKernel])
def test_first_order_stencil_with_imq_and_rq_raises(static):
    """the library's own answer (host only): the message names the limit"""
    k = sk.SigKernel(static(torch.tensor(1.3, requires_grad=True)), 0, _naive_solver=True)
    X = paths(3, 5, 2, True)
    with pytest.raises(NotImplementedError, match="NAIVE_SOLVER"):
        k.compute_Gram(X, X)
    with pytest.raises(NotImplementedError, match="NAIVE_SOLVER"):
        k.compute_kernel(X, X)
    big = torch.zeros(1, 8194, 1, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="8192"):
        sk.SigKernel(static(torch.tensor(1.3, requires_grad=True)), 0).compute_Gram(big, big)
