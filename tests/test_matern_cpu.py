"""The Matern-3/2 and -5/2 static kernels (SIGSVGD_STATIC_MATERN32 = 6, _MATERN52 = 7), the parts that
need no GPU: the numpy reference of tests/matern_reference.py against central differences, the torch forms of
`sigsvgd_amd.sigkernel`, the host side of the C entry points and the Python surface.  Before the feature the constants and
classes do not exist and every query with kind 6 or 7 answers SIGSVGD_E_BADARG.

Reference.  GG is the exact adjoint of the first-order stencil, so with that stencil the reference's gX and dK/d(1/h) are
derivatives of K and central differences of the reference K must reproduce them: to 1e-6 of the largest entry at a relative step
of 1e-5, the bound of tests/test_bandwidth_grad_cpu.py (truncation ~ step^2, rounding ~ 1e-16 / step)."""
import ctypes

import numpy as np
import pytest
import torch

import matern_reference as MR
from cabi import BADARG, FAKE, OK, UNSUPPORTED, lib
from oracle import sigkernel_oracle as O
from parity import rel_max
from sigsvgd_amd import _lib, ops

RBF, LINEAR, IMQ, RQ = _lib.STATIC_RBF, _lib.STATIC_LINEAR, _lib.STATIC_IMQ, _lib.STATIC_RQ
NAIVE = _lib.FLAG_NAIVE_SOLVER
KINDS = list(MR.KINDS)


def paths(A, T, d, seed):
    return O.synthetic_inputs(A, T, d, seed_x=seed)[0].double().numpy()


# ---- 1. the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_slope_is_the_derivative_of_phi(kind):
    for s in (1e-3, 0.3, 2.0, 40.0):
        e = 1e-6 * max(s, 1.0)
        fd = -(MR.phi(kind, s + e) - MR.phi(kind, s - e)) / (2.0 * e)
        # relative to phi's scale at s (the difference of two values of size phi rounds at 1e-16 phi / e)
        assert abs(float(MR.neg_dphi(kind, s)) - fd) < 1e-6 * max(float(MR.neg_dphi(kind, s)), float(MR.phi(kind, s))), s


def test_values_at_zero():
    assert MR.phi(MR.MATERN32, 0.0) == 1.0 and MR.phi(MR.MATERN52, 0.0) == 1.0
    assert MR.neg_dphi(MR.MATERN32, 0.0) == 1.5 and MR.neg_dphi(MR.MATERN52, 0.0) == 5.0 / 6.0
    # the clamp: an argument a few ulp below zero is a coincident point
    assert MR.phi(MR.MATERN32, -1e-16) == 1.0 and MR.neg_dphi(MR.MATERN52, -1e-16) == 5.0 / 6.0
    assert (_lib.STATIC_MATERN32, _lib.STATIC_MATERN52) == (6, 7) == (MR.MATERN32, MR.MATERN52)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("A,B,TX,TY,d,n", [(2, 3, 9, 12, 3, 0), (2, 2, 6, 5, 2, 2)])
def test_contractions_are_derivatives_under_the_first_order_stencil(kind, A, B, TX, TY, d, n):
    X, Y = paths(A, TX, d, 0), paths(B, TY, d, 5)
    h = 1.0
    w = np.random.default_rng(11).standard_normal((A, B))
    _, gX, gY = MR.gram_backward(X, Y, w, kind, h, n, naive=True)
    step = 1e-5
    fdx, fdy = np.zeros_like(X), np.zeros_like(Y)
    for P, fd, first in ((X, fdx, True), (Y, fdy, False)):
        for idx in np.ndindex(*P.shape):
            Pp, Pm = P.copy(), P.copy()
            Pp[idx] += step
            Pm[idx] -= step
            Kp = MR.gram(Pp, Y, kind, h, n, True) if first else MR.gram(X, Pp, kind, h, n, True)
            Km = MR.gram(Pm, Y, kind, h, n, True) if first else MR.gram(X, Pm, kind, h, n, True)
            fd[idx] = (w * (Kp - Km)).sum() / (2.0 * step)
    ref = MR.dK_dinvh(X, Y, kind, h, n, naive=True)
    e = 1e-5 / h
    fdh = (MR.gram(X, Y, kind, 1.0 / (1.0 / h + e), n, True) - MR.gram(X, Y, kind, 1.0 / (1.0 / h - e), n, True)) / (2.0 * e)
    print("matern fd", kind, (A, B, TX, TY, d, n), rel_max(gX, fdx), rel_max(gY, fdy), rel_max(ref, fdh))
    assert rel_max(gX, fdx) < 1e-6 and rel_max(gY, fdy) < 1e-6 and rel_max(ref, fdh) < 1e-6


@pytest.mark.parametrize("kind", KINDS)
def test_y_is_x_is_finite(kind):
    X = paths(4, 7, 2, 0)
    K, gX, gY = MR.gram_backward(X, X, None, kind, 1.0, 2)
    dK = MR.dK_dinvh(X, X, kind, 1.0, 2)
    assert all(np.isfinite(a).all() for a in (K, gX, gY, dK)) and np.allclose(K, K.T, rtol=0, atol=1e-13)
    Kp, gxp, gyp = MR.pair_backward(X, X, None, kind, 1.0, 2)
    assert np.array_equal(Kp, np.diagonal(K)) and np.isfinite(gxp).all() and np.isfinite(gyp).all()
    assert np.array_equal(MR.pair_dK_dinvh(X, X, kind, 1.0, 2), np.diagonal(dK))


# ---- 2. the torch forms ----------------------------------------------------------------------------------------------------
def statics(kind, sigma):
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd import kernels

    cls, batch = ((sk.Matern32StaticKernel, kernels.BatchMatern32Kernel) if kind == MR.MATERN32
                  else (sk.Matern52StaticKernel, kernels.BatchMatern52Kernel))
    return cls(sigma), batch(lambda _: float(sigma))


@pytest.mark.parametrize("kind", KINDS)
def test_torch_forms_equal_the_reference(kind):
    Xn, Yn = paths(3, 9, 3, 0), paths(4, 12, 3, 5)
    X, Y = torch.as_tensor(Xn), torch.as_tensor(Yn)
    sigma = 0.7
    for static in statics(kind, sigma):
        assert static.static_kind == kind and static.inv_bandwidth(X, Y) == 1.0 / sigma
        G = static.Gram_matrix(X, Y).numpy()
        assert G.shape == (3, 4, 9, 12) and np.abs(G - MR.static_gram(Xn, Yn, kind, sigma)).max() < 1e-12
        Gb = static.batch_kernel(X, Y[:3]).numpy()
        ref = np.stack([MR.static_gram(Xn[i:i + 1], Yn[i:i + 1], kind, sigma)[0, 0] for i in range(3)])
        assert Gb.shape == (3, 9, 12) and np.abs(Gb - ref).max() < 1e-12


@pytest.mark.parametrize("kind", KINDS)
def test_autograd_through_coincident_points(kind):
    """Gram_matrix(X, X) has a zero distance on every diagonal cell: torch.sqrt alone would give nan there"""
    Xn = paths(3, 6, 2, 0)
    sigma = 0.7
    for static in statics(kind, sigma):
        X = torch.as_tensor(Xn).requires_grad_(True)
        Xd = X.detach()
        (g,) = torch.autograd.grad(static.Gram_matrix(X, Xd).sum(), X)
        diff = Xn[:, None, :, None, :] - Xn[None, :, None, :, :]
        slope = MR.neg_dphi(kind, (diff * diff).sum(-1) / sigma)
        ref = (-2.0 / sigma) * (slope[..., None] * diff).sum(axis=(1, 3))  # dk/dx = -2/sigma (-phi') (x - y)
        assert torch.isfinite(g).all() and rel_max(g.numpy(), ref) < 1e-12
    # a sigma that requires grad, on the torch form: finite too
    import sigsvgd_amd.sigkernel as sk

    s = torch.tensor(sigma, dtype=torch.float64, requires_grad=True)
    cls = sk.Matern32StaticKernel if kind == MR.MATERN32 else sk.Matern52StaticKernel
    (gs,) = torch.autograd.grad(cls(s).Gram_matrix(Xd, Xd).sum(), s)
    d2 = (diff * diff).sum(-1)
    assert torch.isfinite(gs) and abs(float(gs) - float((slope * d2).sum() / sigma**2)) < 1e-10 * abs(float(gs))


# ---- 3. the C ABI, host only -------------------------------------------------------------------------------------------------
def query(name, *args):
    b = ctypes.c_size_t(12345)
    rc = getattr(lib(), "sigsvgd_" + name)(*args, ctypes.byref(b))
    return rc, b.value


@pytest.mark.parametrize("kind", KINDS)
def test_workspace_and_plan_queries_answer_as_for_imq_and_rq(kind):
    assert _lib.ABI_VERSION == 10 and lib().sigsvgd_abi_version() == 10 and len(_lib.EXPORTS) == 39
    for other in (IMQ, RQ):
        for shape in [(3, 4, 70, 66, 3, 0), (2, 3, 9, 12, 17, 2), (5, 5, 300, 300, 2, 0)]:
            A, _, TX, TY, d, n = shape
            for grad in (0, 1):
                got = query("gram_long_workspace_bytes", *shape, kind, grad, 0)
                assert got[0] == OK and got == query("gram_long_workspace_bytes", *shape, other, grad, 0)
                got = query("pair_workspace_bytes", A, TX, TY, d, n, kind, grad, 0)
                assert got[0] == OK and got == query("pair_workspace_bytes", A, TX, TY, d, n, other, grad, 0)
            for wx, wy in [(1, 1), (1, 0), (0, 0)]:
                got = query("gram_long2_workspace_bytes", *shape, kind, wx, wy, 0)
                assert got[0] == OK and got == query("gram_long2_workspace_bytes", *shape, other, wx, wy, 0)
                got = query("gram_long_h_workspace_bytes", *shape, kind, wx, wy, 0)
                assert got[0] == OK and got == query("gram_long_h_workspace_bytes", *shape, other, wx, wy, 0)
            got = query("pair_h_workspace_bytes", A, TX, TY, d, n, kind, 0)
            assert got[0] == OK and got == query("pair_h_workspace_bytes", A, TX, TY, d, n, other, 0)
        for off in (0, 1):
            got = query("gram_long_partial_workspace_bytes", 12, 70, 3, 0, kind, _lib.FLAG_FOLD_TILES, off, 2)
            assert got[0] == OK and got == query("gram_long_partial_workspace_bytes", 12, 70, 3, 0, other, _lib.FLAG_FOLD_TILES, off, 2)
        for shape in [(5, 6, 4, 2, 3), (5, 6, 20, 17, 0), (5, 6, 128, 14, 0), (64, 64, 6, 2, 0), (4, 4, 64, 7, 0)]:
            for grad in (0, 1):
                for flags in (0, _lib.FLAG_Y_IS_X, NAIVE, _lib.FLAG_FORCE_GENERIC):
                    got = query("gram_workspace_bytes", *shape, kind, grad, flags)
                    assert got[0] == OK and got == query("gram_workspace_bytes", *shape, other, grad, flags)
    r, c, r2, c2 = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    assert lib().sigsvgd_gram_long_partial_plan(12, 70, 3, 0, kind, 0, 2, ctypes.byref(r), ctypes.byref(c)) == OK
    assert lib().sigsvgd_gram_long_partial_plan(12, 70, 3, 0, IMQ, 0, 2, ctypes.byref(r2), ctypes.byref(c2)) == OK
    assert (r.value, c.value) == (r2.value, c2.value) and r.value > 0
    w, g, lds = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    assert lib().sigsvgd_pair_schedule(5, 322, 300, 3, 0, kind, 1, 0, ctypes.byref(w), ctypes.byref(g), ctypes.byref(lds)) == OK
    assert ops.pair_schedule(5, 322, 300, 3, 0, kind) == ops.pair_schedule(5, 322, 300, 3, 0, IMQ)


@pytest.mark.parametrize("kind", KINDS)
def test_naive_solver_is_unsupported_on_the_long_route(kind):
    for name, args in [("gram_long_workspace_bytes", (3, 4, 70, 66, 3, 0, kind, 1, NAIVE)),
                       ("pair_workspace_bytes", (3, 70, 66, 3, 0, kind, 1, NAIVE)),
                       ("gram_long2_workspace_bytes", (3, 4, 70, 66, 3, 0, kind, 1, 1, NAIVE)),
                       ("gram_long_h_workspace_bytes", (3, 4, 70, 66, 3, 0, kind, 1, 1, NAIVE)),
                       ("pair_h_workspace_bytes", (3, 70, 66, 3, 0, kind, NAIVE)),
                       ("gram_long_partial_workspace_bytes", (12, 70, 3, 0, kind, NAIVE, 0, 2))]:
        assert query(name, *args)[0] == UNSUPPORTED, name
        msg = _lib.last_error()
        assert "NAIVE_SOLVER" in msg and "default stencil only" in msg and "Matern" in msg, msg
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    assert lib().sigsvgd_gram_long_partial_plan(12, 70, 3, 0, kind, NAIVE, 2, ctypes.byref(r), ctypes.byref(c)) == UNSUPPORTED
    L = lib()
    assert L.sigsvgd_gram_long_fwd(FAKE, FAKE, 3, 4, 70, 66, 3, _lib.F64, 1.0, 0, kind, NAIVE, FAKE, None, 0, None) == UNSUPPORTED
    assert L.sigsvgd_gram_long_fwd_bwd(FAKE, FAKE, 3, 4, 70, 66, 3, _lib.F64, 1.0, 0, kind, NAIVE, None, FAKE, FAKE, None, 0,
                                       None) == UNSUPPORTED
    assert L.sigsvgd_pair_fwd(FAKE, FAKE, 3, 70, 66, 3, _lib.F64, 1.0, 0, kind, NAIVE, FAKE, None, 0, None) == UNSUPPORTED
    assert L.sigsvgd_gram_long_fwd_bwd2(FAKE, FAKE, 3, 4, 70, 66, 3, _lib.F64, 1.0, 0, kind, NAIVE, None, FAKE, FAKE, FAKE, None,
                                        0, None) == UNSUPPORTED
    assert L.sigsvgd_gram_long_fwd_bwd_h(FAKE, FAKE, 3, 4, 70, 66, 3, _lib.F64, 1.0, 0, kind, NAIVE, None, FAKE, FAKE, FAKE, FAKE,
                                         None, 0, None) == UNSUPPORTED
    assert L.sigsvgd_pair_fwd_bwd_h(FAKE, FAKE, 3, 70, 66, 3, _lib.F64, 1.0, 0, kind, NAIVE, None, FAKE, FAKE, FAKE, FAKE, None, 0,
                                    None) == UNSUPPORTED
    assert L.sigsvgd_gram_long_sym_partial(FAKE, 12, 70, 3, _lib.F64, 1.0, 0, kind, NAIVE, 0, 2, None, FAKE, FAKE, None, 0,
                                           None) == UNSUPPORTED
    assert "default stencil only" in _lib.last_error()
    # the coverage kernel has the first-order solver for every kind
    assert query("gram_workspace_bytes", 5, 6, 20, 3, 0, kind, 1, NAIVE)[0] == OK


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("inv_h", [0.0, -1.0, float("nan")])
def test_bandwidth_must_be_positive(kind, inv_h):
    L = lib()
    calls = [
        lambda: L.sigsvgd_gram_fwd(FAKE, FAKE, 4, 4, 64, 7, _lib.F64, inv_h, 0, kind, 0, FAKE, None, 0, None),
        lambda: L.sigsvgd_gram_fwd_bwd(FAKE, FAKE, 4, 4, 64, 7, _lib.F64, inv_h, 0, kind, 0, None, FAKE, FAKE, None, 0, None),
        lambda: L.sigsvgd_gram_long_fwd(FAKE, FAKE, 3, 4, 70, 66, 3, _lib.F64, inv_h, 0, kind, 0, FAKE, None, 0, None),
        lambda: L.sigsvgd_gram_long_fwd_bwd(FAKE, FAKE, 3, 4, 70, 66, 3, _lib.F64, inv_h, 0, kind, 0, None, FAKE, FAKE, None, 0,
                                            None),
        lambda: L.sigsvgd_pair_fwd_bwd(FAKE, FAKE, 3, 70, 66, 3, _lib.F64, inv_h, 0, kind, 0, None, FAKE, FAKE, FAKE, None, 0,
                                       None),
        lambda: L.sigsvgd_gram_long_fwd_bwd2(FAKE, FAKE, 3, 4, 70, 66, 3, _lib.F64, inv_h, 0, kind, 0, None, FAKE, FAKE, FAKE,
                                             None, 0, None),
        lambda: L.sigsvgd_gram_long_sym_partial(FAKE, 12, 70, 3, _lib.F64, inv_h, 0, kind, 0, 0, 2, None, FAKE, FAKE, None, 0,
                                                None),
        lambda: L.sigsvgd_gram_long_fwd_bwd_h(FAKE, FAKE, 3, 4, 70, 66, 3, _lib.F64, inv_h, 0, kind, 0, None, FAKE, FAKE, FAKE,
                                              FAKE, None, 0, None),
        lambda: L.sigsvgd_pair_fwd_bwd_h(FAKE, FAKE, 3, 70, 66, 3, _lib.F64, inv_h, 0, kind, 0, None, FAKE, FAKE, FAKE, FAKE, None,
                                         0, None),
    ]
    for call in calls:
        assert call() == BADARG
        assert "inv_h > 0" in _lib.last_error() and "Matern" in _lib.last_error()


@pytest.mark.parametrize("kind", KINDS)
def test_fused_partial_solve_refuses(kind):
    rc = lib().sigsvgd_gram_sym_partial(FAKE, 16, 64, 7, _lib.F32, 1.0, kind, 0, 0, 2, None, FAKE, FAKE, None, 0, None)
    assert rc == UNSUPPORTED and "RBF" in _lib.last_error()


@pytest.mark.parametrize("kind", KINDS)
def test_takes_queries_answer_as_for_the_linear_kernel(kind):
    assert ops.gram_takes(4, 4, 64, 7, 0, static_kind=kind) is True
    assert ops.gram_takes(4, 4, 4000, 3, 0, static_kind=kind) is False
    for shape in [(4, 4, 64, 7, 0), (4, 4, 4000, 3, 0), (5, 6, 20, 17, 0), (5, 6, 10, 3, 2), (3, 3, 300, 2, 0), (2, 2, 200, 4, 2),
                  (64, 64, 6, 2, 0)]:
        for grad in (False, True):
            assert ops.gram_takes(*shape, static_kind=kind, want_grad=grad) == ops.gram_takes(*shape, static_kind=LINEAR, want_grad=grad)
    for shape in [(3, 4, 70, 66, 3, 0), (2, 3, 9, 12, 17, 2), (2, 2, 9000, 9000, 2, 0), (2, 2, 300, 300, 2, 6)]:
        assert ops.gram_long2_takes(*shape, static_kind=kind) == ops.gram_long2_takes(*shape, static_kind=LINEAR)
        A, _, TX, TY, d, n = shape
        assert ops.pair_takes(A, TX, TY, d, n, static_kind=kind) == ops.pair_takes(A, TX, TY, d, n, static_kind=LINEAR)
        assert ops.gram_long_h_takes(*shape, static_kind=kind) == ops.gram_long_h_takes(*shape, static_kind=RBF)
        assert ops.pair_h_takes(A, TX, TY, d, n, static_kind=kind) == ops.pair_h_takes(A, TX, TY, d, n, static_kind=RBF)
    assert ops.gram_long2_takes(3, 4, 70, 66, 3, 0, static_kind=kind) and not ops.gram_long2_takes(2, 2, 9000, 9000, 2, 0, static_kind=kind)
    for shape in [(12, 70, 3, 0), (10, 20, 2, 2), (4, 9000, 2, 0)]:
        for world in (1, 2, 3):
            assert (ops.gram_long_partial_takes(*shape, static_kind=kind, tile_stride=world)
                    == ops.gram_long_partial_takes(*shape, static_kind=LINEAR, tile_stride=world))
    assert ops.gram_long_partial_takes(12, 70, 3, 0, static_kind=kind, tile_stride=2)


# ---- 4. the Python surface ---------------------------------------------------------------------------------------------------
def test_signature_kernel_by_name():
    from sigsvgd_amd import kernels

    for name, cls, kind in [("matern32", kernels.BatchMatern32Kernel, 6), ("Matern52", kernels.BatchMatern52Kernel, 7)]:
        k = kernels.SignatureKernel(lambda _: 0.5, depth=1, static_kernel=name)
        assert type(k.kernel.static_kernel) is cls and k.kernel.static_kernel.static_kind == kind
        assert k.kernel.static_kernel.inv_bandwidth(torch.zeros(2, 3, 2), torch.zeros(2, 3, 2)) == 2.0  # (no distances formed)
    assert "BatchMatern32Kernel" in kernels.__all__ and "BatchMatern52Kernel" in kernels.__all__
    with pytest.raises(ValueError):
        kernels.SignatureKernel(static_kernel="matern12")


def test_learned_sigma_is_recognised():
    import sigsvgd_amd.sigkernel as sk

    assert "Matern32StaticKernel" in sk.__all__ and "Matern52StaticKernel" in sk.__all__
    for cls in (sk.Matern32StaticKernel, sk.Matern52StaticKernel):
        s = torch.tensor(1.3, dtype=torch.float64, requires_grad=True)
        assert sk._learned_sigma(cls(s)) is s
        assert sk._learned_sigma(cls(1.3)) is None and sk._learned_sigma(cls(torch.tensor(1.3))) is None
        with torch.no_grad():
            assert sk._learned_sigma(cls(s)) is None
        assert sk._resolve_static(cls(s), None, None) == (cls.static_kind, 1.0 / 1.3)
        with pytest.raises(ValueError):
            sk._learned_sigma(cls(torch.ones(2, requires_grad=True)))


def test_sharded_routes(monkeypatch):
    """ShardedSigSVGD's route for kinds 6 and 7, as tests/test_static_kinds_cabi.py holds it for kinds 2 and 3: never the fused
    partial solve; row-wise where the coverage kernel takes the rows, the long partial solve where it does not; and the
    row-wise solver of a shape only the long route takes is ops.gram_long_fwd_bwd."""
    from sigsvgd_amd.distributed import ShardedSigSVGD

    for kind in KINDS:
        sh = ShardedSigSVGD(1.0, 0.1, static_kind=kind)
        assert sh._route_of(8, torch.zeros(8, 64, 7), 1) == "rowwise"
        assert sh._route_of(8, torch.zeros(8, 300, 2), 1) == "long_partial"
        assert ShardedSigSVGD(1.0, 0.1, static_kind=kind, long_partial=False)._route_of(8, torch.zeros(8, 300, 2), 1) == "rowwise"
        calls = []
        monkeypatch.setattr(ops, "gram_fwd_bwd", lambda *a, **k: calls.append(("fused", a[3:])))
        monkeypatch.setattr(ops, "gram_long_fwd_bwd", lambda *a, **k: calls.append(("long", a[3:])))
        sh.rows_fn(torch.zeros(4, 64, 7), torch.zeros(8, 64, 7), 1.0)
        sh.rows_fn(torch.zeros(4, 300, 2), torch.zeros(8, 300, 2), 1.0)
        assert calls == [("fused", (0, kind)), ("long", (0, kind))]
