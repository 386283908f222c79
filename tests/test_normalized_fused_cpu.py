"""The normalised kernel on the fused Gram route (SIGSVGD_FLAG_NORMALIZED_FUSED) without a device:
(a) the pipeline's algebra, restated on the plain oracle in tests/normalized_fused_reference.py, against the yardstick of the
GPU tests, `log_k_reference.normalized_gram_and_grads`; (b) the host side of the C ABI: the bit, the workspace query, every
refusal before any device work; (c) which launches `SigKernel(..., normalize=True, normalize_route="fused")` and
`kernels.SignatureKernel` issue, with a recorder over `ops` in the style of tests/test_normalized_cpu.py.

On a library without the feature the fused entry points ignore bit 4096 (the flagged query equals the unflagged one, nothing
is refused) and `normalize_route=` is a TypeError: (b) and (c) fail."""
import ctypes

import numpy as np
import pytest
import torch

import log_k_reference as R
import normalized_fused_reference as NF
import sigsvgd_amd.sigkernel as sk
from cabi import BADARG, FAKE, OK, UNSUPPORTED, WORKSPACE, exported_symbols, lib
from sigsvgd_amd import _lib, ops

NF_BIT, NM, LK, EX, NV, YX, SYM = (4096, _lib.FLAG_NORMALIZED, _lib.FLAG_LOG_K, _lib.FLAG_EXACT_ADJOINT, _lib.FLAG_NAIVE_SOLVER,
                                   _lib.FLAG_Y_IS_X, _lib.FLAG_SYM)
NAME = "SIGSVGD_FLAG_NORMALIZED_FUSED"


def _ws(name, *args):
    b = ctypes.c_size_t(12345)
    rc = getattr(lib(), "sigsvgd_" + name)(*args, ctypes.byref(b))
    return rc, b.value


# ---- (a) the algebra ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 2])
@pytest.mark.parametrize("mode", ["ordered", "sym", "yx", "yx_sym"])
def test_the_restatement_equals_the_log_domain_reference(mode, n):
    """A = 4, B = 3 (A = B = 4 where the mode needs one shape), T = 8, d = 2: K^, the gradient and its two terms to 1e-10 of
    the largest entry.  Under Y_IS_X the yardstick gets the diagonal weights set to zero, as tests/test_gpu_normalized.py does."""
    yx, sym = mode.startswith("yx"), mode.endswith("sym")
    A, B = (4, 4) if (yx or sym) else (4, 3)
    X = R.walks(5, A, 8, 2, 0.5)
    Y = X.copy() if yx else R.walks(6, B, 8, 2, 0.5)
    w = np.random.default_rng(7).standard_normal((A, B))
    w[0, B - 1] = 0.0
    Khat, g, t1, t2 = NF.gram_and_grad(X, Y, w, R.RBF, 1.0, n, sym, yx)
    wr = w + w.T if sym else w
    if yx:
        wr = wr - np.diag(np.diag(wr))
    Kref, gref, _ = R.normalized_gram_and_grads(X, Y, wr, R.RBF, 1.0, n)
    assert (Kref > 0).all() and np.isfinite(gref).all()
    assert np.abs(Khat - Kref).max() < 1e-10 * np.abs(Kref).max()
    assert np.abs(g - gref).max() < 1e-10 * np.abs(gref).max()
    r1, r2 = NF.terms(X, Y, w, R.RBF, 1.0, n, sym, yx)
    assert np.abs(t1 - r1).max() < 1e-10 * np.abs(r1).max() and np.abs(t2 - r2).max() < 1e-10 * np.abs(r2).max()
    assert np.abs((r1 - r2) - gref).max() < 1e-10 * np.abs(gref).max()
    if yx:
        assert (np.diag(Khat) == 1.0).all()


# ---- (b) the host side of the C ABI -------------------------------------------------------------------------------------------------
def test_the_bit_is_4096_and_the_abi_is_still_version_10_with_39_exports():
    assert lib().sigsvgd_abi_version() == _lib.ABI_VERSION == 10
    assert len(exported_symbols()) == len(_lib.EXPORTS) == 39
    assert _lib.FLAG_NORMALIZED_FUSED == NF_BIT == 4096
    assert ops._flags(False, False, False, False, normalized_fused=True) == 4096
    assert ops._flags(False, True, True, False, normalized_fused=True) == 2 | 4 | 4096
    assert ops._flags(False, False, False, False, normalized=True) == 2048
    assert ops._flags(False, False, False, False) == 0


@pytest.mark.parametrize("A,B,T,d,n", [(8, 8, 32, 2, 0), (5, 9, 65, 3, 0), (3, 3, 10, 2, 4)])
def test_flagged_workspace_is_the_unflagged_one_plus_its_pieces(A, B, T, d, n):
    """ordered, Y_IS_X and forward-only queries: the unflagged bytes, the logarithms, the diagonal pass's scratch (the paired
    log-domain query's bytes) and, for a gradient launch, W' (counted here in the smaller I/O type), the fp64 diagonal gradients
    and the sums, each padded to 256 B"""
    pad = lambda b: (b + 255) & ~255
    for f in (0, YX, SYM, YX | SYM):
        if f and A != B:
            continue
        for grad in (1, 0):
            rc0, b0 = _ws("gram_workspace_bytes", A, B, T, d, n, 0, grad, f)
            rc1, b1 = _ws("gram_workspace_bytes", A, B, T, d, n, 0, grad, f | NF_BIT)
            rcp, scratch = _ws("pair_workspace_bytes", A, T, T, d, n, 0, grad, LK)
            assert rc0 == OK and rc1 == OK and rcp == OK and scratch > 0, _lib.last_error()
            least = pad(8 * (A + (0 if f & YX else B))) + scratch
            if grad:
                least += pad(4 * A * B) + pad(8 * A * T * d) + pad(8 * A)
            assert b1 >= b0 + least, (f, grad, b0, b1, least)
    # every kind and both orientations of the query are taken
    for kind in (0, 1, 2, 3, 6, 7):
        assert _ws("gram_workspace_bytes", A, B, T, d, n, kind, 1, NF_BIT)[0] == OK, _lib.last_error()


def test_a_launch_without_its_workspace_is_refused_before_any_device_work():
    L = lib()
    for f in (0, YX, YX | SYM):
        geo = (6, 6, 20, 3, _lib.F32, 1.0, 0, 0, NF_BIT | f)
        assert L.sigsvgd_gram_fwd(FAKE, FAKE, *geo, FAKE, None, 0, None) == WORKSPACE, _lib.last_error()
        assert L.sigsvgd_gram_fwd_bwd(FAKE, FAKE, *geo, None, FAKE, FAKE, FAKE, 256, None) == WORKSPACE, _lib.last_error()
        assert "required" in _lib.last_error()


def test_naive_solver_with_the_bit_is_unsupported_and_names_both_flags():
    L = lib()
    geo = (6, 6, 20, 3, _lib.F32, 1.0, 0, 0, NF_BIT | NV)
    calls = [lambda: L.sigsvgd_gram_fwd(FAKE, FAKE, *geo, FAKE, FAKE, 1 << 30, None),
             lambda: L.sigsvgd_gram_fwd_bwd(FAKE, FAKE, *geo, None, FAKE, FAKE, FAKE, 1 << 30, None),
             lambda: _ws("gram_workspace_bytes", 6, 6, 20, 3, 0, 0, 1, NF_BIT | NV)[0],
             lambda: _ws("gram_workspace_bytes", 6, 6, 20, 3, 0, 0, 0, NF_BIT | NV)[0]]
    for k, call in enumerate(calls):
        assert call() == UNSUPPORTED, (k, _lib.last_error())
        assert NAME in _lib.last_error() and "SIGSVGD_FLAG_NAIVE_SOLVER" in _lib.last_error(), (k, _lib.last_error())
    # the exact adjoint keeps the answer it has on these entry points
    assert _ws("gram_workspace_bytes", 6, 6, 20, 3, 0, 0, 1, NF_BIT | EX)[0] == UNSUPPORTED
    assert "SIGSVGD_FLAG_EXACT_ADJOINT" in _lib.last_error()
    geo = (6, 6, 20, 3, _lib.F32, 1.0, 0, 0, NF_BIT | EX)
    assert L.sigsvgd_gram_fwd_bwd(FAKE, FAKE, *geo, None, FAKE, FAKE, FAKE, 1 << 30, None) == UNSUPPORTED
    assert "SIGSVGD_FLAG_EXACT_ADJOINT" in _lib.last_error()


def test_the_partial_solve_refuses_the_bit_by_name():
    rc = lib().sigsvgd_gram_sym_partial(FAKE, 16, 20, 3, _lib.F32, 1.0, 0, NF_BIT, 0, 2, None, FAKE, FAKE, FAKE, 1 << 30, None)
    assert rc == UNSUPPORTED and NAME in _lib.last_error(), _lib.last_error()


def test_a_shape_whose_diagonal_pass_the_paired_plan_refuses_is_refused_as_a_whole():
    """(the fused kernels refuse such shapes themselves long before the paired plan does; the refusal is the first one met)"""
    assert _ws("gram_workspace_bytes", 2, 2, 9000, 2, 0, 0, 1, NF_BIT)[0] == UNSUPPORTED
    assert ops.gram_takes(2, 2, 9000, 2, normalized=True) is False


def test_long_route_pde_and_select_entry_points_answer_badarg_for_4096():
    L = lib()
    A, B, TX, TY, d, n = 3, 3, 300, 300, 2, 0
    geo = (A, B, TX, TY, d, _lib.F64, 1.0, n, 0, NF_BIT)
    pgeo = (A, TX, TY, d, _lib.F64, 1.0, n, 0, NF_BIT)
    two = (A, B, TX, TY, d, n, 0)
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    w, grid, lds = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    calls = [
        lambda: L.sigsvgd_gram_long_fwd(FAKE, FAKE, *geo, FAKE, FAKE, 1 << 30, None),
        lambda: L.sigsvgd_gram_long_fwd_bwd(FAKE, FAKE, *geo, None, FAKE, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("gram_long_workspace_bytes", *two, 1, NF_BIT)[0],
        lambda: L.sigsvgd_gram_long_fwd_bwd2(FAKE, FAKE, *geo, None, FAKE, FAKE, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("gram_long2_workspace_bytes", *two, 1, 1, NF_BIT)[0],
        lambda: _ws("gram_long2_workspace_bytes", *two, 1, 1, NF_BIT | NM)[0],
        lambda: L.sigsvgd_gram_long_fwd_bwd_h(FAKE, FAKE, *geo, None, FAKE, FAKE, None, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("gram_long_h_workspace_bytes", *two, 1, 0, NF_BIT)[0],
        lambda: L.sigsvgd_pair_fwd(FAKE, FAKE, *pgeo, FAKE, FAKE, 1 << 30, None),
        lambda: L.sigsvgd_pair_fwd_bwd(FAKE, FAKE, *pgeo, None, FAKE, FAKE, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("pair_workspace_bytes", A, TX, TY, d, n, 0, 1, NF_BIT)[0],
        lambda: L.sigsvgd_pair_schedule(A, TX, TY, d, n, 0, 1, NF_BIT, ctypes.byref(w), ctypes.byref(grid), ctypes.byref(lds)),
        lambda: L.sigsvgd_pair_fwd_bwd_h(FAKE, FAKE, *pgeo, None, FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("pair_h_workspace_bytes", A, TX, TY, d, n, 0, NF_BIT)[0],
        lambda: L.sigsvgd_gram_long_sym_partial(FAKE, 64, 300, 2, _lib.F64, 1.0, 0, 0, NF_BIT, 0, 2, None, FAKE, FAKE, FAKE,
                                                1 << 30, None),
        lambda: L.sigsvgd_gram_long_partial_plan(64, 300, 2, 0, 0, NF_BIT, 2, ctypes.byref(r), ctypes.byref(c)),
        lambda: _ws("gram_long_partial_workspace_bytes", 64, 300, 2, 0, 0, NF_BIT, 0, 2)[0],
        lambda: _ws("pde_workspace_bytes", 4, 30, 20, 1, 1, NF_BIT)[0],
        lambda: L.sigsvgd_pde_fwd(FAKE, 4, 30, 20, _lib.F64, 1, NF_BIT, FAKE, FAKE, 1 << 30, None),
        lambda: L.sigsvgd_pde_fwd_bwd(FAKE, 4, 30, 20, _lib.F64, 1, NF_BIT, None, FAKE, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("sqdist_select_workspace_bytes", 4, 4, 9, 9, 2, NF_BIT)[0],
    ]
    for k, call in enumerate(calls):
        assert call() == BADARG, (k, _lib.last_error())
        assert "0x1000" in _lib.last_error(), (k, _lib.last_error())
    # bit 2048 stays the ignored bit it was on the fused query
    assert _ws("gram_workspace_bytes", 8, 8, 32, 2, 0, 0, 1, NM) == _ws("gram_workspace_bytes", 8, 8, 32, 2, 0, 0, 1, 0)


# ---- (c) the Python layer ------------------------------------------------------------------------------------------------------------
A, B, T, TY, D = 5, 4, 6, 5, 2
NKW = {"normalized": True}


class Recorder:
    """stands in for the launches and queries of `ops` a call on the fused route may reach; every other launch raises"""

    def __init__(self, takes=True):
        self.takes, self.launches, self.queries = takes, [], []

    def gram_takes(self, A, B, T, d, dyadic_order=0, static_kind=0, want_grad=True, naive=False, sym=False, y_is_x=False, **kw):
        self.queries.append(("gram_takes", (A, B, T, d), bool(want_grad), bool(sym), bool(y_is_x), dict(kw)))
        return self.takes

    def gram_fwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, naive=False, force_generic=False, y_is_x=False, **kw):
        self.launches.append(("gram_fwd", tuple(X.shape), tuple(Y.shape), X.data_ptr() == Y.data_ptr(),
                              "yx" if y_is_x else "", dict(kw), None))
        return torch.full((X.shape[0], Y.shape[0]), 0.5, dtype=X.dtype)

    def gram_fwd_bwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False, y_is_x=False,
                     force_generic=False, **kw):
        flags = dict(naive=naive, sym=sym, yx=y_is_x, w=grad_out is not None)
        self.launches.append(("gram_fwd_bwd", tuple(X.shape), tuple(Y.shape), X.data_ptr() == Y.data_ptr(),
                              " ".join(k for k, v in flags.items() if v), dict(kw),
                              None if grad_out is None else grad_out.clone()))
        return torch.full((X.shape[0], Y.shape[0]), 0.5, dtype=X.dtype), 2 * torch.ones_like(X)

    def svgd_phi(self, K, score, grad_k, **kw):
        self.launches.append(("svgd_phi", tuple(K.shape), tuple(grad_k.shape)))
        return torch.zeros_like(score)

    def install(self, monkeypatch):
        def refuse(name):
            def f(*a, **k):
                raise AssertionError(f"ops.{name} reached by a call on the fused route")
            return f

        for name in ("gram_long_fwd", "gram_long_fwd_bwd", "gram_long_fwd_bwd2", "gram_long2_takes", "gram_long_fwd_bwd_h",
                     "pair_fwd", "pair_fwd_bwd", "pair_takes", "pair_fwd_bwd_h", "path_sqdist_select", "pde_fwd_bwd"):
            monkeypatch.setattr(ops, name, refuse(name))
        for name in ("gram_takes", "gram_fwd", "gram_fwd_bwd", "svgd_phi"):
            monkeypatch.setattr(ops, name, getattr(self, name))
        return self


def paths(n, t, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, t, D, dtype=torch.float64, generator=g)


def brief(rec):
    return [c[:6] for c in rec.launches]


def fused(static=None, order=0, **kw):
    return sk.SigKernel(static or sk.RBFKernel(1.0), order, normalize=True, normalize_route="fused", **kw)


def test_gram_and_grad_issues_exactly_one_flagged_fused_launch(monkeypatch):
    rec = Recorder().install(monkeypatch)
    kernel = fused()
    X, Y = paths(A, T), paths(B, TY, 1)
    sx, sy = (A, T, D), (B, TY, D)
    K, g = kernel.gram_and_grad(X)
    assert brief(rec) == [("gram_fwd_bwd", sx, sx, True, "yx", NKW)]
    assert rec.queries == [("gram_takes", (A, A, T, D), True, False, True, NKW)]
    assert torch.equal(K, torch.full((A, A), 0.5).double()) and torch.equal(g, 2 * torch.ones_like(X))  # handed back as they are
    G = torch.arange(1.0, A * A + 1).reshape(A, A).double()
    rec.launches.clear()
    kernel.gram_and_grad(X, None, G, sym=True)
    assert brief(rec) == [("gram_fwd_bwd", sx, sx, True, "sym yx w", NKW)] and torch.equal(rec.launches[0][6], G)
    rec.launches.clear()
    K, g = kernel.gram_and_grad(X, Y, G[:, :B])
    assert brief(rec) == [("gram_fwd_bwd", sx, sy, False, "w", NKW)] and K.shape == (A, B) and g.shape == X.shape
    rec.launches.clear()
    sk.gram_and_grad(kernel, X)  # the module-level function
    assert brief(rec) == [("gram_fwd_bwd", sx, sx, True, "yx", NKW)]
    # every kind and order the constructor takes; fp32_sweeps means what it means without normalize
    rec.launches.clear()
    fused(sk.IMQStaticKernel(2.0), 2).gram_and_grad(X)
    fused(sk.IMQStaticKernel(2.0), 0, fp32_sweeps=True).gram_and_grad(X)
    assert brief(rec) == [("gram_fwd_bwd", sx, sx, True, "yx", NKW),
                          ("gram_fwd_bwd", sx, sx, True, "yx", {"normalized": True, "fp32_sweeps": True})]


def test_compute_gram_is_a_node_of_the_two_flagged_launches_and_mmd_follows(monkeypatch):
    rec = Recorder().install(monkeypatch)
    kernel = fused()
    X, Y = paths(A, T).requires_grad_(True), paths(B, T, 1)
    sx, sy = (A, T, D), (B, T, D)
    K = kernel.compute_Gram(X, Y)
    assert brief(rec) == [("gram_fwd", sx, sy, False, "", NKW)]
    G = torch.arange(1.0, A * B + 1).reshape(A, B).double()
    (g,) = torch.autograd.grad((G * K).sum(), X)
    assert brief(rec)[1:] == [("gram_fwd_bwd", sx, sy, False, "w", NKW)] and torch.equal(rec.launches[1][6], G)
    assert torch.equal(g, 2 * torch.ones_like(X))
    rec.launches.clear()
    K = kernel.compute_Gram(X, X, sym=True)  # one tensor in both slots: Y_IS_X, and sym as it means today
    K.sum().backward()
    assert brief(rec) == [("gram_fwd", sx, sx, True, "yx", NKW), ("gram_fwd_bwd", sx, sx, True, "sym yx w", NKW)]
    rec.launches.clear()
    with torch.no_grad():
        kernel.compute_mmd(X, Y)
    assert [c[:5] for c in rec.launches] == [("gram_fwd", sx, sx, True, "yx"), ("gram_fwd", sy, sy, True, "yx"),
                                             ("gram_fwd", sx, sy, False, "")]
    assert all(c[5] == NKW for c in rec.launches)


def test_signature_kernel_hands_the_route_on_and_an_svgd_step_issues_the_launch(monkeypatch):
    from sigsvgd_amd.inference import SVGD
    from sigsvgd_amd.kernels import SignatureKernel

    rec = Recorder().install(monkeypatch)
    kernel = SignatureKernel(depth=0, static_kernel=sk.RBFKernel(1.0), normalize=True, normalize_route="fused")
    assert kernel.kernel.normalize is True and kernel.kernel.normalize_route == "fused"
    assert SignatureKernel(depth=0, static_kernel=sk.RBFKernel(1.0), normalize=True).kernel.normalize_route == "long"
    X = paths(A, T)
    sx = (A, T, D)
    svgd = SVGD(kernel, optimizer_class=None, lr=0.1)
    X1, info = svgd.step(X, grad_log_p=torch.ones_like(X))
    assert rec.launches[0][:6] == ("gram_fwd_bwd", sx, sx, True, "yx", NKW)
    assert rec.launches[1:] == [("svgd_phi", (A, A), (A, T * D))]
    assert torch.equal(info["k_xx"], torch.full((A, A), 0.5).double()) and X1.shape == X.shape


def test_the_default_route_issues_what_it_issued_before(monkeypatch):
    """normalize=True alone (route "long"): one `ops.gram_long_fwd_bwd2(..., normalized=True)`, through recorders with the
    signatures from before this route; normalize=False: `ops.gram_fwd_bwd` without any `normalized=`"""
    seen = []

    def gram_long2_takes(A, B, TX, TY, d, dyadic_order=0, static_kind=0, want_gradX=True, want_gradY=True, y_is_x=False,
                         exact_adjoint=False, nan_tails=False, log_k=False, normalized=False):
        return True

    def gram_long_fwd_bwd2(X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False, y_is_x=False,
                           want_gradX=True, want_gradY=True, exact_adjoint=False, nan_tails=False, log_k=False, normalized=False):
        seen.append(("gram_long_fwd_bwd2", y_is_x, normalized))
        return torch.zeros(X.shape[0], Y.shape[0], dtype=X.dtype), torch.zeros_like(X), None

    def gram_takes(A, B, T, d, dyadic_order=0, static_kind=0, want_grad=True, naive=False, sym=False, y_is_x=False,
                   fp32_sweeps=False):
        return True

    def gram_fwd_bwd(X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False, y_is_x=False,
                     force_generic=False, check_regime=True, stored_forward=False, fp32_sweeps=False):
        seen.append(("gram_fwd_bwd", sym, y_is_x))
        return torch.zeros(X.shape[0], Y.shape[0], dtype=X.dtype), torch.zeros_like(X)

    for f in (gram_long2_takes, gram_long_fwd_bwd2, gram_takes, gram_fwd_bwd):
        monkeypatch.setattr(ops, f.__name__, f)
    X = paths(A, T)
    sk.SigKernel(sk.RBFKernel(1.0), 0, normalize=True).gram_and_grad(X)
    sk.SigKernel(sk.RBFKernel(1.0), 0, normalize=True, normalize_route="long").gram_and_grad(X)
    sk.SigKernel(sk.RBFKernel(1.0), 0).gram_and_grad(X)
    assert seen == [("gram_long_fwd_bwd2", True, True)] * 2 + [("gram_fwd_bwd", False, True)]


def test_refusals_are_raised_before_any_launch(monkeypatch):
    from parity import DisguisedRBF

    rec = Recorder().install(monkeypatch)
    X, Y = paths(A, T), paths(B, TY, 1)
    with pytest.raises(ValueError, match="normalize=True"):
        sk.SigKernel(sk.RBFKernel(1.0), 0, normalize_route="fused")
    with pytest.raises(ValueError, match="normalize_route"):
        sk.SigKernel(sk.RBFKernel(1.0), 0, normalize=True, normalize_route="short")
    with pytest.raises(ValueError, match="fp32_sweeps"):  # (the default route keeps its answer)
        sk.SigKernel(sk.IMQStaticKernel(1.0), 0, fp32_sweeps=True, normalize=True)
    with pytest.raises(NotImplementedError, match="exact_grad"):
        fused(exact_grad=True)
    with pytest.raises(NotImplementedError, match="_naive_solver"):
        fused(_naive_solver=True)
    kernel = fused()
    with pytest.raises(NotImplementedError, match="grad_Y"):
        kernel.compute_Gram(X, Y, grad_Y=True)
    with pytest.raises(NotImplementedError, match="grad_Y"):
        kernel.compute_mmd(X, Y, grad_Y=True)
    for kw in (dict(lengths_X=[T] * A), dict(lengths_Y=[TY] * B)):
        with pytest.raises(NotImplementedError, match="lengths"):
            kernel.compute_Gram(X, Y, **kw)
    learned = fused(sk.RBFKernel(torch.tensor(1.0, requires_grad=True)))
    for call in (lambda: learned.gram_and_grad(X), lambda: learned.compute_Gram(X, Y)):
        with pytest.raises(NotImplementedError, match="sigma that requires grad"):
            call()
    user = fused(DisguisedRBF(1.0))
    for call in (lambda: user.gram_and_grad(X), lambda: user.compute_Gram(X, Y)):
        with pytest.raises(NotImplementedError, match="user static kernel"):
            call()
    assert rec.launches == [] and rec.queries == []
    # shapes gram_takes refuses: the library's message
    rec.takes = False
    monkeypatch.setattr(_lib, "last_error", lambda: "refused by the plan")
    for call in (lambda: kernel.gram_and_grad(X), lambda: kernel.compute_Gram(X, Y)):
        with pytest.raises(NotImplementedError, match="refused by the plan"):
            call()
    assert rec.launches == [] and len(rec.queries) == 2 and all(q[5] == NKW for q in rec.queries)


def test_compute_kernel_and_the_log_methods_keep_the_long_route(monkeypatch):
    seen = []

    def pair_takes(*a, **k):
        return True

    def pair_fwd(X, Y, inv_h, dyadic_order=0, static_kind=0, naive=False, **kw):
        seen.append(("pair_fwd", dict(kw)))
        return torch.zeros(X.shape[0], dtype=X.dtype)

    monkeypatch.setattr(ops, "pair_takes", pair_takes)
    monkeypatch.setattr(ops, "pair_fwd", pair_fwd)
    kernel = fused()
    X, Y = paths(A, T), paths(A, T, 1)
    kernel.compute_kernel(X, Y)
    kernel.compute_log_kernel(X, Y)
    assert seen == [("pair_fwd", {"log_k": True})] * 4
