"""The exact adjoint of the discrete signature kernel (SIGSVGD_FLAG_EXACT_ADJOINT) without a device:
the fp64 helper of tests/exact_adjoint_reference.py against central differences of its own K and against the oracle, the host
side of the C ABI (every acceptance and refusal of the flag returns before any device work), and where `exact_grad=True` goes
in the Python layer, with recorders in the style of tests/test_fp32_static_routing_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import exact_adjoint_reference as E
import sigsvgd_amd.sigkernel as sk
from cabi import BADARG, FAKE, OK, UNSUPPORTED, exported_symbols, lib
from oracle import sigkernel_oracle as O
from parity import rel_max
from sigsvgd_amd import _lib, ops

EX, NV = _lib.FLAG_EXACT_ADJOINT, _lib.FLAG_NAIVE_SOLVER


# ---- 1 - 3: the helper ---------------------------------------------------------------------------------------------------------
def rough_pair(M, N, d=2, seed=0, step=0.6):
    """one pair of fp64 random walks with steps of size `step` per channel: rough enough at bandwidth 1 that GG and the exact
    adjoint are per cents apart (test_default_stencil_is_not_gg), the regime the GPU cases use too"""
    rng = np.random.default_rng(seed + 1000 * M + N)
    return (np.cumsum(step * rng.standard_normal((1, M, d)), axis=1), np.cumsum(step * rng.standard_normal((1, N, d)), axis=1))


FD_SHAPES = [(6, 5, 0), (9, 7, 1), (20, 17, 2), (70, 66, 0)]


@pytest.mark.parametrize("M,N,n", FD_SHAPES)
def test_helper_matches_central_differences(M, N, n):
    X, Y = rough_pair(M, N)
    G = E.static_gram(X, Y, E.RBF, 1.0)[0, 0]
    _, S, _ = E.pde(G, n)
    fd = E.fd_dK_dD(O.increments(G), n)
    err_D = rel_max(S, fd)
    _, gX, _ = E.gram_backward(X, Y, None, E.RBF, 1.0, n)
    err_X = rel_max(gX, E.fd_dK_dX(X, Y, E.RBF, 1.0, n))
    print(f"M={M} N={N} n={n}: dK/dD {err_D:.2e}, dK/dX {err_X:.2e} of the largest entry")
    assert err_D < 1e-6 and err_X < 1e-6


@pytest.mark.parametrize("M,N,n", FD_SHAPES[:3])
@pytest.mark.parametrize("kind", [O.RBF, O.LINEAR])
def test_naive_stencil_is_the_oracles_gg(M, N, n, kind):
    """with the first-order stencil the recurrence is GG itself: the helper is tied to oracle/"""
    rng = np.random.default_rng(M)
    X, Y = rough_pair(M, N, seed=1)
    X, Y = np.repeat(X, 2, 0) + 0.1 * rng.standard_normal((2, M, 2)), np.repeat(Y, 3, 0) + 0.1 * rng.standard_normal((3, N, 2))
    if M != N:  # (the oracle's gram_backward takes one length)
        Y = np.concatenate([Y, np.repeat(Y[:, -1:], M - N, axis=1)], axis=1)
    w = rng.uniform(0.5, 1.5, (2, 3))
    Ko, go = O.gram_backward(X, Y, w, kind, 1.0, n, naive=True)
    K, gX, _ = E.gram_backward(X, Y, w, kind, 1.0, n, naive=True)
    assert rel_max(K, Ko) < 1e-13 and rel_max(gX, go) < 1e-12


@pytest.mark.parametrize("M,N,n", FD_SHAPES[1:])
def test_default_stencil_is_not_gg(M, N, n):
    """on the rough cases the GPU tests use, GG is more than 1e-2 of the largest entry away: a GG kernel cannot pass them"""
    X, Y = rough_pair(M, N)
    Y = np.concatenate([Y, np.repeat(Y[:, -1:], M - N, axis=1)], axis=1)
    _, go = O.gram_backward(X, Y, None, O.RBF, 1.0, n)
    _, gX, _ = E.gram_backward(X, Y, None, E.RBF, 1.0, n)
    assert rel_max(go, gX) > 1e-2


# ---- 4: the host side of the C ABI ---------------------------------------------------------------------------------------------
GEO = dict(A=3, B=3, TX=300, TY=200, d=2, n=0)


def _ws(name, *args):
    b = ctypes.c_size_t(12345)
    rc = getattr(lib(), "sigsvgd_" + name)(*args, ctypes.byref(b))
    return rc, b.value


def test_abi_is_version_10_with_39_exports():
    assert lib().sigsvgd_abi_version() == _lib.ABI_VERSION == 10
    assert len(exported_symbols()) == len(_lib.EXPORTS) == 39
    assert _lib.FLAG_EXACT_ADJOINT == 256
    assert ops._flags(True, True, True, True, True, True) == 1 | 2 | 4 | 8 | 32 | 128
    assert ops._flags(False, False, False, False, exact_adjoint=True) == 256
    assert ops._flags(False, True, False, False, fp32_sweeps=True, exact_adjoint=True) == 2 | 128 | 256


@pytest.mark.parametrize("extra", [0, NV])
def test_workspace_queries_accept_the_flag_with_equal_bytes(extra):
    g = GEO
    queries = [
        ("pde_workspace_bytes", (4, 30, 20, 1, 1)),
        ("gram_long_workspace_bytes", (g["A"], g["B"], g["TX"], g["TY"], g["d"], g["n"], 0, 1)),
        ("pair_workspace_bytes", (g["A"], g["TX"], g["TY"], g["d"], g["n"], 0, 1)),
        ("gram_long2_workspace_bytes", (g["A"], g["B"], g["TX"], g["TY"], g["d"], g["n"], 0, 1, 1)),
        ("gram_long2_workspace_bytes", (g["A"], g["B"], g["TX"], g["TY"], g["d"], g["n"], 0, 0, 1)),
        ("gram_long_h_workspace_bytes", (g["A"], g["B"], g["TX"], g["TY"], g["d"], g["n"], 0, 1, 1)),
        ("gram_long_h_workspace_bytes", (g["A"], g["B"], g["TX"], g["TY"], g["d"], g["n"], 0, 0, 0)),
        ("pair_h_workspace_bytes", (g["A"], g["TX"], g["TY"], g["d"], g["n"], 0)),
    ]
    for name, args in queries:
        rc0, b0 = _ws(name, *args, extra)
        rc1, b1 = _ws(name, *args, extra | EX)
        assert rc0 == OK and rc1 == OK, (name, _lib.last_error())
        assert b0 == b1 and b0 > 0, name


def test_forward_only_queries_and_launches_refuse_the_flag():
    g = GEO
    L = lib()
    assert _ws("pde_workspace_bytes", 4, 30, 20, 1, 0, EX)[0] == BADARG
    assert _ws("gram_long_workspace_bytes", g["A"], g["B"], g["TX"], g["TY"], g["d"], g["n"], 0, 0, EX)[0] == BADARG
    assert _ws("pair_workspace_bytes", g["A"], g["TX"], g["TY"], g["d"], g["n"], 0, 0, EX)[0] == BADARG
    assert _ws("gram_long2_workspace_bytes", g["A"], g["B"], g["TX"], g["TY"], g["d"], g["n"], 0, 0, 0, EX)[0] == BADARG
    assert L.sigsvgd_pde_fwd(FAKE, 4, 30, 20, _lib.F64, 1, EX, FAKE, FAKE, 1 << 30, None) == BADARG
    assert "0x100" in _lib.last_error()
    geo = (g["A"], g["B"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, EX)
    assert L.sigsvgd_gram_long_fwd(FAKE, FAKE, *geo, FAKE, FAKE, 1 << 30, None) == BADARG
    assert "0x100" in _lib.last_error()
    pgeo = (g["A"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, EX)
    assert L.sigsvgd_pair_fwd(FAKE, FAKE, *pgeo, FAKE, FAKE, 1 << 30, None) == BADARG
    assert "0x100" in _lib.last_error()
    # the two-sided launch without a gradient output is forward only
    assert L.sigsvgd_gram_long_fwd_bwd2(FAKE, FAKE, *geo, None, FAKE, None, None, FAKE, 1 << 30, None) == BADARG


def test_gradient_launches_take_the_flag():
    """every gradient entry point passes its flag check with the bit: the refusal it then gives is the next check's (a
    workspace of 0 bytes, before any device work), not BADARG"""
    g = GEO
    L = lib()
    WS = _lib.E_WORKSPACE
    for flags in (EX, EX | NV):
        assert L.sigsvgd_pde_fwd_bwd(FAKE, 4, 30, 20, _lib.F64, 1, flags, None, FAKE, FAKE, None, 0, None) == WS, \
            _lib.last_error()
        geo = (g["A"], g["B"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, flags)
        pgeo = (g["A"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, flags)
        assert L.sigsvgd_gram_long_fwd_bwd(FAKE, FAKE, *geo, None, FAKE, FAKE, None, 0, None) == WS, _lib.last_error()
        assert L.sigsvgd_gram_long_fwd_bwd2(FAKE, FAKE, *geo, None, FAKE, FAKE, FAKE, None, 0, None) == WS, _lib.last_error()
        assert L.sigsvgd_gram_long_fwd_bwd_h(FAKE, FAKE, *geo, None, FAKE, None, None, FAKE, None, 0, None) == WS, \
            _lib.last_error()
        assert L.sigsvgd_pair_fwd_bwd(FAKE, FAKE, *pgeo, None, FAKE, FAKE, FAKE, None, 0, None) == WS, _lib.last_error()
        assert L.sigsvgd_pair_fwd_bwd_h(FAKE, FAKE, *pgeo, None, FAKE, FAKE, None, FAKE, None, 0, None) == WS, \
            _lib.last_error()
    # every kind with the default stencil; the other flags of the two-sided mode with it
    for kind in E.KINDS:
        assert _ws("gram_long2_workspace_bytes", 3, 3, 300, 300, 2, 0, kind, 1, 0, EX | _lib.FLAG_Y_IS_X)[0] == OK
        assert _ws("gram_long_workspace_bytes", 3, 3, 300, 300, 2, 0, kind, 1, EX | _lib.FLAG_SYM)[0] == OK
    # an unknown bit beside it is still refused
    assert _ws("gram_long_workspace_bytes", 3, 3, 300, 300, 2, 0, 0, 1, EX | _lib.FLAG_WS_CLEAN)[0] == BADARG
    assert _ws("pair_workspace_bytes", 3, 300, 300, 2, 0, 0, 1, EX | _lib.FLAG_SYM)[0] == BADARG


def test_routes_without_exact_kernels_say_unsupported():
    L = lib()
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    assert L.sigsvgd_gram_long_partial_plan(64, 300, 2, 0, 0, EX, 2, ctypes.byref(r), ctypes.byref(c)) == UNSUPPORTED
    assert "SIGSVGD_FLAG_EXACT_ADJOINT" in _lib.last_error()
    assert _ws("gram_long_partial_workspace_bytes", 64, 300, 2, 0, 0, EX, 0, 2)[0] == UNSUPPORTED
    assert "SIGSVGD_FLAG_EXACT_ADJOINT" in _lib.last_error()
    rc = L.sigsvgd_gram_long_sym_partial(FAKE, 64, 300, 2, _lib.F64, 1.0, 0, 0, EX, 0, 2, None, FAKE, FAKE, FAKE, 1 << 30, None)
    assert rc == UNSUPPORTED and "SIGSVGD_FLAG_EXACT_ADJOINT" in _lib.last_error()
    assert _ws("gram_workspace_bytes", 8, 8, 32, 2, 0, 0, 1, EX)[0] == UNSUPPORTED
    assert "SIGSVGD_FLAG_EXACT_ADJOINT" in _lib.last_error()
    rc = L.sigsvgd_gram_fwd_bwd(FAKE, FAKE, 8, 8, 32, 2, _lib.F32, 1.0, 0, 0, EX, None, FAKE, FAKE, FAKE, 1 << 30, None)
    assert rc == UNSUPPORTED and "SIGSVGD_FLAG_EXACT_ADJOINT" in _lib.last_error()
    rc = L.sigsvgd_gram_sym_partial(FAKE, 8, 32, 2, _lib.F32, 1.0, 0, EX, 0, 1, None, FAKE, FAKE, FAKE, 1 << 30, None)
    assert rc == UNSUPPORTED and "SIGSVGD_FLAG_EXACT_ADJOINT" in _lib.last_error()
    # ... and without the bit these answer as they did
    assert _ws("gram_workspace_bytes", 8, 8, 32, 2, 0, 0, 1, 0)[0] == OK
    assert L.sigsvgd_gram_long_partial_plan(64, 300, 2, 0, 0, 0, 2, ctypes.byref(r), ctypes.byref(c)) == OK


def test_pair_schedule_reports_one_wave_per_pair(monkeypatch):
    """a shape whose unflagged gradient launch is band-parallel (pinned with SIGSVGD_PAIR_MODE, which the flag overrides)"""
    monkeypatch.setenv("SIGSVGD_PAIR_MODE", "bands")
    assert ops.pair_schedule(2, 1200, 1200, 2)[0] > 1
    assert ops.pair_schedule(2, 1200, 1200, 2, exact_adjoint=True)[0] == 1
    w, grid, lds = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    out = (ctypes.byref(w), ctypes.byref(grid), ctypes.byref(lds))
    # with the first-order stencil the launch is the unflagged one, and so is its schedule
    assert lib().sigsvgd_pair_schedule(2, 1200, 1200, 2, 0, 0, 1, EX | NV, *out) == OK and w.value > 1
    assert lib().sigsvgd_pair_schedule(2, 1200, 1200, 2, 0, 0, 0, EX, *out) == BADARG


# ---- 5: routing ----------------------------------------------------------------------------------------------------------------
A, B, T, TY, D = 5, 4, 6, 5, 2
LONG = ("gram_long_fwd_bwd", "gram_long_fwd_bwd2", "pair_fwd_bwd", "gram_long_fwd_bwd_h", "pair_fwd_bwd_h", "pde_fwd_bwd")
QUERIES = ("gram_long2_takes", "pair_takes", "gram_long_h_takes", "pair_h_takes")


class Recorder:
    """every `ops` function a SigKernel can reach notes the keywords it got beyond its parent-revision signature"""

    def __init__(self):
        self.calls = []

    def _note(self, name, kw):
        self.calls.append((name, dict(kw)))

    def gram_takes(self, A, B, T, d, dyadic_order=0, static_kind=0, want_grad=True, naive=False, sym=False, y_is_x=False, **kw):
        self._note("gram_takes", kw)
        return True  # (the fused kernels would take every launch: exact_grad must not ask them for a gradient)

    def gram_fwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, naive=False, force_generic=False, y_is_x=False,
                 stored_forward=False, **kw):
        self._note("gram_fwd", kw)
        return torch.zeros(X.shape[0], Y.shape[0], dtype=X.dtype)

    def gram_fwd_bwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False, y_is_x=False,
                     force_generic=False, check_regime=True, stored_forward=False, **kw):
        self._note("gram_fwd_bwd", kw)
        return torch.zeros(X.shape[0], Y.shape[0], dtype=X.dtype), torch.zeros_like(X)

    def gram_long_fwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, naive=False):
        self._note("gram_long_fwd", {})
        return torch.zeros(X.shape[0], Y.shape[0], dtype=X.dtype)

    def gram_long_fwd_bwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False, **kw):
        self._note("gram_long_fwd_bwd", kw)
        return torch.zeros(X.shape[0], Y.shape[0], dtype=X.dtype), torch.zeros_like(X)

    def gram_long2_takes(self, A, B, TX, TY, d, dyadic_order=0, static_kind=0, want_gradX=True, want_gradY=True, y_is_x=False,
                         **kw):
        self._note("gram_long2_takes", kw)
        return True

    def gram_long_fwd_bwd2(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False,
                           y_is_x=False, want_gradX=True, want_gradY=True, **kw):
        self._note("gram_long_fwd_bwd2", kw)
        K = torch.zeros(X.shape[0], Y.shape[0], dtype=X.dtype)
        return K, (torch.zeros_like(X) if want_gradX else None), (torch.zeros_like(Y) if want_gradY else None)

    def pair_takes(self, A, TX, TY, d, dyadic_order=0, static_kind=0, want_grad=True, **kw):
        self._note("pair_takes" if want_grad else "pair_takes_fwd", kw)  # (a forward-only call asks without the flag)
        return True

    def pair_fwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, naive=False):
        self._note("pair_fwd", {})
        return torch.zeros(X.shape[0], dtype=X.dtype)

    def pair_fwd_bwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, want_x=True, want_y=True,
                     **kw):
        self._note("pair_fwd_bwd", kw)
        return (torch.zeros(X.shape[0], dtype=X.dtype), torch.zeros_like(X) if want_x else None,
                torch.zeros_like(Y) if want_y else None)

    def gram_long_h_takes(self, A, B, TX, TY, d, dyadic_order=0, static_kind=0, want_gradX=True, want_gradY=True, naive=False,
                          y_is_x=False, **kw):
        self._note("gram_long_h_takes", kw)
        return True

    def gram_long_fwd_bwd_h(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False,
                            y_is_x=False, want_gradX=True, want_gradY=True, **kw):
        self._note("gram_long_fwd_bwd_h", kw)
        K = torch.zeros(X.shape[0], Y.shape[0], dtype=X.dtype)
        return K, (torch.zeros_like(X) if want_gradX else None), (torch.zeros_like(Y) if want_gradY else None), K.clone()

    def pair_h_takes(self, A, TX, TY, d, dyadic_order=0, static_kind=0, naive=False, **kw):
        self._note("pair_h_takes", kw)
        return True

    def pair_fwd_bwd_h(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, want_x=True, want_y=True,
                       **kw):
        K = torch.zeros(X.shape[0], dtype=X.dtype)
        self._note("pair_fwd_bwd_h", kw)
        return K, (torch.zeros_like(X) if want_x else None), (torch.zeros_like(Y) if want_y else None), K.clone()

    def pde_fwd(self, G, dyadic_order=0, naive=False):
        self._note("pde_fwd", {})
        return torch.zeros(G.shape[0], dtype=G.dtype)

    def pde_fwd_bwd(self, G, dyadic_order=0, grad_out=None, naive=False, **kw):
        self._note("pde_fwd_bwd", kw)
        return torch.zeros(G.shape[0], dtype=G.dtype), torch.zeros_like(G)


def paths(n, t, grad):
    return torch.linspace(0.0, 1.0, n * t * D, dtype=torch.float64).reshape(n, t, D).requires_grad_(grad)


def run_everything(kernel):
    """forward-only, speculated, weighted backward, grad_Y, sym, gram_and_grad, compute_kernel, compute_distance, compute_mmd"""
    X, Y = paths(A, T, True), paths(B, TY, True)
    kernel.compute_Gram(X.detach(), Y.detach())
    K = kernel.compute_Gram(X, X)
    (K * torch.arange(1.0, K.numel() + 1.0, dtype=K.dtype).reshape(K.shape)).sum().backward()
    kernel.compute_Gram(X, Y, grad_Y=True).sum().backward()
    kernel.compute_Gram(X, X, sym=True).sum().backward()
    kernel.gram_and_grad(X.detach(), Y.detach())
    kernel.gram_and_grad(X.detach(), None, sym=True)
    Z = paths(A, TY, True)
    kernel.compute_kernel(X.detach(), Z.detach())
    kernel.compute_kernel(X, Z).sum().backward()
    kernel.compute_distance(X, Z).backward()
    kernel.compute_mmd(X, Y, grad_Y=True).backward()


def record(monkeypatch, kernel):
    rec = Recorder()
    for name in [n for n in dir(rec) if not n.startswith("_") and n != "calls"]:
        monkeypatch.setattr(ops, name, getattr(rec, name))
    monkeypatch.setattr(sk, "_device_cus", lambda X: 256)
    run_everything(kernel)
    return rec.calls


class UserRBF:
    """a user static kernel: upstream's interface and nothing the package recognises"""

    def Gram_matrix(self, X, Y):
        return torch.exp(-sk.gram_sqdist(X, Y))

    def batch_kernel(self, X, Y):
        return torch.exp(-sk.batch_sqdist(X, Y))


def static_kernels():
    return [sk.RBFKernel(0.7), sk.LinearKernel(), sk.Matern52StaticKernel(0.7),
            sk.RBFKernel(torch.tensor(0.7, dtype=torch.float64, requires_grad=True)), UserRBF()]


@pytest.mark.parametrize("static", static_kernels(), ids=["rbf", "linear", "matern52", "learned_sigma", "user"])
def test_exact_grad_reaches_only_flagged_long_route_launches(monkeypatch, static):
    calls = record(monkeypatch, sk.SigKernel(static, 1, exact_grad=True))
    names = {name for name, _ in calls}
    assert "gram_fwd_bwd" not in names  # no gradient from a GG-only route
    grads = [(name, kw) for name, kw in calls if name in LONG]
    assert grads and all(kw == {"exact_adjoint": True} for _, kw in grads), grads
    asked = [(name, kw) for name, kw in calls if name in QUERIES]
    assert all(kw == {"exact_adjoint": True} for _, kw in asked), asked
    # forward-only calls are untouched: they ask the fused kernels first, with no new keyword
    assert all(kw == {} for name, kw in calls
               if name in ("gram_takes", "gram_fwd", "gram_long_fwd", "pair_takes_fwd", "pair_fwd", "pde_fwd"))
    if isinstance(static, UserRBF):
        assert names <= {"pde_fwd", "pde_fwd_bwd"}
    elif isinstance(getattr(static, "sigma", None), torch.Tensor):
        assert {"gram_long_fwd_bwd_h", "pair_fwd_bwd_h"} <= names
    else:
        assert "pair_fwd_bwd" in names and names & {"gram_long_fwd_bwd", "gram_long_fwd_bwd2"}


@pytest.mark.parametrize("static", static_kernels(), ids=["rbf", "linear", "matern52", "learned_sigma", "user"])
def test_default_kernel_hands_over_no_keyword(monkeypatch, static):
    calls = record(monkeypatch, sk.SigKernel(static, 1))
    assert calls and all(kw == {} for _, kw in calls), [c for c in calls if c[1]]


def test_exact_grad_refusals(monkeypatch):
    with pytest.raises(ValueError, match="fp32_sweeps"):
        sk.SigKernel(sk.IMQStaticKernel(1.0), 0, fp32_sweeps=True, exact_grad=True)
    from sigsvgd_amd.kernels import SignatureKernel

    assert SignatureKernel(lambda _: 1.0, depth=0, exact_grad=True).kernel.exact_grad is True
    assert SignatureKernel(lambda _: 1.0, depth=0).kernel.exact_grad is False
    # a shape the long route refuses (the library's own answer, host only): NotImplementedError, no launch
    kernel = sk.SigKernel(sk.RBFKernel(1.0), 10, exact_grad=True)
    X = paths(2, 10, True)  # 9 * 1024 cells > 8192
    with pytest.raises(NotImplementedError, match="exact"):
        kernel.compute_Gram(X, X)
    with pytest.raises(NotImplementedError, match="exact"):
        kernel.compute_kernel(X, X)
