"""The normalised kernel and its gradient from one launch (SIGSVGD_FLAG_NORMALIZED) without a device:
(a) the host side of the C ABI (every acceptance and refusal of the flag returns before any device work), (b) which launches
`SigKernel(..., normalize=True).gram_and_grad`, `kernels.SignatureKernel(normalize=True)` and an `SVGD` step on it issue, with
a recorder over `ops` in the style of tests/test_log_k_cpu.py, and (c) the first-slot semantics of the Y_IS_X launch, stated on
the reference of tests/log_k_reference.py, against torch autograd.

On a library without the feature bit 2048 is SIGSVGD_E_BADARG and `normalize=` does not reach `gram_and_grad`: (a) and (b) fail."""
import ctypes

import numpy as np
import pytest
import torch

import log_k_reference as R
import sigsvgd_amd.sigkernel as sk
from cabi import BADARG, FAKE, OK, UNSUPPORTED, WORKSPACE, exported_symbols, lib
from sigsvgd_amd import _lib, ops

NM, LK, NT, EX, NV, YX, SYM = (2048, _lib.FLAG_LOG_K, _lib.FLAG_NAN_TAILS, _lib.FLAG_EXACT_ADJOINT, _lib.FLAG_NAIVE_SOLVER,
                               _lib.FLAG_Y_IS_X, _lib.FLAG_SYM)
GEO = dict(A=3, B=3, TX=300, TY=300, d=2, n=0)
NAME = "SIGSVGD_FLAG_NORMALIZED"


def _ws(name, *args):
    b = ctypes.c_size_t(12345)
    rc = getattr(lib(), "sigsvgd_" + name)(*args, ctypes.byref(b))
    return rc, b.value


# ---- (a) the host side of the C ABI ----------------------------------------------------------------------------------------------
def test_the_bit_is_2048_and_the_abi_is_still_version_10_with_39_exports():
    assert lib().sigsvgd_abi_version() == _lib.ABI_VERSION == 10
    assert len(exported_symbols()) == len(_lib.EXPORTS) == 39
    assert _lib.FLAG_NORMALIZED == NM == 2048
    assert ops._flags(False, False, False, False, normalized=True) == 2048
    assert ops._flags(False, True, True, False, normalized=True) == 2 | 4 | 2048
    assert ops._flags(False, False, False, False) == 0


def test_the_two_accepting_entry_points_take_the_flag():
    """both pass their flag check with the bit in every mode -- both sides, row only, column only, Y_IS_X, Y_IS_X | SYM, SYM,
    forward only: the refusal the launch then gives is the next check's (a workspace of 0 bytes, before any device work), not
    BADARG.  A forward-only flagged launch needs a workspace too: the diagonals' logarithms and the block exponents."""
    g, L = GEO, lib()
    geo = lambda f: (g["A"], g["B"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, NM | f)
    for gx, gy, f in [(FAKE, FAKE, 0), (FAKE, None, 0), (None, FAKE, 0), (FAKE, None, YX), (FAKE, None, YX | SYM),
                      (FAKE, None, SYM), (None, None, 0), (None, None, YX)]:
        for go in (None, FAKE):
            assert L.sigsvgd_gram_long_fwd_bwd2(FAKE, FAKE, *geo(f), go, FAKE, gx, gy, None, 0, None) == WORKSPACE, \
                (gx, gy, f, _lib.last_error())
        rc, b = _ws("gram_long2_workspace_bytes", g["A"], g["B"], g["TX"], g["TY"], g["d"], g["n"], 0, int(gx is not None),
                    int(gy is not None), NM | f)
        assert rc == OK and b > 0, (gx, gy, f, _lib.last_error())
    for kind in (0, 1, 2, 3, 6, 7):  # every kind, orders past 0, both I/O types
        for n in (0, 2):
            assert _ws("gram_long2_workspace_bytes", 3, 3, 300, 300, 2, n, kind, 1, 1, NM)[0] == OK, _lib.last_error()
            for dtype in (_lib.F32, _lib.F64):
                assert L.sigsvgd_gram_long_fwd_bwd2(FAKE, FAKE, 3, 3, 300, 300, 2, dtype, 1.0, n, kind, NM, None, FAKE, FAKE,
                                                    FAKE, None, 0, None) == WORKSPACE, _lib.last_error()
    # an unknown bit beside it is still refused
    assert _ws("gram_long2_workspace_bytes", 3, 3, 300, 300, 2, 0, 0, 1, 1, NM | _lib.FLAG_WS_CLEAN)[0] == BADARG
    assert _ws("gram_long2_workspace_bytes", 3, 3, 300, 300, 2, 0, 0, 1, 1, NM | 4096)[0] == BADARG


@pytest.mark.parametrize("other,name", [(NV, "SIGSVGD_FLAG_NAIVE_SOLVER"), (EX, "SIGSVGD_FLAG_EXACT_ADJOINT"),
                                        (NT, "SIGSVGD_FLAG_NAN_TAILS"), (LK, "SIGSVGD_FLAG_LOG_K")])
def test_the_four_forbidden_pairs_say_unsupported_and_name_both_flags(other, name):
    g, L = GEO, lib()
    geo = (g["A"], g["B"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, NM | other)
    two = (g["A"], g["B"], g["TX"], g["TY"], g["d"], g["n"], 0)
    calls = [
        lambda: L.sigsvgd_gram_long_fwd_bwd2(FAKE, FAKE, *geo, None, FAKE, FAKE, FAKE, FAKE, 1 << 30, None),
        lambda: L.sigsvgd_gram_long_fwd_bwd2(FAKE, FAKE, *geo, None, FAKE, None, None, FAKE, 1 << 30, None),
        lambda: _ws("gram_long2_workspace_bytes", *two, 1, 1, NM | other)[0],
        lambda: _ws("gram_long2_workspace_bytes", *two, 0, 0, NM | other)[0],
    ]
    for k, call in enumerate(calls):
        assert call() == UNSUPPORTED, (k, _lib.last_error())
        assert NAME in _lib.last_error() and name in _lib.last_error(), (k, _lib.last_error())


def test_other_entry_points_answer_as_before():
    """every entry point but the accepting two keeps its answer for bit 2048: an unknown flag bit where it checks its flags,
    no effect where it does not"""
    g, L = GEO, lib()
    geo = (g["A"], g["B"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, NM)
    pgeo = (g["A"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, NM)
    two = (g["A"], g["B"], g["TX"], g["TY"], g["d"], g["n"], 0)
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    w, grid, lds = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    calls = [
        lambda: L.sigsvgd_gram_long_fwd(FAKE, FAKE, *geo, FAKE, FAKE, 1 << 30, None),
        lambda: L.sigsvgd_gram_long_fwd_bwd(FAKE, FAKE, *geo, None, FAKE, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("gram_long_workspace_bytes", *two, 1, NM)[0],
        lambda: L.sigsvgd_gram_long_fwd_bwd_h(FAKE, FAKE, *geo, None, FAKE, FAKE, None, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("gram_long_h_workspace_bytes", *two, 1, 0, NM)[0],
        lambda: L.sigsvgd_pair_fwd(FAKE, FAKE, *pgeo, FAKE, FAKE, 1 << 30, None),
        lambda: L.sigsvgd_pair_fwd_bwd(FAKE, FAKE, *pgeo, None, FAKE, FAKE, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("pair_workspace_bytes", g["A"], g["TX"], g["TY"], g["d"], g["n"], 0, 1, NM)[0],
        lambda: L.sigsvgd_pair_schedule(g["A"], g["TX"], g["TY"], g["d"], g["n"], 0, 1, NM, ctypes.byref(w), ctypes.byref(grid),
                                        ctypes.byref(lds)),
        lambda: L.sigsvgd_pair_fwd_bwd_h(FAKE, FAKE, *pgeo, None, FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("pair_h_workspace_bytes", g["A"], g["TX"], g["TY"], g["d"], g["n"], 0, NM)[0],
        lambda: L.sigsvgd_gram_long_sym_partial(FAKE, 64, 300, 2, _lib.F64, 1.0, 0, 0, NM, 0, 2, None, FAKE, FAKE, FAKE,
                                                1 << 30, None),
        lambda: L.sigsvgd_gram_long_partial_plan(64, 300, 2, 0, 0, NM, 2, ctypes.byref(r), ctypes.byref(c)),
        lambda: _ws("gram_long_partial_workspace_bytes", 64, 300, 2, 0, 0, NM, 0, 2)[0],
        lambda: _ws("pde_workspace_bytes", 4, 30, 20, 1, 1, NM)[0],
        lambda: L.sigsvgd_pde_fwd(FAKE, 4, 30, 20, _lib.F64, 1, NM, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("sqdist_select_workspace_bytes", 4, 4, 9, 9, 2, NM)[0],
    ]
    for k, call in enumerate(calls):
        assert call() == BADARG, (k, _lib.last_error())
        assert "0x800" in _lib.last_error(), (k, _lib.last_error())
    # the paired entry points still refuse it beside the flags they take
    assert _ws("pair_workspace_bytes", g["A"], g["TX"], g["TY"], g["d"], g["n"], 0, 1, NM | LK)[0] == BADARG
    assert _ws("gram_workspace_bytes", 8, 8, 32, 2, 0, 0, 1, NM) == _ws("gram_workspace_bytes", 8, 8, 32, 2, 0, 0, 1, 0)


def test_flagged_workspace_is_at_least_the_log_domain_launchs():
    """the LOG_K launch's bytes, the diagonals' logarithms, for a gradient launch the pairs' fp64 weights, and per side whose
    gradient is wanted its fp64 diagonal gradients and sums: never less, and a forward-only flagged launch needs some too"""
    pad = lambda b: (b + 255) & ~255
    for (A, B, TX, TY, d, n) in [(3, 3, 300, 300, 2, 0), (2, 5, 70, 131, 3, 1), (100, 70, 40, 30, 2, 0)]:
        for gx, gy, f in [(1, 1, 0), (1, 0, 0), (0, 1, 0), (0, 0, 0), (1, 0, YX), (0, 0, YX), (1, 0, YX | SYM)]:
            if (f & YX) and (A != B or TX != TY):
                continue
            rc0, b0 = _ws("gram_long2_workspace_bytes", A, B, TX, TY, d, n, 0, gx, gy, f | LK)
            rc1, b1 = _ws("gram_long2_workspace_bytes", A, B, TX, TY, d, n, 0, gx, gy, f | NM)
            assert rc0 == OK and rc1 == OK and b1 >= b0 > 0, (A, B, gx, gy, f, b0, b1, _lib.last_error())
            # what the flag adds at the least (the diagonal passes' scratch aliases the launch's and may enlarge it)
            least = pad(8 * (A + (0 if f & YX else B)))
            least += gx * (pad(8 * A * TX * d) + pad(8 * A)) + gy * (pad(8 * B * TY * d) + pad(8 * B))
            least += pad(8 * A * B) if gx or gy else 0  # the pairs' weights w K^ of a gradient launch
            assert b1 >= b0 + least, (A, B, gx, gy, f, b0, b1, least)


def test_a_shape_whose_diagonal_pass_outgrows_the_lds_is_refused_as_a_whole():
    """the diagonal pass solves (X_i, X_i) on a TX x TX grid: with one long side and many channels its per-wave state -- the
    ring of 64 x 128 increments, the boundary row of TX cells, 65 points of d channels -- passes 160 KiB where the launch's own
    TX x 2 grid does not.  The flagged launch and its query then answer UNSUPPORTED before any device work, with the plan's
    message; the LOG_K launch of the same shape is taken, and so is the flagged one with the sides swapped into one the
    diagonal passes fit (fewer channels)."""
    L = lib()
    A, B, TX, TY, d = 2, 2, 4000, 2, 200
    assert (64 + (TX - 1) + 2 + 64 + 65 * d) * 8 < 160 * 1024 < (64 * 128 + (TX - 1) + 2 + 64 + 65 * d) * 8
    for gx, gy in [(1, 1), (1, 0), (0, 1), (0, 0)]:
        assert _ws("gram_long2_workspace_bytes", A, B, TX, TY, d, 0, 0, gx, gy, LK)[0] == OK, _lib.last_error()
        assert _ws("gram_long2_workspace_bytes", A, B, TX, TY, d, 0, 0, gx, gy, NM)[0] == UNSUPPORTED
        assert "LDS" in _lib.last_error(), _lib.last_error()
    assert L.sigsvgd_gram_long_fwd_bwd2(FAKE, FAKE, A, B, TX, TY, d, _lib.F64, 1.0, 0, 0, NM, None, FAKE, FAKE, FAKE, FAKE, 1 << 30,
                                        None) == UNSUPPORTED
    assert "LDS" in _lib.last_error(), _lib.last_error()
    assert ops.gram_long2_takes(A, B, TX, TY, d, normalized=True) is False and ops.gram_long2_takes(A, B, TX, TY, d, log_k=True)
    assert _ws("gram_long2_workspace_bytes", A, B, TX, TY, 50, 0, 0, 1, 1, NM)[0] == OK, _lib.last_error()


# ---- (b) the Python layer --------------------------------------------------------------------------------------------------------
A, B, T, TY, D = 5, 4, 6, 5, 2
NKW = {"normalized": True}


class Recorder:
    """stands in for the launches and queries of `ops` a normalised call may reach; every other launch raises"""

    def __init__(self, takes=True):
        self.takes, self.launches, self.queries = takes, [], []

    def gram_long2_takes(self, A, B, TX, TY, d, dyadic_order=0, static_kind=0, want_gradX=True, want_gradY=True, y_is_x=False,
                         **kw):
        self.queries.append(("gram_long2_takes", bool(want_gradX), bool(want_gradY), bool(y_is_x), dict(kw)))
        return self.takes

    def gram_long_fwd_bwd2(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False,
                           y_is_x=False, want_gradX=True, want_gradY=True, **kw):
        flags = dict(naive=naive, sym=sym, yx=y_is_x, gx=want_gradX, gy=want_gradY, w=grad_out is not None)
        self.launches.append(("gram_long_fwd_bwd2", tuple(X.shape), tuple(Y.shape), X.data_ptr() == Y.data_ptr(),
                              " ".join(k for k, v in flags.items() if v), dict(kw),
                              None if grad_out is None else grad_out.clone()))
        return (torch.full((X.shape[0], Y.shape[0]), 0.5, dtype=X.dtype), 2 * torch.ones_like(X) if want_gradX else None,
                torch.ones_like(Y) if want_gradY and not (sym or y_is_x) else None)

    def svgd_phi(self, K, score, grad_k, **kw):
        self.launches.append(("svgd_phi", tuple(K.shape), tuple(grad_k.shape)))
        return torch.zeros_like(score)

    def install(self, monkeypatch):
        def refuse(name):
            def f(*a, **k):
                raise AssertionError(f"ops.{name} reached by a normalised gram_and_grad")
            return f

        for name in ("gram_takes", "gram_fwd", "gram_fwd_bwd", "gram_long_fwd", "gram_long_fwd_bwd", "gram_long_fwd_bwd_h",
                     "pair_fwd", "pair_fwd_bwd", "pair_takes", "pair_fwd_bwd_h", "path_sqdist_select", "pde_fwd_bwd"):
            monkeypatch.setattr(ops, name, refuse(name))
        for name in ("gram_long2_takes", "gram_long_fwd_bwd2", "svgd_phi"):
            monkeypatch.setattr(ops, name, getattr(self, name))
        return self


def paths(n, t, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, t, D, dtype=torch.float64, generator=g)


def brief(rec):
    return [c[:6] for c in rec.launches]


def test_gram_and_grad_issues_exactly_one_flagged_launch(monkeypatch):
    rec = Recorder().install(monkeypatch)
    kernel = sk.SigKernel(sk.RBFKernel(1.0), 0, normalize=True)
    X, Y = paths(A, T), paths(B, TY, 1)
    sx, sy = (A, T, D), (B, TY, D)
    K, g = kernel.gram_and_grad(X)
    assert brief(rec) == [("gram_long_fwd_bwd2", sx, sx, True, "yx gx", NKW)]
    assert rec.queries == [("gram_long2_takes", True, False, True, NKW)]
    assert torch.equal(K, torch.full((A, A), 0.5).double()) and torch.equal(g, 2 * torch.ones_like(X))  # handed back as they are
    # weights, sym, and a second batch: one launch each, the weights as given
    G = torch.arange(1.0, A * A + 1).reshape(A, A).double()
    rec.launches.clear()
    kernel.gram_and_grad(X, None, G, sym=True)
    assert brief(rec) == [("gram_long_fwd_bwd2", sx, sx, True, "sym yx gx w", NKW)] and torch.equal(rec.launches[0][6], G)
    rec.launches.clear()
    K, g = kernel.gram_and_grad(X, Y, G[:, :B])
    assert brief(rec) == [("gram_long_fwd_bwd2", sx, sy, False, "gx w", NKW)] and K.shape == (A, B) and g.shape == X.shape
    rec.launches.clear()
    sk.gram_and_grad(kernel, X)  # the module-level function
    assert brief(rec) == [("gram_long_fwd_bwd2", sx, sx, True, "yx gx", NKW)]
    # every kind and order the constructor takes
    rec.launches.clear()
    sk.SigKernel(sk.IMQStaticKernel(2.0), 2, normalize=True).gram_and_grad(X)
    assert brief(rec) == [("gram_long_fwd_bwd2", sx, sx, True, "yx gx", NKW)]


def test_signature_kernel_hands_the_flag_on_and_an_svgd_step_issues_the_launch(monkeypatch):
    from sigsvgd_amd.inference import SVGD
    from sigsvgd_amd.kernels import SignatureKernel

    rec = Recorder().install(monkeypatch)
    kernel = SignatureKernel(depth=0, static_kernel=sk.RBFKernel(1.0), normalize=True)
    assert kernel.kernel.normalize is True
    assert SignatureKernel(depth=0, static_kernel=sk.RBFKernel(1.0)).kernel.normalize is False
    X = paths(A, T)
    sx = (A, T, D)
    K, g = kernel.gram_and_grad(X)
    assert brief(rec) == [("gram_long_fwd_bwd2", sx, sx, True, "yx gx", NKW)]
    rec.launches.clear()
    svgd = SVGD(kernel, optimizer_class=None, lr=0.1)
    X1, info = svgd.step(X, grad_log_p=torch.ones_like(X))
    assert rec.launches[0][:6] == ("gram_long_fwd_bwd2", sx, sx, True, "yx gx", NKW)
    assert rec.launches[1:] == [("svgd_phi", (A, A), (A, T * D))]
    assert torch.equal(info["k_xx"], torch.full((A, A), 0.5).double()) and X1.shape == X.shape


def test_the_default_issues_what_it_issued_before(monkeypatch):
    """normalize=False, the default: `gram_and_grad` reaches `ops` as it always did -- recorders with the signatures from before
    the keyword, so a `normalized=` handed to any of them is a TypeError"""
    from sigsvgd_amd.kernels import SignatureKernel

    seen = []

    def gram_takes(A, B, T, d, dyadic_order=0, static_kind=0, want_grad=True, naive=False, sym=False, y_is_x=False,
                   fp32_sweeps=False):
        return True

    def gram_fwd_bwd(X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False, y_is_x=False,
                     force_generic=False, check_regime=True, stored_forward=False, fp32_sweeps=False):
        seen.append(("gram_fwd_bwd", sym, y_is_x))
        return torch.zeros(X.shape[0], Y.shape[0], dtype=X.dtype), torch.zeros_like(X)

    for f in (gram_takes, gram_fwd_bwd):
        monkeypatch.setattr(ops, f.__name__, f)
    X = paths(A, T)
    for kernel in (sk.SigKernel(sk.RBFKernel(1.0), 0), sk.SigKernel(sk.RBFKernel(1.0), 0, normalize=False),
                   SignatureKernel(depth=0, static_kernel=sk.RBFKernel(1.0)).kernel,
                   SignatureKernel(depth=0, static_kernel=sk.RBFKernel(1.0), normalize=False).kernel):
        kernel.gram_and_grad(X)
    assert seen == [("gram_fwd_bwd", False, True)] * 4


def test_refusals_are_raised_before_any_launch(monkeypatch):
    from parity import DisguisedRBF

    rec = Recorder().install(monkeypatch)
    X, Y = paths(A, T), paths(B, TY, 1)
    with pytest.raises(ValueError, match="fp32_sweeps"):
        sk.SigKernel(sk.IMQStaticKernel(1.0), 0, fp32_sweeps=True, normalize=True)
    with pytest.raises(NotImplementedError, match="exact_grad"):
        sk.SigKernel(sk.RBFKernel(1.0), 0, exact_grad=True, normalize=True)
    with pytest.raises(NotImplementedError, match="_naive_solver"):
        sk.SigKernel(sk.RBFKernel(1.0), 0, _naive_solver=True, normalize=True)
    learned = sk.SigKernel(sk.RBFKernel(torch.tensor(1.0, requires_grad=True)), 0, normalize=True)
    for call in (lambda: learned.gram_and_grad(X), lambda: learned.gram_and_grad(X, Y)):
        with pytest.raises(NotImplementedError, match="sigma that requires grad"):
            call()
    user = sk.SigKernel(DisguisedRBF(1.0), 0, normalize=True)
    for call in (lambda: user.gram_and_grad(X), lambda: user.gram_and_grad(X, Y)):
        with pytest.raises(NotImplementedError, match="user static kernel"):
            call()
    assert rec.launches == [] and rec.queries == []
    # shapes the long route refuses
    rec.takes = False
    monkeypatch.setattr(_lib, "last_error", lambda: "refused")
    with pytest.raises(NotImplementedError, match="the normalised kernel"):
        sk.SigKernel(sk.RBFKernel(1.0), 0, normalize=True).gram_and_grad(X)
    assert rec.launches == [] and rec.queries == [("gram_long2_takes", True, False, True, NKW)]


# ---- (c) the first-slot semantics of the Y_IS_X launch --------------------------------------------------------------------------
def test_first_slot_semantics_against_torch_autograd():
    """gradX_out[i] of the Y_IS_X launch without SYM is the derivative in X_i of sum_j w_ij K^(X_i, stop(X_j)) -- what
    `normalized_gram_and_grads(X, X.copy(), w)[1]` returns -- and with SYM the derivative of sum_ij w_ij K^(X_i, X_j) in both
    slots, the `same=True` result: at A = 3, T = 9, d = 2, where K fits fp64, against torch autograd through
    K / sqrt(K_xx K_yy) of the oracle.  The diagonal pair contributes nothing: its row of K^ is constant 1."""
    X = R.walks(1, 3, 9, 2, 0.5)
    w = np.random.default_rng(3).standard_normal((3, 3))
    w[1, 2] = 0.0
    Khat, gX, _ = R.normalized_gram_and_grads(X, X.copy(), w)
    Xt = torch.tensor(X, requires_grad=True)
    ref = R.normalized_torch(Xt, Xt.detach().clone())
    (g,) = torch.autograd.grad((torch.tensor(w) * ref).sum(), Xt)
    assert np.abs(Khat - ref.detach().numpy()).max() < 1e-13
    assert np.abs(gX - g.numpy()).max() < 1e-12 * np.abs(gX).max()
    # the diagonal weights change nothing
    w0 = w.copy()
    np.fill_diagonal(w0, 0.0)
    g0 = R.normalized_gram_and_grads(X, X.copy(), w0)[1]
    assert np.abs(gX - g0).max() < 1e-12 * np.abs(gX).max()
    # SYM: both slots of one tensor
    _, gS, _ = R.normalized_gram_and_grads(X, X, w, same=True)
    Xs = torch.tensor(X, requires_grad=True)
    (gs,) = torch.autograd.grad((torch.tensor(w) * R.normalized_torch(Xs, Xs)).sum(), Xs)
    assert np.abs(gS - gs.numpy()).max() < 1e-12 * np.abs(gS).max()
    first_sym = R.normalized_gram_and_grads(X, X.copy(), w + w.T)[1]
    assert np.abs(gS - first_sym).max() < 1e-12 * np.abs(gS).max()  # = the first-slot gradient under w + w^T
