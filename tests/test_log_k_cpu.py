"""The log-domain solve and the normalised kernel (SIGSVGD_FLAG_LOG_K) without a device: (a) the numpy
restatement of tests/log_k_reference.py against the plain oracle and a long-double run, (b) the host side of the C ABI (every
acceptance and refusal of the flag returns before any device work), (c) which launches `SigKernel(..., normalize=True)` and
the `compute_log_*` methods issue, with a recorder over `ops` in the style of tests/test_nan_tails_cpu.py, and (d) the algebra
of the normalisation, fed with the reference's ln K and gradients, against torch autograd."""
import ctypes

import numpy as np
import pytest
import torch

import log_k_reference as R
import sigsvgd_amd.sigkernel as sk
from cabi import BADARG, FAKE, OK, UNSUPPORTED, WORKSPACE, exported_symbols, lib
from oracle import sigkernel_oracle as O
from sigsvgd_amd import _lib, ops

LK, NT, EX, NV, YX, SYM = (_lib.FLAG_LOG_K, _lib.FLAG_NAN_TAILS, _lib.FLAG_EXACT_ADJOINT, _lib.FLAG_NAIVE_SOLVER,
                           _lib.FLAG_Y_IS_X, _lib.FLAG_SYM)
GEO = dict(A=3, B=3, TX=300, TY=300, d=2, n=0)
NAME = "SIGSVGD_FLAG_LOG_K"


def _ws(name, *args):
    b = ctypes.c_size_t(12345)
    rc = getattr(lib(), "sigsvgd_" + name)(*args, ctypes.byref(b))
    return rc, b.value


# ---- (a) the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,step", [(O.RBF, 0.5), (O.LINEAR, 0.12)])
@pytest.mark.parametrize("n", [0, 1, 2])
def test_reference_is_the_log_of_the_oracle(kind, step, n):
    """ln K = log(K) and grad ln K = grad K / K (the oracle's GG gradient weighted by w / K; the second slot from the swapped
    call) to fp64 rounding -- 1e-12: every anti-diagonal adds a few roundings, and dividing by arbitrary factors a few more --
    and the same whatever the anti-diagonals are divided by"""
    X, Y = R.walks(n, 3, 9, 2, step), R.walks(n + 10, 2, 7, 2, step)
    w = np.random.default_rng(n).uniform(0.5, 1.5, (3, 2))
    K = O.gram(X, Y, kind, 1.0, n)
    assert (K > 0).all()
    gX = O.gram_backward(X, Y, w / K, kind, 1.0, n)[1]
    gY = O.gram_backward(Y, X, (w / K).T, kind, 1.0, n)[1]
    rng = np.random.default_rng(5)
    for factor in (R._by_max, lambda s, v: rng.uniform(0.1, 10.0, size=v.shape[:-1])):
        ln, rX, rY = R.log_gram_backward(X, Y, w, kind, 1.0, n, factor=factor)
        assert np.abs(ln - np.log(K)).max() < 1e-12  # (the bound tests/test_nan_tails_cpu.py holds two sweeps of one K to)
        assert np.abs(rX - gX).max() < 1e-12 * np.abs(gX).max() and np.abs(rY - gY).max() < 1e-12 * np.abs(gY).max()
    lp, pX, pY = R.log_pair_backward(X[:2], Y, w[0])
    ld = R.log_gram(X[:2], Y)
    assert np.array_equal(lp, ld.diagonal())


def test_reference_nan_where_K_is_not_positive():
    """two-channel rough walks of 131 points have pairs whose discrete K is negative: NaN there, finite elsewhere"""
    X, Y = R.walks(300, 2, 131, 2, 0.5).astype(np.float32), R.walks(301, 2, 131, 2, 0.5).astype(np.float32)
    K = O.gram(X, Y)
    assert (K <= 0).any() and (K > 0).any()
    assert np.array_equal(np.isnan(R.log_gram(X, Y)), K <= 0)


def test_reference_on_an_overflowing_pair_against_long_double():
    if np.finfo(np.longdouble).maxexp < 16384:  # (x87 extended: finite up to 1e4932)
        pytest.skip("np.longdouble is not wider than fp64 here: no unscaled run of an overflowing pair to compare with")
    x = R.walks(3, 1, 1700, 3, 2.0).astype(np.float32).astype(np.float64)
    ln = R.log_gram(x, x)[0, 0]
    assert ln > 709.79  # K itself is past DBL_MAX
    want = R.longdouble_log_K(R.EA.static_gram(x, x, O.RBF, 1.0)[0, 0])
    assert abs(ln - float(want)) < 1e-12 * ln


# ---- (b) the host side of the C ABI ----------------------------------------------------------------------------------------------
def test_abi_is_still_version_10_with_39_exports():
    assert lib().sigsvgd_abi_version() == _lib.ABI_VERSION == 10
    assert len(exported_symbols()) == len(_lib.EXPORTS) == 39
    assert _lib.FLAG_LOG_K == 1024
    assert ops._flags(False, False, False, False, log_k=True) == 1024
    assert ops._flags(False, True, True, False, log_k=True) == 2 | 4 | 1024
    assert ops._flags(True, True, True, True, True, True, True, True) == 1 | 2 | 4 | 8 | 32 | 128 | 256 | 512  # (as before)


def test_accepting_entry_points_take_the_flag():
    """every accepting entry point passes its flag check with the bit: the refusal it then gives is the next check's (a
    workspace of 0 bytes, before any device work), not BADARG.  A forward-only flagged launch needs a workspace too: the block
    exponents."""
    g, L = GEO, lib()
    geo = lambda f: (g["A"], g["B"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, LK | f)
    pgeo = (g["A"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, LK)
    for gx, gy, f in [(None, None, 0), (FAKE, None, 0), (None, FAKE, 0), (FAKE, FAKE, 0), (FAKE, None, YX),
                      (FAKE, None, YX | SYM), (None, None, YX), (FAKE, None, SYM)]:
        assert L.sigsvgd_gram_long_fwd_bwd2(FAKE, FAKE, *geo(f), FAKE, FAKE, gx, gy, None, 0, None) == WORKSPACE, \
            _lib.last_error()
    assert L.sigsvgd_pair_fwd(FAKE, FAKE, *pgeo, FAKE, None, 0, None) == WORKSPACE, _lib.last_error()
    for gx, gy in [(FAKE, FAKE), (FAKE, None), (None, FAKE)]:
        assert L.sigsvgd_pair_fwd_bwd(FAKE, FAKE, *pgeo, None, FAKE, gx, gy, None, 0, None) == WORKSPACE, _lib.last_error()
    for kind in (0, 1, 2, 3, 6, 7):  # every kind, and orders past 0
        for n in (0, 2):
            assert _ws("gram_long2_workspace_bytes", 3, 3, 300, 300, 2, n, kind, 1, 1, LK)[0] == OK, _lib.last_error()
            assert _ws("pair_workspace_bytes", 3, 300, 300, 2, n, kind, 1, LK)[0] == OK, _lib.last_error()
    # an unknown bit beside it is still refused
    assert _ws("gram_long2_workspace_bytes", 3, 3, 300, 300, 2, 0, 0, 1, 1, LK | _lib.FLAG_WS_CLEAN)[0] == BADARG
    assert _ws("pair_workspace_bytes", 3, 300, 300, 2, 0, 0, 1, LK | SYM)[0] == BADARG


@pytest.mark.parametrize("other,name", [(NV, "SIGSVGD_FLAG_NAIVE_SOLVER"), (EX, "SIGSVGD_FLAG_EXACT_ADJOINT"),
                                        (NT, "SIGSVGD_FLAG_NAN_TAILS")])
def test_the_three_forbidden_pairs_say_unsupported_and_name_both_flags(other, name):
    g, L = GEO, lib()
    geo = (g["A"], g["B"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, LK | other)
    pgeo = (g["A"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, LK | other)
    two = (g["A"], g["B"], g["TX"], g["TY"], g["d"], g["n"], 0)
    w, grid, lds = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    calls = [
        lambda: L.sigsvgd_gram_long_fwd_bwd2(FAKE, FAKE, *geo, None, FAKE, FAKE, FAKE, FAKE, 1 << 30, None),
        lambda: L.sigsvgd_gram_long_fwd_bwd2(FAKE, FAKE, *geo, None, FAKE, None, None, FAKE, 1 << 30, None),
        lambda: _ws("gram_long2_workspace_bytes", *two, 1, 1, LK | other)[0],
        lambda: _ws("gram_long2_workspace_bytes", *two, 0, 0, LK | other)[0],
        lambda: L.sigsvgd_pair_fwd(FAKE, FAKE, *pgeo, FAKE, FAKE, 1 << 30, None),
        lambda: L.sigsvgd_pair_fwd_bwd(FAKE, FAKE, *pgeo, None, FAKE, FAKE, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("pair_workspace_bytes", g["A"], g["TX"], g["TY"], g["d"], g["n"], 0, 1, LK | other)[0],
        lambda: _ws("pair_workspace_bytes", g["A"], g["TX"], g["TY"], g["d"], g["n"], 0, 0, LK | other)[0],
        lambda: L.sigsvgd_pair_schedule(g["A"], g["TX"], g["TY"], g["d"], g["n"], 0, 1, LK | other, ctypes.byref(w),
                                        ctypes.byref(grid), ctypes.byref(lds)),
    ]
    for k, call in enumerate(calls):
        assert call() == UNSUPPORTED, (k, _lib.last_error())
        assert NAME in _lib.last_error() and name in _lib.last_error(), (k, _lib.last_error())


def test_flagged_workspace_is_at_least_the_unflagged():
    """the block exponents: (bands x blocks of 64 steps) ints per wave, which a forward-only launch keeps too"""
    for (A, B, TX, TY, d, n) in [(3, 3, 300, 300, 2, 0), (2, 5, 70, 131, 3, 1), (100, 70, 40, 30, 2, 0)]:
        for gx, gy, f in [(1, 1, 0), (1, 0, 0), (0, 1, 0), (0, 0, 0), (1, 0, YX), (0, 0, YX), (1, 0, YX | SYM)]:
            if (f & YX) and (A != B or TX != TY):
                continue
            rc0, b0 = _ws("gram_long2_workspace_bytes", A, B, TX, TY, d, n, 0, gx, gy, f)
            rc1, b1 = _ws("gram_long2_workspace_bytes", A, B, TX, TY, d, n, 0, gx, gy, f | LK)
            assert rc0 == OK and rc1 == OK and b1 >= b0 and b1 > 0, (A, B, gx, gy, f, b0, b1, _lib.last_error())
        for want in (0, 1):
            rc0, b0 = _ws("pair_workspace_bytes", A, TX, TY, d, n, 0, want, 0)
            rc1, b1 = _ws("pair_workspace_bytes", A, TX, TY, d, n, 0, want, LK)
            assert rc0 == OK and rc1 == OK and b1 >= b0 and b1 > 0, (A, want, b0, b1)


def test_flagged_paired_launches_run_one_wave_per_pair():
    """a shape whose unflagged schedule deals a pair's bands to a workgroup: with the bit it is one wavefront per pair"""
    L = lib()
    w, grid, lds = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    out = (ctypes.byref(w), ctypes.byref(grid), ctypes.byref(lds))
    waves, ldsb = {}, {}
    for want in (0, 1):
        for f in (0, LK):
            assert L.sigsvgd_pair_schedule(6, 1024, 1024, 4, 0, 0, want, f, *out) == OK, _lib.last_error()
            waves[want, f], ldsb[want, f] = w.value, lds.value
    assert waves[0, 0] > 1 and waves[1, 0] > 1, waves
    assert waves[0, LK] == 1 and waves[1, LK] == 1, waves
    assert ops.pair_schedule(6, 1024, 1024, 4, log_k=True)[0] == 1
    # the one-wavefront kernel's LDS and one int per block of 64 steps (+ 1, rounded to 8 bytes)
    plain = ((64 * 128 + 1023 + 2 + 64 + 65 * 4) * 8)
    assert ldsb[1, LK] == plain + ((1023 + 63 + 63) // 64 + 1) * 4


def test_other_entry_points_answer_as_before():
    """every entry point outside the accepting six keeps its answer for bit 1024: an unknown flag bit where it checks its flags,
    no effect where it does not"""
    g, L = GEO, lib()
    geo = (g["A"], g["B"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, LK)
    pgeo = (g["A"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, LK)
    two = (g["A"], g["B"], g["TX"], g["TY"], g["d"], g["n"], 0)
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    calls = [
        lambda: L.sigsvgd_gram_long_fwd(FAKE, FAKE, *geo, FAKE, FAKE, 1 << 30, None),
        lambda: L.sigsvgd_gram_long_fwd_bwd(FAKE, FAKE, *geo, None, FAKE, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("gram_long_workspace_bytes", *two, 1, LK)[0],
        lambda: L.sigsvgd_gram_long_fwd_bwd_h(FAKE, FAKE, *geo, None, FAKE, FAKE, None, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("gram_long_h_workspace_bytes", *two, 1, 0, LK)[0],
        lambda: L.sigsvgd_pair_fwd_bwd_h(FAKE, FAKE, *pgeo, None, FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("pair_h_workspace_bytes", g["A"], g["TX"], g["TY"], g["d"], g["n"], 0, LK)[0],
        lambda: L.sigsvgd_gram_long_sym_partial(FAKE, 64, 300, 2, _lib.F64, 1.0, 0, 0, LK, 0, 2, None, FAKE, FAKE, FAKE,
                                                1 << 30, None),
        lambda: L.sigsvgd_gram_long_partial_plan(64, 300, 2, 0, 0, LK, 2, ctypes.byref(r), ctypes.byref(c)),
        lambda: _ws("gram_long_partial_workspace_bytes", 64, 300, 2, 0, 0, LK, 0, 2)[0],
        lambda: _ws("pde_workspace_bytes", 4, 30, 20, 1, 1, LK)[0],
        lambda: L.sigsvgd_pde_fwd(FAKE, 4, 30, 20, _lib.F64, 1, LK, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("sqdist_select_workspace_bytes", 4, 4, 9, 9, 2, LK)[0],
    ]
    for k, call in enumerate(calls):
        assert call() == BADARG, (k, _lib.last_error())
        assert "0x400" in _lib.last_error(), (k, _lib.last_error())
    assert _ws("gram_workspace_bytes", 8, 8, 32, 2, 0, 0, 1, LK) == _ws("gram_workspace_bytes", 8, 8, 32, 2, 0, 0, 1, 0)


# ---- (c) the Python layer --------------------------------------------------------------------------------------------------------
A, B, T, TY, D = 5, 4, 6, 5, 2
LKW = {"log_k": True}


class Recorder:
    """stands in for the launches and queries of `ops` a log-domain call may reach; every other launch raises"""

    def __init__(self, takes=True):
        self.takes, self.launches, self.queries = takes, [], []

    def _note(self, name, X, Y, kw, grad_out=None, **flags):
        self.launches.append((name, tuple(X.shape), tuple(Y.shape), X.data_ptr() == Y.data_ptr(),
                              " ".join(k for k, v in flags.items() if v), dict(kw),
                              None if grad_out is None else grad_out.clone()))

    def gram_long2_takes(self, A, B, TX, TY, d, dyadic_order=0, static_kind=0, want_gradX=True, want_gradY=True, y_is_x=False,
                         **kw):
        self.queries.append(("gram_long2_takes", dict(kw)))
        return self.takes

    def pair_takes(self, A, TX, TY, d, dyadic_order=0, static_kind=0, want_grad=True, **kw):
        self.queries.append(("pair_takes", dict(kw)))
        return self.takes

    def gram_long_fwd_bwd2(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False,
                           y_is_x=False, want_gradX=True, want_gradY=True, **kw):
        self._note("gram_long_fwd_bwd2", X, Y, kw, grad_out, sym=sym, yx=y_is_x, gx=want_gradX, gy=want_gradY,
                   w=grad_out is not None)
        return (torch.zeros(X.shape[0], Y.shape[0], dtype=X.dtype), torch.ones_like(X) if want_gradX else None,
                torch.ones_like(Y) if want_gradY and not (sym or y_is_x) else None)

    def pair_fwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, naive=False, **kw):
        self._note("pair_fwd", X, Y, kw)
        return torch.zeros(X.shape[0], dtype=X.dtype)

    def pair_fwd_bwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, want_x=True, want_y=True,
                     **kw):
        self._note("pair_fwd_bwd", X, Y, kw, grad_out, gx=want_x, gy=want_y, w=grad_out is not None)
        return (torch.zeros(X.shape[0], dtype=X.dtype), torch.ones_like(X) if want_x else None,
                torch.ones_like(Y) if want_y else None)

    def install(self, monkeypatch):
        def refuse(name):
            def f(*a, **k):
                raise AssertionError(f"ops.{name} reached by a log-domain call")
            return f

        for name in ("gram_takes", "gram_fwd", "gram_fwd_bwd", "gram_long_fwd", "gram_long_fwd_bwd", "gram_long_fwd_bwd_h",
                     "pair_fwd_bwd_h", "path_sqdist_select", "pde_fwd_bwd"):
            monkeypatch.setattr(ops, name, refuse(name))
        for name in ("gram_long2_takes", "pair_takes", "gram_long_fwd_bwd2", "pair_fwd", "pair_fwd_bwd"):
            monkeypatch.setattr(ops, name, getattr(self, name))
        return self


def paths(n, t, grad, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, t, D, dtype=torch.float64, generator=g).requires_grad_(grad)


def brief(rec):
    return [c[:6] for c in rec.launches]


def test_normalized_gram_issues_the_listed_launches(monkeypatch):
    rec = Recorder().install(monkeypatch)
    kernel = sk.SigKernel(sk.RBFKernel(1.0), 0, normalize=True)
    X, Y = paths(A, T, True), paths(B, TY, True, 1)
    G = torch.arange(1.0, A * B + 1).reshape(A, B).double()
    K = kernel.compute_Gram(X, Y, grad_Y=True)
    sx, sy = (A, T, D), (B, TY, D)
    assert brief(rec) == [("gram_long_fwd_bwd2", sx, sy, False, "", LKW), ("pair_fwd", sx, sx, True, "", LKW),
                          ("pair_fwd", sy, sy, True, "", LKW)]
    assert torch.equal(K, torch.ones(A, B).double())  # (the recorder's logarithms are zeros)
    rec.launches.clear()
    (K * G).sum().backward()
    assert brief(rec) == [("gram_long_fwd_bwd2", sx, sy, False, "gx gy w", LKW), ("pair_fwd_bwd", sx, sx, True, "gx gy w", LKW),
                          ("pair_fwd_bwd", sy, sy, True, "gx gy w", LKW)]
    W = G * K.detach()
    assert torch.equal(rec.launches[0][6], W) and torch.equal(rec.launches[1][6], -0.5 * W.sum(1))
    assert torch.equal(rec.launches[2][6], -0.5 * W.sum(0))
    assert torch.equal(X.grad, 3 * torch.ones_like(X)) and torch.equal(Y.grad, 3 * torch.ones_like(Y))  # cross + both slots
    assert rec.queries == [("gram_long2_takes", LKW)]
    # without grad_Y, Y gets nothing and its paired launch is not issued
    rec.launches.clear()
    X.grad = Y.grad = None
    kernel.compute_Gram(X, Y).sum().backward()
    assert [c[0] for c in rec.launches] == ["gram_long_fwd_bwd2", "pair_fwd", "pair_fwd", "gram_long_fwd_bwd2", "pair_fwd_bwd"]
    assert rec.launches[3][4] == "gx w" and Y.grad is None


def test_one_tensor_in_both_slots_takes_one_paired_launch(monkeypatch):
    rec = Recorder().install(monkeypatch)
    kernel = sk.SigKernel(sk.IMQStaticKernel(2.0), 1, normalize=True)
    X = paths(A, T, True)
    sx = (A, T, D)
    G = torch.arange(1.0, A * A + 1).reshape(A, A).double()
    (kernel.compute_Gram(X, X, sym=True) * G).sum().backward()
    assert brief(rec) == [("gram_long_fwd_bwd2", sx, sx, True, "yx", LKW), ("pair_fwd", sx, sx, True, "", LKW),
                          ("gram_long_fwd_bwd2", sx, sx, True, "sym yx gx w", LKW), ("pair_fwd_bwd", sx, sx, True, "gx gy w", LKW)]
    assert torch.equal(rec.launches[3][6], -0.5 * (G.sum(1) + G.sum(0)))  # the two contributions add
    rec.launches.clear()
    X.grad = None
    (kernel.compute_Gram(X, X, grad_Y=True) * G).sum().backward()  # both slots through autograd: every ordered pair
    assert brief(rec) == [("gram_long_fwd_bwd2", sx, sx, True, "yx", LKW), ("pair_fwd", sx, sx, True, "", LKW),
                          ("gram_long_fwd_bwd2", sx, sx, True, "gx gy w", LKW), ("pair_fwd_bwd", sx, sx, True, "gx gy w", LKW),
                          ("pair_fwd_bwd", sx, sx, True, "gx gy w", LKW)]
    assert torch.equal(X.grad, 6 * torch.ones_like(X))


def test_kernel_distance_mmd_and_log_methods(monkeypatch):
    rec = Recorder().install(monkeypatch)
    kernel = sk.SigKernel(sk.RBFKernel(1.0), 0, normalize=True)
    X, Y = paths(A, T, True), paths(A, TY, False, 1)
    kernel.compute_kernel(X, Y).sum().backward()
    assert [(c[0], c[2][1], c[3], c[4], c[5]) for c in rec.launches] == [
        ("pair_fwd_bwd", T, True, "gx gy", LKW), ("pair_fwd_bwd", TY, False, "gx", LKW), ("pair_fwd", TY, True, "", LKW)]
    rec.launches.clear()
    kernel.compute_distance(X.detach(), Y)
    assert all(c[0] == "pair_fwd" and c[5] == LKW for c in rec.launches) and len(rec.launches) == 5
    rec.launches.clear()
    kernel.compute_mmd(X.detach(), Y)
    assert [(c[0], c[4]) for c in rec.launches] == [("gram_long_fwd_bwd2", "yx"), ("pair_fwd", ""),
                                                    ("gram_long_fwd_bwd2", "yx"), ("pair_fwd", ""),
                                                    ("gram_long_fwd_bwd2", ""), ("pair_fwd", ""), ("pair_fwd", "")]
    assert all(c[5] == LKW for c in rec.launches)
    # the logarithm itself, from a kernel with or without normalize
    for k in (kernel, sk.SigKernel(sk.RBFKernel(1.0), 0)):
        rec.launches.clear()
        Xg = paths(A, T, True)
        k.compute_log_Gram(Xg, Y).sum().backward()
        k.compute_log_kernel(Xg, Y).sum().backward()
        assert [(c[0], c[4], c[5]) for c in rec.launches] == [("gram_long_fwd_bwd2", "", LKW), ("gram_long_fwd_bwd2", "gx w", LKW),
                                                              ("pair_fwd_bwd", "gx", LKW)]


def test_without_normalize_no_keyword_reaches_ops(monkeypatch):
    """normalize=False, the default, reaches `ops` as it always did: recorders with the signatures from before the keyword"""
    seen = []

    def gram_takes(A, B, T, d, dyadic_order=0, static_kind=0, want_grad=True, naive=False, sym=False, y_is_x=False):
        return False

    def gram_long_fwd_bwd2(X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False, y_is_x=False,
                           want_gradX=True, want_gradY=True):
        seen.append("gram_long_fwd_bwd2")
        return torch.zeros(X.shape[0], Y.shape[0], dtype=X.dtype), torch.zeros_like(X), torch.zeros_like(Y)

    def pair_takes(A, TX, TY, d, dyadic_order=0, static_kind=0, want_grad=True):
        return True

    def pair_fwd_bwd(X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, want_x=True, want_y=True):
        seen.append("pair_fwd_bwd")
        return torch.zeros(X.shape[0], dtype=X.dtype), torch.zeros_like(X), torch.zeros_like(Y)

    for f in (gram_takes, gram_long_fwd_bwd2, pair_takes, pair_fwd_bwd):
        monkeypatch.setattr(ops, f.__name__, f)
    for kernel in (sk.SigKernel(sk.RBFKernel(1.0), 0), sk.SigKernel(sk.RBFKernel(1.0), 0, normalize=False)):
        X, Y = paths(A, T, True), paths(A, TY, True, 1)
        kernel.compute_Gram(X, Y, grad_Y=True).sum().backward()
        kernel.compute_kernel(X, Y).sum().backward()
    assert seen == ["gram_long_fwd_bwd2", "pair_fwd_bwd"] * 2


def test_errors_of_normalize(monkeypatch):
    from parity import DisguisedRBF

    rec = Recorder().install(monkeypatch)
    X, Y = paths(A, T, False), paths(B, TY, False, 1)
    with pytest.raises(ValueError, match="fp32_sweeps"):
        sk.SigKernel(sk.IMQStaticKernel(1.0), 0, fp32_sweeps=True, normalize=True)
    with pytest.raises(NotImplementedError, match="exact_grad"):
        sk.SigKernel(sk.RBFKernel(1.0), 0, exact_grad=True, normalize=True)
    with pytest.raises(NotImplementedError, match="_naive_solver"):
        sk.SigKernel(sk.RBFKernel(1.0), 0, _naive_solver=True, normalize=True)
    rbf = sk.SigKernel(sk.RBFKernel(1.0), 0, normalize=True)
    for call in (lambda: rbf.compute_Gram(X, Y, lengths_X=[6, 1, 3, 2, 5]), lambda: rbf.compute_kernel(X, X, [6, 1, 3, 2, 5]),
                 lambda: rbf.compute_distance(X, X, [6, 1, 3, 2, 5], [6, 1, 3, 2, 5]),
                 lambda: rbf.compute_mmd(X, Y, lengths_Y=[5, 2, 1, 4])):
        with pytest.raises(NotImplementedError, match="lengths"):
            call()
    learned = sk.SigKernel(sk.RBFKernel(torch.tensor(1.0, requires_grad=True)), 0, normalize=True)
    for call in (lambda: learned.compute_Gram(X, Y), lambda: learned.compute_kernel(X, X), lambda: learned.compute_log_Gram(X, Y)):
        with pytest.raises(NotImplementedError, match="sigma that requires grad"):
            call()
    user = sk.SigKernel(DisguisedRBF(1.0), 0, normalize=True)
    for call in (lambda: user.compute_Gram(X, Y), lambda: user.compute_kernel(X, X), lambda: user.compute_mmd(X, Y)):
        with pytest.raises(NotImplementedError, match="user static kernel"):
            call()
    for plain in (sk.SigKernel(sk.RBFKernel(1.0), 0, exact_grad=True), sk.SigKernel(sk.RBFKernel(1.0), 0, _naive_solver=True)):
        with pytest.raises(NotImplementedError, match="default stencil"):
            plain.compute_log_Gram(X, Y)
    assert rec.launches == [] and rec.queries == []
    # shapes the long route refuses
    rec.takes = False
    monkeypatch.setattr(_lib, "last_error", lambda: "refused")
    with pytest.raises(NotImplementedError, match="the log-domain solve"):
        rbf.compute_Gram(X, Y)
    with pytest.raises(NotImplementedError, match="the log-domain solve"):
        rbf.compute_kernel(X, X)
    with pytest.raises(NotImplementedError, match="the log-domain solve"):
        rbf.compute_log_kernel(X, X)
    assert rec.launches == []


# ---- (d) the algebra of the normalisation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("same", [False, True])
def test_normalisation_algebra_against_torch_autograd(same):
    """exp(l - a / 2 - b / 2) and its gradient from one weighted launch of grad ln K and one paired launch per batch, fed with
    the reference's numbers at A = 3, B = 2, T = 9, d = 2, against torch autograd through K / sqrt(K_xx K_yy) of the oracle"""
    X = R.walks(1, 3, 9, 2, 0.5)
    Y = X if same else R.walks(2, 2, 9, 2, 0.5)
    G = np.random.default_rng(3).standard_normal((3, len(Y)))
    Khat, gX, gY = R.normalized_gram_and_grads(X, Y, G, same=same)
    Xt = torch.tensor(X, requires_grad=True)
    Yt = Xt if same else torch.tensor(Y, requires_grad=True)
    ref = R.normalized_torch(Xt, Yt)
    (torch.tensor(G) * ref).sum().backward()
    assert np.abs(Khat - ref.detach().numpy()).max() < 1e-13
    assert np.abs(gX - Xt.grad.numpy()).max() < 1e-12 * np.abs(gX).max()
    if same:
        assert np.array_equal(np.diagonal(Khat), np.ones(3))
    else:
        assert np.abs(gY - Yt.grad.numpy()).max() < 1e-12 * np.abs(gY).max()
