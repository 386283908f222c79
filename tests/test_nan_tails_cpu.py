"""Variable-length batches on the long route (SIGSVGD_FLAG_NAN_TAILS) without a device: the host side
of the C ABI (every acceptance and refusal of the flag returns before any device work), the property the feature rests on
(padding with the last point is exact) on the numpy oracle, and where `lengths_X` / `lengths_Y` go in the Python layer, with
recorders in the style of tests/test_gram_routing_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import nan_tails_reference as R
import sigsvgd_amd.sigkernel as sk
from cabi import BADARG, FAKE, OK, UNSUPPORTED, WORKSPACE, exported_symbols, lib
from oracle import sigkernel_oracle as O
from sigsvgd_amd import _lib, ops

NT, EX, NV, YX, SYM = (_lib.FLAG_NAN_TAILS, _lib.FLAG_EXACT_ADJOINT, _lib.FLAG_NAIVE_SOLVER, _lib.FLAG_Y_IS_X, _lib.FLAG_SYM)
GEO = dict(A=3, B=3, TX=300, TY=300, d=2, n=0)
NAME = "SIGSVGD_FLAG_NAN_TAILS"


def _ws(name, *args):
    b = ctypes.c_size_t(12345)
    rc = getattr(lib(), "sigsvgd_" + name)(*args, ctypes.byref(b))
    return rc, b.value


# ---- the reference helpers ---------------------------------------------------------------------------------------------------
def test_reference_helpers():
    paths = R.rough_paths(0, [3, 1, 5], 2)
    Xn, Xl = R.pad_nan(paths, 5), R.pad_last(paths, 5)
    assert R.lengths(Xn).tolist() == [3, 1, 5] and R.lengths(Xl).tolist() == [5, 5, 5]
    assert np.isnan(Xn[0, 3:]).all() and np.array_equal(Xl[1], np.repeat(paths[1], 5, axis=0))
    g = np.arange(30.0).reshape(3, 5, 2)
    f = R.fold(g, [3, 1, 5])
    assert np.array_equal(f[0, 2], g[0, 2:].sum(0)) and not f[0, 3:].any() and np.array_equal(f[2], g[2])
    assert np.array_equal(f[1, 0], g[1].sum(0)) and f.sum() == g.sum()


# ---- the host side of the C ABI ------------------------------------------------------------------------------------------------
def test_abi_is_still_version_10_with_39_exports():
    assert lib().sigsvgd_abi_version() == _lib.ABI_VERSION == 10
    assert len(exported_symbols()) == len(_lib.EXPORTS) == 39
    assert _lib.FLAG_NAN_TAILS == 512
    assert ops._flags(False, False, False, False, nan_tails=True) == 512
    assert ops._flags(True, True, True, False, nan_tails=True) == 1 | 2 | 4 | 512
    assert ops._flags(True, True, True, True, True, True, True) == 1 | 2 | 4 | 8 | 32 | 128 | 256  # (as before the keyword)


def test_accepting_entry_points_take_the_flag():
    """every accepting entry point passes its flag check with the bit: the refusal it then gives is the next check's (a
    workspace of 0 bytes, before any device work), not BADARG.  A forward-only flagged launch needs a workspace too: the
    lengths."""
    g, L = GEO, lib()
    for extra in (0, NV):
        geo = lambda f: (g["A"], g["B"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, NT | extra | f)
        pgeo = (g["A"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, NT | extra)
        for gx, gy, f in [(None, None, 0), (FAKE, None, 0), (None, FAKE, 0), (FAKE, FAKE, 0), (FAKE, None, YX),
                          (FAKE, None, YX | SYM), (None, None, YX), (FAKE, None, SYM)]:
            assert L.sigsvgd_gram_long_fwd_bwd2(FAKE, FAKE, *geo(f), FAKE, FAKE, gx, gy, None, 0, None) == WORKSPACE, \
                _lib.last_error()
        assert L.sigsvgd_pair_fwd(FAKE, FAKE, *pgeo, FAKE, None, 0, None) == WORKSPACE, _lib.last_error()
        for gx, gy in [(FAKE, FAKE), (FAKE, None), (None, FAKE)]:
            assert L.sigsvgd_pair_fwd_bwd(FAKE, FAKE, *pgeo, None, FAKE, gx, gy, None, 0, None) == WORKSPACE, _lib.last_error()
    # every kind with the default stencil
    for kind in (0, 1, 2, 3, 6, 7):
        assert _ws("gram_long2_workspace_bytes", 3, 3, 300, 300, 2, 0, kind, 1, 1, NT)[0] == OK, _lib.last_error()
        assert _ws("pair_workspace_bytes", 3, 300, 300, 2, 0, kind, 1, NT)[0] == OK, _lib.last_error()
    # an unknown bit beside it is still refused, and so is NAIVE_SOLVER where the kind has the default stencil only
    assert _ws("gram_long2_workspace_bytes", 3, 3, 300, 300, 2, 0, 0, 1, 1, NT | _lib.FLAG_WS_CLEAN)[0] == BADARG
    assert _ws("pair_workspace_bytes", 3, 300, 300, 2, 0, 0, 1, NT | SYM)[0] == BADARG
    assert _ws("pair_workspace_bytes", 3, 300, 300, 2, 0, 2, 1, NT | NV)[0] == UNSUPPORTED


def _aligned(nbytes):
    return (nbytes + 255) // 256 * 256


@pytest.mark.parametrize("extra", [0, NV])
def test_workspace_grows_by_the_aligned_length_arrays(extra):
    """flagged queries are OK and give the unflagged bytes plus the int arrays of the lengths padded to 256 B (one array with
    Y_IS_X), plus the 256 B of pointer alignment where the unflagged launch needs no workspace at all"""
    g = GEO
    two = (g["A"], g["B"], g["TX"], g["TY"], g["d"], g["n"], 0)
    for gx, gy, f, n_int in [(1, 1, 0, 6), (1, 0, 0, 6), (0, 1, 0, 6), (0, 0, 0, 6), (1, 0, YX, 3), (0, 0, YX, 3),
                             (1, 0, YX | SYM, 3)]:
        rc0, b0 = _ws("gram_long2_workspace_bytes", *two, gx, gy, extra | f)
        rc1, b1 = _ws("gram_long2_workspace_bytes", *two, gx, gy, extra | f | NT)
        assert rc0 == OK and rc1 == OK, _lib.last_error()
        assert b1 >= b0 and b1 == b0 + _aligned(4 * n_int) + (0 if b0 else 256), (gx, gy, f, b0, b1)
    for want in (0, 1):
        rc0, b0 = _ws("pair_workspace_bytes", g["A"], g["TX"], g["TY"], g["d"], g["n"], 0, want, extra)
        rc1, b1 = _ws("pair_workspace_bytes", g["A"], g["TX"], g["TY"], g["d"], g["n"], 0, want, extra | NT)
        assert rc0 == OK and rc1 == OK, _lib.last_error()
        assert b1 >= b0 and b1 == b0 + _aligned(4 * 2 * g["A"]) + (0 if b0 else 256), (want, b0, b1)
    # more paths than one 256-B block of lengths holds
    b0, b1 = (_ws("gram_long2_workspace_bytes", 100, 70, 40, 30, 2, 0, 0, 1, 1, f)[1] for f in (0, NT))
    assert b1 == b0 + _aligned(4 * 170)


def test_flagged_paired_launches_run_one_wave_per_pair():
    """a shape whose unflagged schedule deals a pair's bands to a workgroup: with the bit it is one wavefront per pair"""
    L = lib()
    w, grid, lds = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    out = (ctypes.byref(w), ctypes.byref(grid), ctypes.byref(lds))
    waves = {}
    for want in (0, 1):
        for f in (0, NT):
            assert L.sigsvgd_pair_schedule(6, 1024, 1024, 4, 0, 0, want, f, *out) == OK, _lib.last_error()
            waves[want, f] = w.value
    assert waves[0, 0] > 1 and waves[1, 0] > 1, waves
    assert waves[0, NT] == 1 and waves[1, NT] == 1, waves


def test_entry_points_without_the_kernels_say_unsupported():
    g, L = GEO, lib()
    geo = (g["A"], g["B"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, NT)
    pgeo = (g["A"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, NT)
    two = (g["A"], g["B"], g["TX"], g["TY"], g["d"], g["n"], 0)
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    calls = [
        lambda: L.sigsvgd_gram_long_fwd(FAKE, FAKE, *geo, FAKE, FAKE, 1 << 30, None),
        lambda: L.sigsvgd_gram_long_fwd_bwd(FAKE, FAKE, *geo, None, FAKE, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("gram_long_workspace_bytes", *two, 0, NT)[0],
        lambda: _ws("gram_long_workspace_bytes", *two, 1, NT)[0],
        lambda: L.sigsvgd_gram_long_fwd_bwd_h(FAKE, FAKE, *geo, None, FAKE, FAKE, None, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("gram_long_h_workspace_bytes", *two, 1, 0, NT)[0],
        lambda: L.sigsvgd_pair_fwd_bwd_h(FAKE, FAKE, *pgeo, None, FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("pair_h_workspace_bytes", g["A"], g["TX"], g["TY"], g["d"], g["n"], 0, NT)[0],
        lambda: L.sigsvgd_gram_long_sym_partial(FAKE, 64, 300, 2, _lib.F64, 1.0, 0, 0, NT, 0, 2, None, FAKE, FAKE, FAKE,
                                                1 << 30, None),
        lambda: L.sigsvgd_gram_long_partial_plan(64, 300, 2, 0, 0, NT, 2, ctypes.byref(r), ctypes.byref(c)),
        lambda: _ws("gram_long_partial_workspace_bytes", 64, 300, 2, 0, 0, NT, 0, 2)[0],
    ]
    for k, call in enumerate(calls):
        assert call() == UNSUPPORTED, (k, _lib.last_error())
        assert NAME in _lib.last_error(), (k, _lib.last_error())


def test_the_flag_with_the_exact_adjoint_says_unsupported():
    g, L = GEO, lib()
    geo = (g["A"], g["B"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, NT | EX)
    pgeo = (g["A"], g["TX"], g["TY"], g["d"], _lib.F64, 1.0, g["n"], 0, NT | EX)
    two = (g["A"], g["B"], g["TX"], g["TY"], g["d"], g["n"], 0)
    w, grid, lds = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    calls = [
        lambda: L.sigsvgd_gram_long_fwd_bwd2(FAKE, FAKE, *geo, None, FAKE, FAKE, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("gram_long2_workspace_bytes", *two, 1, 1, NT | EX)[0],
        lambda: L.sigsvgd_pair_fwd_bwd(FAKE, FAKE, *pgeo, None, FAKE, FAKE, FAKE, FAKE, 1 << 30, None),
        lambda: _ws("pair_workspace_bytes", g["A"], g["TX"], g["TY"], g["d"], g["n"], 0, 1, NT | EX)[0],
        lambda: L.sigsvgd_pair_schedule(g["A"], g["TX"], g["TY"], g["d"], g["n"], 0, 1, NT | EX, ctypes.byref(w),
                                        ctypes.byref(grid), ctypes.byref(lds)),
    ]
    for k, call in enumerate(calls):
        assert call() == UNSUPPORTED, (k, _lib.last_error())
        assert NAME in _lib.last_error() and "SIGSVGD_FLAG_EXACT_ADJOINT" in _lib.last_error(), (k, _lib.last_error())


def test_other_routes_answer_as_before():
    """the entry points outside the long route's Gram and paired modes keep the answer they had for bit 512: an unknown flag
    bit where they check their flags (the PDE launches), no effect where they do not (the fused Gram launches' queries)"""
    L = lib()
    assert _ws("pde_workspace_bytes", 4, 30, 20, 1, 1, NT)[0] == BADARG and "0x200" in _lib.last_error()
    assert L.sigsvgd_pde_fwd(FAKE, 4, 30, 20, _lib.F64, 1, NT, FAKE, FAKE, 1 << 30, None) == BADARG
    assert _ws("gram_workspace_bytes", 8, 8, 32, 2, 0, 0, 1, NT) == _ws("gram_workspace_bytes", 8, 8, 32, 2, 0, 0, 1, 0)
    assert _ws("sqdist_select_workspace_bytes", 4, 4, 9, 9, 2, NT)[0] == BADARG


# ---- the property the feature rests on -------------------------------------------------------------------------------------------
# (T, pairs of lengths): the issue's T = 20 and the T = 131 of the device tests, short against long both ways round
PROPERTY_CASES = [(20, [(20, 7), (3, 20), (11, 13), (2, 2)]), (131, [(131, 9), (65, 130), (2, 131), (66, 8)])]


@pytest.mark.parametrize("n", [0, 1, 2])
@pytest.mark.parametrize("T,pairs", PROPERTY_CASES)
def test_last_point_padding_is_exact_on_the_oracle(T, pairs, n):
    """K of the last-point-padded pair against K of the truncated pair within 1e-12 per entry, the padded gradient folded onto
    the end point within 1e-12 of the truncated gradient's largest entry (rough walks: steps of 0.5, bandwidth 1).  Measured
    on these cases, orders 0 to 2: at most 4.6e-14 / 4.8e-15 at T = 20 and 1.8e-13 / 2.3e-14 at T = 131, so the bound of
    1e-12 holds at T = 131 too and is not widened."""
    worst_K = worst_g = 0.0
    for k, (LX, LY) in enumerate(pairs):
        (x,), (y,) = R.rough_paths(100 * T + k, [LX], 2, dtype=np.float64), R.rough_paths(100 * T + k + 50, [LY], 2,
                                                                                        dtype=np.float64)
        Kt, gt = O.gram_backward(x[None], y[None], None, O.RBF, 1.0, n)
        Kp, gp = O.gram_backward(R.pad_last([x], T), R.pad_last([y], T), None, O.RBF, 1.0, n)
        worst_K = max(worst_K, float(np.abs(Kp - Kt).max() / np.abs(Kt).max()))
        worst_g = max(worst_g, float(np.abs(R.fold(gp, [LX])[0, :LX] - gt[0]).max() / np.abs(gt).max()))
    print(f"T={T} n={n}: K {worst_K:.2e}, folded gradient {worst_g:.2e}")
    assert worst_K < 1e-12 and worst_g < 1e-12


# ---- the Python layer ----------------------------------------------------------------------------------------------------------
A, B, T, TY, D = 5, 4, 6, 5, 2
LX, LY = [6, 1, 3, 2, 5], [5, 2, 1, 4]


class Recorder:
    """stands in for the launches and queries of `ops` a call with lengths may reach; every other launch raises"""

    def __init__(self, takes=True):
        self.takes, self.launches, self.queries = takes, [], []

    def _note(self, name, X, Y, kw, **flags):
        self.launches.append((name, R.lengths(X.detach().numpy()).tolist(), R.lengths(Y.detach().numpy()).tolist(),
                              X.data_ptr() == Y.data_ptr(),  # (one padded tensor in both slots)
                              " ".join(k for k, v in flags.items() if v), dict(kw)))

    def gram_long2_takes(self, A, B, TX, TY, d, dyadic_order=0, static_kind=0, want_gradX=True, want_gradY=True, y_is_x=False,
                         **kw):
        self.queries.append(("gram_long2_takes", dict(kw)))
        return self.takes

    def pair_takes(self, A, TX, TY, d, dyadic_order=0, static_kind=0, want_grad=True, **kw):
        self.queries.append(("pair_takes", dict(kw)))
        return self.takes

    def gram_long_fwd_bwd2(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False,
                           y_is_x=False, want_gradX=True, want_gradY=True, **kw):
        self._note("gram_long_fwd_bwd2", X, Y, kw, sym=sym, yx=y_is_x, gx=want_gradX, gy=want_gradY, w=grad_out is not None)
        return (torch.zeros(X.shape[0], Y.shape[0], dtype=X.dtype), torch.ones_like(X) if want_gradX else None,
                torch.ones_like(Y) if want_gradY else None)

    def pair_fwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, naive=False, **kw):
        self._note("pair_fwd", X, Y, kw)
        return torch.zeros(X.shape[0], dtype=X.dtype)

    def pair_fwd_bwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, want_x=True, want_y=True,
                     **kw):
        self._note("pair_fwd_bwd", X, Y, kw, gx=want_x, gy=want_y)
        return (torch.zeros(X.shape[0], dtype=X.dtype), torch.ones_like(X) if want_x else None,
                torch.ones_like(Y) if want_y else None)

    def install(self, monkeypatch):
        def refuse(name):
            def f(*a, **k):
                raise AssertionError(f"ops.{name} reached by a call with lengths")
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


NTKW = {"nan_tails": True}


@pytest.mark.parametrize("as_tensor", [False, True])
def test_compute_gram_with_lengths_is_the_flagged_two_sided_launch(monkeypatch, as_tensor):
    rec = Recorder().install(monkeypatch)
    kernel = sk.SigKernel(sk.RBFKernel(1.0), 0)
    lx, ly = (torch.tensor(LX), torch.tensor(LY, dtype=torch.int32)) if as_tensor else (LX, tuple(LY))
    X, Y = paths(A, T, True), paths(B, TY, True, 1)
    K = kernel.compute_Gram(X, Y, grad_Y=True, lengths_X=lx, lengths_Y=ly)
    (K * torch.arange(1.0, A * B + 1).reshape(A, B).double()).sum().backward()
    assert rec.launches == [("gram_long_fwd_bwd2", LX, LY, False, "gx gy", NTKW),
                            ("gram_long_fwd_bwd2", LX, LY, False, "gx gy w", NTKW)]
    assert rec.queries == [("gram_long2_takes", NTKW)] * 2
    # the gradient reaches the kept entries only (the recorder's gradient is all ones)
    keep = torch.arange(T)[None, :] < torch.tensor(LX)[:, None]
    assert torch.equal(X.grad != 0, keep[:, :, None].expand_as(X))
    assert torch.equal(Y.grad != 0, (torch.arange(TY)[None, :] < torch.tensor(LY)[:, None])[:, :, None].expand_as(Y))


def test_one_tensor_in_both_slots_is_padded_once(monkeypatch):
    rec = Recorder().install(monkeypatch)
    kernel = sk.SigKernel(sk.RBFKernel(1.0), 1)
    X = paths(A, T, True)
    kernel.compute_Gram(X, X, sym=True, lengths_X=LX, lengths_Y=list(LX)).sum().backward()
    kernel.compute_Gram(X.detach(), X.detach(), lengths_X=LX, lengths_Y=LX)
    kernel.compute_Gram(X.detach(), X.detach(), lengths_X=LX)  # (Y whole: two batches)
    assert rec.launches == [("gram_long_fwd_bwd2", LX, LX, True, "sym yx gx", NTKW),
                            ("gram_long_fwd_bwd2", LX, LX, True, "yx", NTKW),
                            ("gram_long_fwd_bwd2", LX, [T] * A, False, "", NTKW)]


def test_compute_kernel_distance_and_mmd_with_lengths(monkeypatch):
    rec = Recorder().install(monkeypatch)
    kernel = sk.SigKernel(sk.IMQStaticKernel(2.0), 0)
    X, Y = paths(A, T, True), paths(A, TY, False, 1)
    ly = LY + [3]
    kernel.compute_kernel(X, Y, LX, ly).sum().backward()
    kernel.compute_kernel(X.detach(), Y, LX, ly)
    assert rec.launches == [("pair_fwd_bwd", LX, ly, False, "gx", NTKW), ("pair_fwd", LX, ly, False, "", NTKW)]
    assert rec.queries == [("pair_takes", NTKW)] * 2
    rec.launches.clear()
    kernel.compute_distance(X.detach(), Y, LX, ly)
    assert rec.launches == [("pair_fwd", LX, LX, True, "", NTKW), ("pair_fwd", ly, ly, True, "", NTKW),
                            ("pair_fwd", LX, ly, False, "", NTKW)]
    rec.launches.clear()
    Yg = paths(A, TY, True, 1)
    kernel.compute_mmd(X, Yg, grad_Y=True, lengths_X=LX, lengths_Y=ly).backward()
    assert [(c[0], c[1], c[2], c[3], c[4]) for c in rec.launches] == [
        ("gram_long_fwd_bwd2", LX, LX, True, "sym yx gx"), ("gram_long_fwd_bwd2", ly, ly, True, "sym yx gx"),
        ("gram_long_fwd_bwd2", LX, ly, False, "gx gy")]
    assert all(c[5] == NTKW for c in rec.launches)


def test_without_lengths_no_keyword_reaches_ops(monkeypatch):
    """a call without lengths reaches `ops` as it always did: recorders with the signatures from before the keyword"""
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
    kernel = sk.SigKernel(sk.RBFKernel(1.0), 0)
    X, Y = paths(A, T, True), paths(A, TY, True, 1)
    kernel.compute_Gram(X, Y, grad_Y=True).sum().backward()
    kernel.compute_kernel(X, Y).sum().backward()
    assert seen == ["gram_long_fwd_bwd2", "pair_fwd_bwd"]


def test_errors_of_a_call_with_lengths(monkeypatch):
    from sigsvgd_amd.kernels import BatchGaussianKernel
    from parity import DisguisedRBF

    rec = Recorder().install(monkeypatch)
    X, Y = paths(A, T, False), paths(B, TY, False, 1)
    rbf = sk.SigKernel(sk.RBFKernel(1.0), 0)
    bad = [[6, 1, 3, 2], [6, 1, 3, 2, 7], [6, 0, 3, 2, 5], [6, 1.5, 3, 2, 5], torch.tensor([6.0, 1, 3, 2, 5]),
           torch.tensor([[6, 1, 3, 2, 5]]), [6, 1, 3, 2, True]]
    for lengths in bad:
        with pytest.raises(ValueError, match="lengths_X"):
            rbf.compute_Gram(X, Y, lengths_X=lengths)
    with pytest.raises(ValueError, match="lengths_Y"):
        rbf.compute_kernel(X, X, LX, [1, 2, 3, 4, 9])
    with pytest.raises(ValueError, match="sym=True"):
        rbf.compute_Gram(X, X, sym=True, lengths_X=LX, lengths_Y=[6, 1, 3, 2, 4])
    with pytest.raises(ValueError, match="sym=True"):
        rbf.compute_Gram(X, X, sym=True, lengths_X=LX)
    with pytest.raises(ValueError, match="fp32_sweeps"):
        sk.SigKernel(sk.IMQStaticKernel(1.0), 0, fp32_sweeps=True).compute_Gram(X, Y, lengths_X=LX)
    for static in (BatchGaussianKernel(), BatchGaussianKernel(bandwidth_fn=lambda sq: sq.mean())):
        with pytest.raises(ValueError, match="explicit bandwidth"):
            sk.SigKernel(static, 0).compute_Gram(X, Y, lengths_X=LX)
    with pytest.raises(NotImplementedError, match="exact_grad"):
        sk.SigKernel(sk.RBFKernel(1.0), 0, exact_grad=True).compute_Gram(X, Y, lengths_X=LX)
    with pytest.raises(NotImplementedError, match="sigma that requires grad"):
        sk.SigKernel(sk.RBFKernel(torch.tensor(1.0, requires_grad=True)), 0).compute_kernel(X, X, LX, LX)
    with pytest.raises(NotImplementedError, match="user static kernel"):
        sk.SigKernel(DisguisedRBF(1.0), 0).compute_Gram(X, Y, lengths_X=LX)
    assert rec.launches == [] and rec.queries == []
    # a constant bandwidth_fn is an explicit bandwidth
    sk.SigKernel(BatchGaussianKernel(bandwidth_fn=lambda _: 0.5), 0).compute_Gram(X, Y, lengths_X=LX)
    assert len(rec.launches) == 1
    # shapes the long route refuses
    rec.takes = False
    monkeypatch.setattr(_lib, "last_error", lambda: "refused")
    with pytest.raises(NotImplementedError, match="a batch with lengths"):
        rbf.compute_Gram(X, Y, lengths_X=LX)
    with pytest.raises(NotImplementedError, match="a batch with lengths"):
        rbf.compute_kernel(X, X, LX, LX)
