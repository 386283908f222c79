"""Variable-length batches on the long route (SIGSVGD_FLAG_NAN_TAILS) on the device.

Inputs are fp32-valued rough walks (steps of 0.5 per channel, bandwidth 1), NaN-padded to one length.  Every case asserts:
 1. the library takes the flag (before the feature it answered BADARG: these tests fail without it);
 2. each single pair, launched 1 x 1 with the flag, gives K, gX and gY bit for bit as the unflagged launch on the truncated
    tensors does (a pair with a one-point path: K = 1 exactly and no gradient);
 3. the whole launch against the pairs assembled from those 1 x 1 launches: K bit for bit, fp64-I/O gradients within 1e-9 of
    the largest entry (the project's figure for the same fp64 sums in another order, tests/test_gpu_long_partial.py);
 4. against the C oracle on the truncated pairs (RBF and linear, the kinds it has): K within 1e-9 per entry (fp64 I/O) or
    2^-23 (fp32 I/O), each gradient within 1e-5 of its largest entry;
 5. against the unflagged launch on the last-point-padded input: K within 1e-9 per entry, the folded gradient within 1e-5;
 6. rows >= L of every gradient are exact zeros, from outputs that held NaN before the launch;
 7. a second call gives the same bits.
Every launch of this file runs on an exactly sized, guarded workspace whose bytes are 0xFF before the launch, one byte past
a 256-B boundary (tests/guarded_workspace.py), and writes outputs that `ops` allocated NaN-filled."""
import numpy as np
import pytest
import torch

import nan_tails_reference as R
from guarded_workspace import GuardedWorkspace
from parity import np64, rel_entry, rel_max, signed_weights
from plans import device_cus, long2_plan, oracle_at_own_lengths
from sigsvgd_amd import _lib, ops

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
H = 1.0
RBF, LINEAR = _lib.STATIC_RBF, _lib.STATIC_LINEAR
_CACHED_WORKSPACE = ops._workspace  # (the autouse fixture below replaces it for every test)
KINDS = (_lib.STATIC_RBF, _lib.STATIC_LINEAR, _lib.STATIC_IMQ, _lib.STATIC_RQ, _lib.STATIC_MATERN32, _lib.STATIC_MATERN52)


class _NanEmptyTorch:
    """`torch` as `ops` sees it in this file: `torch.empty` gives floating tensors filled with NaN, so an output entry the
    launch does not write shows"""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def empty(*args, **kwargs):
        t = torch.empty(*args, **kwargs)
        return t.fill_(float("nan")) if t.is_floating_point() else t


@pytest.fixture(autouse=True)
def harness(monkeypatch):
    monkeypatch.setattr(ops, "torch", _NanEmptyTorch())
    ws = GuardedWorkspace("ones", 1).install(monkeypatch)
    yield ws
    ws.check()


def dev(a, io, gpu):
    return None if a is None else torch.as_tensor(np.asarray(a), device=gpu).to(io)


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int64 if a.dtype == F64 else torch.int32),
                                                                     b.view(torch.int64 if b.dtype == F64 else torch.int32))


def zero_tails(g, L):
    """rows >= L of every path's gradient are exact zeros, the rows before hold numbers"""
    g = np64(g)
    return all(not g[i, l:].any() and np.isfinite(g[i, :l]).all() for i, l in enumerate(L))


def pair_references(gpu, xs, ys, d, n, kind, naive, io):
    """per pair (i, j): the flagged 1 x 1 launch on the NaN-padded pair checked bit for bit against the unflagged launch on the
    truncated pair (assertion 2) -> K [A, B], gX [A, B, TX, d], gY [A, B, TY, d] of the pairs, unit weights, as numpy fp64"""
    TX, TY = max(map(len, xs)), max(map(len, ys))
    A, B = len(xs), len(ys)
    K, gX, gY = np.zeros((A, B)), np.zeros((A, B, TX, d)), np.zeros((A, B, TY, d))
    for i, x in enumerate(xs):
        for j, y in enumerate(ys):
            xn, yn = dev(R.pad_nan([x], TX), io, gpu), dev(R.pad_nan([y], TY), io, gpu)
            k1, gx1, gy1 = ops.gram_long_fwd_bwd2(xn, yn, 1.0 / H, n, kind, None, naive, nan_tails=True)
            if len(x) >= 2 and len(y) >= 2:
                k0, gx0, gy0 = ops.gram_long_fwd_bwd2(dev(x[None], io, gpu), dev(y[None], io, gpu), 1.0 / H, n, kind, None, naive)
                assert same_bits(k1, k0), (i, j)
                assert same_bits(gx1[:, :len(x)].contiguous(), gx0) and same_bits(gy1[:, :len(y)].contiguous(), gy0), (i, j)
            else:  # a one-point path: the constant kernel
                assert float(k1) == 1.0 and not gx1.any() and not gy1.any(), (i, j)
            assert zero_tails(gx1, [len(x)]) and zero_tails(gy1, [len(y)]), (i, j)
            K[i, j], gX[i, j], gY[i, j] = float(k1), np64(gx1)[0], np64(gy1)[0]
    return K, gX, gY


def oracle_pairs(xs, ys, n, kind, naive):
    """the C oracle on every truncated pair (assertion 4's reference), unit weights; a one-point path is its point twice"""
    two = lambda p: p if len(p) >= 2 else np.repeat(p, 2, axis=0)
    TX, TY, d = max(map(len, xs)), max(map(len, ys)), xs[0].shape[1]
    A, B = len(xs), len(ys)
    K, gX, gY = np.zeros((A, B)), np.zeros((A, B, TX, d)), np.zeros((A, B, TY, d))
    for i, x in enumerate(xs):
        for j, y in enumerate(ys):
            k, gx = oracle_at_own_lengths(two(x)[None], two(y)[None], H, n, naive, kind, None)
            _, gy = oracle_at_own_lengths(two(y)[None], two(x)[None], H, n, naive, kind, None)
            K[i, j] = k[0, 0]
            if len(x) >= 2 and len(y) >= 2:
                gX[i, j, :len(x)], gY[i, j, :len(y)] = gx[0], gy[0]
    return K, gX, gY


def check_two_sided(gpu, xs, ys, n, kind, naive, io, seed, forms):
    """assertions 1 - 7 for the two-sided launch of the NaN-padded batches, in each of `forms`: "both", "gx", "gy", "fwd",
    and for one batch in both slots (ys is xs) "yx" (signed weights) and "yx sym" """
    d, A, B = xs[0].shape[1], len(xs), len(ys)
    TX, TY = max(map(len, xs)), max(map(len, ys))
    LX, LY = [len(p) for p in xs], [len(p) for p in ys]
    Xn, Yn = dev(R.pad_nan(xs, TX), io, gpu), dev(R.pad_nan(ys, TY), io, gpu)
    Xl, Yl = dev(R.pad_last(xs, TX), io, gpu), dev(R.pad_last(ys, TY), io, gpu)
    assert R.lengths(np64(Xn)).tolist() == LX and R.lengths(np64(Yn)).tolist() == LY
    Kp, gXp, gYp = pair_references(gpu, xs, ys, d, n, kind, naive, io)
    Ko, gXo, gYo = oracle_pairs(xs, ys, n, kind, naive) if kind in (RBF, LINEAR) else (None, None, None)
    Wn = signed_weights(A, B, seed)
    tolK = 1e-9 if io == F64 else 2.0**-23
    for form in forms:
        yx, sym = form.startswith("yx"), form.endswith("sym")
        want_x, want_y = form in ("both", "gx") or yx, form in ("both", "gy")
        Wt = None if form == "fwd" else dev(Wn, io, gpu)
        kw = dict(sym=sym, y_is_x=yx, want_gradX=want_x, want_gradY=want_y)
        K, gX, gY = ops.gram_long_fwd_bwd2(Xn, Yn, 1.0 / H, n, kind, Wt, naive, nan_tails=True, **kw)  # (1: no BADARG)
        assert (gX is not None) == want_x and (gY is not None) == want_y, form
        # 3: the pairs.  (Y_IS_X solves the pairs i <= j and mirrors K: the 1 x 1 launch of (j, i) is the transposed solve,
        # whose increments round differently, so the lower triangle is held to the mirror's bits)
        if yx:
            assert np.array_equal(np.triu(np64(K)), np.triu(Kp)) and np.array_equal(np64(K), np64(K).T), form
        else:
            assert np.array_equal(np64(K), Kp), form
        Weff = Wn + Wn.T if sym else Wn
        # gX = sum_j W_ij d1 k(x_i, y_j) in every form (Y_IS_X: the first-slot gradient of every ordered pair), gY the second slot
        refs = {name: (Kq, np.einsum("ij,ijtc->itc", Weff, gXq), np.einsum("ij,ijtc->jtc", Weff, gYq))
                for name, Kq, gXq, gYq in (("pairs", Kp, gXp, gYp), ("oracle", Ko, gXo, gYo)) if Kq is not None}
        for name, (Kq, rx, ry) in refs.items():
            # (fp32 I/O, where the issue sets no figure: each of the at most 6 terms of a sum was rounded to fp32, 2^-24 of at
            # most 1.5 times the largest entry, and so was the launch's own sum: below 1e-6)
            tol = (1e-9 if io == F64 else 1e-6) if name == "pairs" else 1e-5
            if name == "oracle":  # 4
                eK = rel_entry(np64(K), Kq, 0.0)
                print(f"{form}: K vs oracle {eK:.2e}")
                assert eK < tolK, form
            for g, r, what in ((gX, rx, "gX"), (gY, ry, "gY")):
                if g is not None:
                    e = rel_max(np64(g), r)
                    print(f"{form}: {what} vs {name} {e:.2e}")
                    assert e < tol, (form, what, name)
        # 5: the unflagged launch on the last-point-padded batches
        Ku, gXu, gYu = ops.gram_long_fwd_bwd2(Xl, Yl, 1.0 / H, n, kind, Wt, naive, **kw)
        assert rel_entry(np64(K), np64(Ku), 0.0) < tolK, form
        if gX is not None:
            assert rel_max(np64(gX), R.fold(np64(gXu), LX)) < 1e-5, form
        if gY is not None:
            assert rel_max(np64(gY), R.fold(np64(gYu), LY)) < 1e-5, form
        # 6, 7
        assert gX is None or zero_tails(gX, LX), form
        assert gY is None or zero_tails(gY, LY), form
        K2, gX2, gY2 = ops.gram_long_fwd_bwd2(Xn, Yn, 1.0 / H, n, kind, Wt, naive, nan_tails=True, **kw)
        assert same_bits(K2, K) and same_bits(gX2, gX) and same_bits(gY2, gY), form


# (name, T, order, d, lengths of X, lengths of Y): lengths mixed so that short pairs follow long ones and the other way round.
#  edges   L_X - 1 in {1, 63, 64, 65, 128, 129} x L_Y - 1 in {1, 7, 8, 9}: the band hand-over, a last band of one row, the
#          8-deep ring of stored forward values
#  full    L = T = 131 at order 0 next to L = 4: the refill inside a band with W capped; one-point and two-point paths
#  order1 / order2   T = 33 and 18;  order7  T = 3 and L = 2 (nrow = 1)
LENGTH_CASES = {
    "edges": (131, 0, 3, [130, 2, 65, 129, 64, 66], [10, 2, 9, 8]),
    "full": (131, 0, 3, [131, 4, 1, 131, 2], [4, 131, 1, 2, 131]),
    "order1": (33, 1, 3, [33, 2, 17, 32, 5], [9, 33, 2, 3]),
    "order2": (18, 2, 3, [18, 2, 17, 3, 9], [2, 18, 16, 5]),
    "order7": (3, 7, 3, [3, 2, 2, 3, 2], [2, 3, 2]),
}


def case_paths(name, d=None, dtype=np.float32):
    T, n, d0, LX, LY = LENGTH_CASES[name]
    d = d or d0
    seed = sorted(LENGTH_CASES).index(name)
    return n, R.rough_paths(10 + seed, LX, d), R.rough_paths(50 + seed, LY, d)


@pytest.mark.parametrize("name", sorted(LENGTH_CASES))
def test_two_sided_lengths_fp64(gpu, name):
    n, xs, ys = case_paths(name)
    check_two_sided(gpu, xs, ys, n, RBF, False, F64, 1, ["both", "gx", "gy", "fwd"])


@pytest.mark.parametrize("name", ["edges", "order1"])
def test_two_sided_lengths_fp32_io(gpu, name):
    n, xs, ys = case_paths(name)
    check_two_sided(gpu, xs, ys, n, RBF, False, F32, 2, ["both", "fwd"])


@pytest.mark.parametrize("name", ["edges", "full", "order2"])
def test_one_batch_in_both_slots(gpu, name):
    """Y_IS_X with signed weights, and with SYM: each unordered pair solved once, both members' rows in gX"""
    n, xs, _ = case_paths(name)
    check_two_sided(gpu, xs, xs, n, RBF, False, F64, 3, ["yx", "yx sym", "fwd"])


@pytest.mark.parametrize("kind", [RBF, LINEAR])
def test_naive_stencil(gpu, kind):
    n, xs, ys = case_paths("order1")
    check_two_sided(gpu, xs, ys, n, kind, True, F64, 4, ["both"])


@pytest.mark.parametrize("kind", KINDS[1:])
def test_every_kind(gpu, kind):
    n, xs, ys = case_paths("order1")
    scale = 0.25 if kind == LINEAR else 1.0  # (the linear signature kernel of walks this rough overflows nothing but is huge)
    check_two_sided(gpu, [scale * p for p in xs], [scale * p for p in ys], n, kind, False, F64, 5, ["both"])


@pytest.mark.parametrize("d", [1, 7, 17])
def test_channels(gpu, d):
    n, xs, ys = case_paths("order1", d=d)
    s = np.float32(d**-0.5)
    check_two_sided(gpu, [s * p for p in xs], [s * p for p in ys], n, RBF, False, F64, 6, ["both"])


def test_a_batch_without_nan_equals_the_unflagged_launch(gpu):
    rng = np.random.default_rng(7)
    X = dev(np.cumsum(0.5 * rng.standard_normal((5, 131, 3)), axis=1).astype(np.float32), F64, gpu)
    Y = dev(np.cumsum(0.5 * rng.standard_normal((4, 70, 3)), axis=1).astype(np.float32), F64, gpu)
    W = dev(signed_weights(5, 4, 8), F64, gpu)
    for kw in (dict(), dict(want_gradY=False), dict(want_gradX=False, want_gradY=False)):
        a = ops.gram_long_fwd_bwd2(X, Y, 1.0, 0, RBF, W, **kw)
        b = ops.gram_long_fwd_bwd2(X, Y, 1.0, 0, RBF, W, nan_tails=True, **kw)
        assert all(same_bits(u, v) for u, v in zip(a, b)), kw
    Wx = dev(signed_weights(5, 5, 9), F64, gpu)
    for sym in (False, True):
        a = ops.gram_long_fwd_bwd2(X, X, 1.0, 0, RBF, Wx, sym=sym, y_is_x=True)
        b = ops.gram_long_fwd_bwd2(X, X, 1.0, 0, RBF, Wx, sym=sym, y_is_x=True, nan_tails=True)
        assert all(same_bits(u, v) for u, v in zip(a, b)), sym
    Yp = Y[:, :, :][torch.arange(5, device=gpu) % 4]
    a, b = ops.pair_fwd_bwd(X, Yp, 1.0, 0, RBF), ops.pair_fwd_bwd(X, Yp, 1.0, 0, RBF, nan_tails=True)
    assert all(same_bits(u, v) for u, v in zip(a, b))
    assert same_bits(ops.pair_fwd(X, Yp, 1.0, 0, RBF), ops.pair_fwd(X, Yp, 1.0, 0, RBF, nan_tails=True))


def test_many_pairs_per_wavefront(gpu):
    """more pairs than resident wavefronts, at T = 131 and at T = 16 (tiles of several rows and columns): every wavefront walks
    pairs of different lengths one after the other.  The whole launch against the unflagged launch on the last-point-padded
    batches and against the oracle on them (folded), and K bit for bit against 1 x 1 launches of sampled pairs."""
    cus = device_cus()
    for (A, B, T, short) in [(70, 40, 131, [130, 2, 65, 129, 64, 66, 131, 4, 1]), (150, 250, 16, list(range(1, 17)))]:
        pl = long2_plan(A, B, T, T, 2, 0, True, True, False, cus)
        assert pl["items"] > pl["grid"] or pl["IC"] * pl["JC"] > 1, pl
        rng = np.random.default_rng(A)
        LX, LY = rng.choice(short, A).tolist(), rng.choice(short, B).tolist()
        xs, ys = R.rough_paths(A, LX, 2), R.rough_paths(B, LY, 2)
        Xn, Yn = dev(R.pad_nan(xs, T), F64, gpu), dev(R.pad_nan(ys, T), F64, gpu)
        Xl, Yl = R.pad_last(xs, T), R.pad_last(ys, T)
        Wn = signed_weights(A, B, 11)
        W = dev(Wn, F64, gpu)
        K, gX, gY = ops.gram_long_fwd_bwd2(Xn, Yn, 1.0, 0, RBF, W, nan_tails=True)
        Ku, gXu, gYu = ops.gram_long_fwd_bwd2(dev(Xl, F64, gpu), dev(Yl, F64, gpu), 1.0, 0, RBF, W)
        assert rel_entry(np64(K), np64(Ku), 0.0) < 1e-9
        assert rel_max(np64(gX), R.fold(np64(gXu), LX)) < 1e-5 and rel_max(np64(gY), R.fold(np64(gYu), LY)) < 1e-5
        Ko, gXo = oracle_at_own_lengths(Xl, Yl, H, 0, False, RBF, Wn)
        _, gYo = oracle_at_own_lengths(Yl, Xl, H, 0, False, RBF, np.ascontiguousarray(Wn.T))
        assert rel_entry(np64(K), Ko, 0.0) < 1e-9
        assert rel_max(np64(gX), R.fold(gXo, LX)) < 1e-5 and rel_max(np64(gY), R.fold(gYo, LY)) < 1e-5
        assert zero_tails(gX, LX) and zero_tails(gY, LY)
        for i, j in zip(rng.integers(0, A, 12), rng.integers(0, B, 12)):
            k1 = ops.gram_long_fwd_bwd2(Xn[i:i + 1], Yn[j:j + 1], 1.0, 0, RBF, None, want_gradX=False, want_gradY=False,
                                        nan_tails=True)[0]
            assert same_bits(k1, K[i:i + 1, j:j + 1].contiguous()), (i, j)
        K2, gX2, gY2 = ops.gram_long_fwd_bwd2(Xn, Yn, 1.0, 0, RBF, W, nan_tails=True)
        assert same_bits(K2, K) and same_bits(gX2, gX) and same_bits(gY2, gY)


# ---- the paired launches ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,io,kind,naive", [("edges", F64, RBF, False), ("full", F64, RBF, False), ("order1", F32, RBF, False),
                                                ("order2", F64, LINEAR, True), ("order7", F64, RBF, False),
                                                ("order1", F64, _lib.STATIC_MATERN52, False)])
def test_paired_launches(gpu, name, io, kind, naive):
    """pair i is (X_i, Y_i): assertions 1 - 7 with the whole launch against 1 x 1 paired launches and the truncated pairs"""
    n, xs, ys = case_paths(name)
    if kind == LINEAR:
        xs, ys = [0.25 * p for p in xs], [0.25 * p for p in ys]
    A = len(xs)
    ys = [ys[i % len(ys)] for i in range(A)]
    d, TX, TY = xs[0].shape[1], max(map(len, xs)), max(map(len, ys))
    LX, LY = [len(p) for p in xs], [len(p) for p in ys]
    Xn, Yn = dev(R.pad_nan(xs, TX), io, gpu), dev(R.pad_nan(ys, TY), io, gpu)
    Wn = signed_weights(A, 1, 12)[:, 0]
    W = dev(Wn, io, gpu)
    assert ops.pair_schedule(A, TX, TY, d, n, kind, True, nan_tails=True)[0] == 1
    assert ops.pair_schedule(A, TX, TY, d, n, kind, False, nan_tails=True)[0] == 1
    K, gX, gY = ops.pair_fwd_bwd(Xn, Yn, 1.0 / H, n, kind, W, naive, nan_tails=True)
    assert same_bits(ops.pair_fwd(Xn, Yn, 1.0 / H, n, kind, naive, nan_tails=True), K)
    Kx, gx, none = ops.pair_fwd_bwd(Xn, Yn, 1.0 / H, n, kind, W, naive, want_y=False, nan_tails=True)
    Ky, none2, gy = ops.pair_fwd_bwd(Xn, Yn, 1.0 / H, n, kind, W, naive, want_x=False, nan_tails=True)
    assert none is None and none2 is None and same_bits(Kx, K) and same_bits(Ky, K) and same_bits(gx, gX) and same_bits(gy, gY)
    assert zero_tails(gX, LX) and zero_tails(gY, LY)
    Ku, gXu, gYu = ops.pair_fwd_bwd(dev(R.pad_last(xs, TX), io, gpu), dev(R.pad_last(ys, TY), io, gpu), 1.0 / H, n, kind, W, naive)
    assert rel_entry(np64(K), np64(Ku), 0.0) < (1e-9 if io == F64 else 2.0**-23)
    assert rel_max(np64(gX), R.fold(np64(gXu), LX)) < 1e-5 and rel_max(np64(gY), R.fold(np64(gYu), LY)) < 1e-5
    for i, (x, y) in enumerate(zip(xs, ys)):
        w = W[i:i + 1]
        k1, gx1, gy1 = ops.pair_fwd_bwd(Xn[i:i + 1], Yn[i:i + 1], 1.0 / H, n, kind, w, naive, nan_tails=True)
        assert same_bits(k1, K[i:i + 1]) and same_bits(gx1, gX[i:i + 1]) and same_bits(gy1, gY[i:i + 1]), i
        if len(x) >= 2 and len(y) >= 2:
            k0, gx0, gy0 = ops.pair_fwd_bwd(dev(x[None], io, gpu), dev(y[None], io, gpu), 1.0 / H, n, kind, w, naive)
            assert same_bits(k0, k1) and same_bits(gx0, gx1[:, :len(x)].contiguous()), i
            assert same_bits(gy0, gy1[:, :len(y)].contiguous()), i
            if kind in (RBF, LINEAR):
                ko, gxo = oracle_at_own_lengths(x[None], y[None], H, n, naive, kind, None)
                _, gyo = oracle_at_own_lengths(y[None], x[None], H, n, naive, kind, None)
                assert rel_entry(np64(k1), ko[0], 0.0) < (1e-9 if io == F64 else 2.0**-23), i
                assert rel_max(np64(gx0), Wn[i] * gxo) < 1e-5 and rel_max(np64(gy0), Wn[i] * gyo) < 1e-5, i
        else:
            assert float(k1) == 1.0 and not gx1.any() and not gy1.any(), i
    K2, gX2, gY2 = ops.pair_fwd_bwd(Xn, Yn, 1.0 / H, n, kind, W, naive, nan_tails=True)
    assert same_bits(K2, K) and same_bits(gX2, gX) and same_bits(gY2, gY)


# ---- the public surface --------------------------------------------------------------------------------------------------------
def surface(gpu, grad=True):
    T, n, d, LX, LY = LENGTH_CASES["order1"]
    LY = LY + [7]
    xs, ys = R.rough_paths(90, LX, d), R.rough_paths(91, LY, d)
    junk = lambda paths, T: dev(np.where(np.isnan(R.pad_nan(paths, T)), 3.0, R.pad_nan(paths, T)), F64, gpu).requires_grad_(grad)
    return xs, ys, LX, LY, junk(xs, T), junk(ys, T)  # (the entries past a path's end hold a number: lengths decide, not values)


# The truncated 1 x 1 calls of a SigKernel take the launch its routing gives a pair of that shape: the fused kernels here,
# whose contract is K within 1e-5 relative per entry and each gradient within 1e-5 of its largest entry;
# the long route's own is 1e-9 / 1e-5 against the same fp64 reference.  A weighted sum of pairs may differ from the flagged call
# by the sum of both bounds over its terms, and by no more: that sum is the bound below, entry by entry.
PAIR_TOL = 2e-5


class PairSums:
    """sum_ij w[i][j] k(x_i, y_j) from truncated 1 x 1 calls of `kernel`, the gradient per path, and for each the bound the
    contracts above allow; a one-point path is the constant kernel"""

    def __init__(self, kernel, xs, ys, gpu, w, T):
        d = xs[0].shape[1]
        self.value = self.value_tol = 0.0
        self.gx, self.gy = torch.zeros(len(xs), T, d, dtype=F64), torch.zeros(len(ys), T, d, dtype=F64)
        self.tx, self.ty = torch.zeros(len(xs)), torch.zeros(len(ys))
        for i, x in enumerate(xs):
            for j, y in enumerate(ys):
                if w[i][j] == 0.0:
                    continue
                if len(x) < 2 or len(y) < 2:
                    self.value += w[i][j]
                    continue
                xt, yt = dev(x[None], F64, gpu).requires_grad_(True), dev(y[None], F64, gpu).requires_grad_(True)
                k = kernel.compute_Gram(xt, yt, grad_Y=True)[0, 0]
                a, b = torch.autograd.grad(k, (xt, yt))
                self.value += w[i][j] * float(k.detach())
                self.value_tol += abs(w[i][j]) * PAIR_TOL * abs(float(k.detach()))
                self.gx[i, :len(x)] += w[i][j] * a[0].cpu()
                self.gy[j, :len(y)] += w[i][j] * b[0].cpu()
                self.tx[i] += abs(w[i][j]) * PAIR_TOL * float(a.abs().max())
                self.ty[j] += abs(w[i][j]) * PAIR_TOL * float(b.abs().max())


def within(grad, ref, tol):
    """|grad - ref| <= tol[path] in every entry"""
    return bool(((grad.detach().cpu().double() - ref).abs().amax(dim=(1, 2)) <= tol.double()).all())


def test_sigkernel_surface_with_lengths(gpu):
    import sigsvgd_amd.sigkernel as sk

    kernel = sk.SigKernel(sk.RBFKernel(H), 1)
    xs, ys, LX, LY, X, Y = surface(gpu)
    A, T = len(xs), X.shape[1]
    # compute_Gram, both slots
    W = signed_weights(A, A, 13)
    K = kernel.compute_Gram(X, Y, grad_Y=True, lengths_X=LX, lengths_Y=torch.tensor(LY, device=gpu))
    (K * dev(W, F64, gpu)).sum().backward()
    ref = PairSums(kernel, xs, ys, gpu, W, T)
    assert abs(float((K.detach() * dev(W, F64, gpu)).sum()) - ref.value) <= ref.value_tol
    assert within(X.grad, ref.gx, ref.tx) and within(Y.grad, ref.gy, ref.ty)
    assert zero_tails(X.grad, LX) and zero_tails(Y.grad, LY)
    # compute_kernel: the diagonal
    X.grad = Y.grad = None
    w = signed_weights(A, 1, 14)[:, 0]
    k = kernel.compute_kernel(X, Y, LX, LY)
    (k * dev(w, F64, gpu)).sum().backward()
    ref = PairSums(kernel, xs, ys, gpu, np.diag(w), T)
    assert abs(float((k.detach() * dev(w, F64, gpu)).sum()) - ref.value) <= ref.value_tol
    assert within(X.grad, ref.gx, ref.tx) and within(Y.grad, ref.gy, ref.ty)
    assert zero_tails(X.grad, LX) and zero_tails(Y.grad, LY)
    # compute_distance and compute_mmd(grad_Y=True): their three terms from the same truncated calls
    ones, eye = np.ones((A, A)) / (A * A), np.eye(A) / A
    for call, w in ((lambda: kernel.compute_distance(X, Y, LX, LY), eye),
                    (lambda: kernel.compute_mmd(X, Y, grad_Y=True, lengths_X=LX, lengths_Y=LY), ones)):
        X.grad = Y.grad = None
        v = call()
        v.backward()
        xx, yy, xy = PairSums(kernel, xs, xs, gpu, w, T), PairSums(kernel, ys, ys, gpu, w, T), PairSums(kernel, xs, ys, gpu, w, T)
        assert abs(float(v.detach()) - (xx.value + yy.value - 2.0 * xy.value)) <= xx.value_tol + yy.value_tol + 2.0 * xy.value_tol
        assert within(X.grad, xx.gx + xx.gy - 2.0 * xy.gx, xx.tx + xx.ty + 2.0 * xy.tx)
        assert within(Y.grad, yy.gx + yy.gy - 2.0 * xy.gy, yy.tx + yy.ty + 2.0 * xy.ty)
        assert zero_tails(X.grad, LX) and zero_tails(Y.grad, LY)


def test_flagged_launch_is_capturable(gpu, monkeypatch):
    """no read-back and no host sync between the length pass and the solve: the flagged launch is captured and replayed (on
    the cached workspace of `ops`, which the warm-up allocates before the capture)"""
    monkeypatch.setattr(ops, "_workspace", _CACHED_WORKSPACE)
    n, xs, ys = case_paths("order1")
    Xn, Yn = dev(R.pad_nan(xs, 33), F64, gpu), dev(R.pad_nan(ys, 33), F64, gpu)
    want = ops.gram_long_fwd_bwd2(Xn, Yn, 1.0, n, RBF, None, nan_tails=True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(gpu)
    with torch.cuda.stream(s):
        ops.gram_long_fwd_bwd2(Xn, Yn, 1.0, n, RBF, None, nan_tails=True)  # (warm-up on the capture stream)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        got = ops.gram_long_fwd_bwd2(Xn, Yn, 1.0, n, RBF, None, nan_tails=True)
    for t in got:
        t.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip(got, want))
