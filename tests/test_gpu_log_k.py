"""SIGSVGD_FLAG_LOG_K on the device: ln K and the gradients of ln K from the flagged launches of the
long route against the unflagged launches (where nothing overflows) and against the fp64 restatement of
tests/log_k_reference.py, and the normalised kernel of `SigKernel(..., normalize=True)` built on them.

Every case first asserts on the reference that all its K are > 0 (ln K finite), so no case hides behind a NaN.  The checks:

    ln K      |ln K_flagged - log(K_unflagged)| <= 1e-13 max(1, |ln K|) with fp64 I/O: one log and one fma, since the scaling
              is by powers of two and leaves the mantissa alone.  With fp32 I/O both stored numbers are rounded to 2^-24
              relative, which log carries into an absolute 2^-24: 3 * 2^-24 max(1, |ln K|).  Against the reference, whose
              sweep sums in another order and rescales by other factors, 1e-12 max(1, |ln K|) (fp32 I/O: 2 * 2^-24).  On the
              long rough cases an off-diagonal K of order 1 is what is left of terms that cancel, and neither fp64 sweep knows
              it to 1e-12: the reference is 1e-11 off a long-double run of the pair (x, y) at T = 400 and 4e-11 to 1e-10 off
              itself when it divides the anti-diagonals by other factors.  Rounding is relative to the values a step adds,
              so those cases multiply the bound by the pair's largest |K[p][q]| over its final K
              (log_k_reference.cancellation; 1 for a pair (x, x), whose K grows to its end).
    gradient  within BOUND = 1e-5 of the largest entry, the long route's bound (tests/test_gpu_exact_adjoint.py): of the
              unflagged launch weighted by w / K (grad ln K = grad K / K), and of the reference.

Where the unflagged K passes fp32 (from T = 200 at steps of 2.0) the unflagged launch's stored forward solution overflows, so
its gradient is no yardstick; the flagged gradient is then held to the reference alone.

Every flagged launch fails on a library without the feature, which answers SIGSVGD_E_BADARG for bit 1024."""
import functools

import numpy as np
import pytest
import torch

import log_k_reference as R
from parity import np64, rel_max, signed_weights
from sigsvgd_amd import _lib, ops

pytestmark = pytest.mark.gpu

BOUND = 1e-5
F64, F32 = torch.float64, torch.float32
RBF, LINEAR = _lib.STATIC_RBF, _lib.STATIC_LINEAR
KINDS = (_lib.STATIC_RBF, _lib.STATIC_LINEAR, _lib.STATIC_IMQ, _lib.STATIC_RQ, _lib.STATIC_MATERN32, _lib.STATIC_MATERN52)

# name -> (A, B, TX, TY, d, n): the exact adjoint's small shapes, a 129-row band edge, d = 1, 7, 17, several pairs per launch
SHAPES = {
    "P63_Q1_d1": (2, 3, 64, 2, 1, 0),
    "P64_Q7": (3, 2, 65, 8, 3, 0),
    "P65_Q8_d7": (2, 2, 66, 9, 7, 0),
    "P129_Q8": (2, 2, 130, 9, 3, 0),
    "d17": (2, 2, 20, 12, 17, 0),
    "T131": (2, 2, 131, 131, 2, 0),
    "order2_T18": (3, 3, 18, 18, 3, 2),
    "A5_B9": (5, 9, 20, 14, 3, 0),
}
SQUARE = ("T131", "order2_T18")
# (rough walks now and then have a pair whose discrete K is negative, two-channel ones of 131 steps often: these cases take
#  the next seeds whose pairs, (X, Y) and (X, X), are all positive)  (name, kind) -> added to the seed
SEED_BUMP = {("T131", RBF): 4, ("P65_Q8_d7", LINEAR): 2, ("order2_T18", _lib.STATIC_MATERN52): 1}


def rough(seed, B, T, d, kind=RBF, step=0.5):
    """[B, T, d] fp32-valued walks (fp32 and fp64 I/O see the same inputs); the linear kernel, whose increments are not
    bounded by 1, gets steps of 0.12 so that K stays positive"""
    step = 0.12 if kind == LINEAR else step
    return R.walks(seed, B, T, d, step, np.float32).astype(np.float64)


def inputs(name, kind=RBF):
    A, B, TX, TY, d, n = SHAPES[name]
    seed = sum(map(ord, name)) + 17 * kind + SEED_BUMP.get((name, kind), 0)
    return rough(seed, A, TX, d, kind), rough(seed + 1, B, TY, d, kind), n


def dev(a, io, gpu):
    return None if a is None else torch.as_tensor(a, dtype=io, device=gpu)


def ln_bound(ref, io, against_reference=False):
    scale = np.maximum(1.0, np.abs(ref))
    if io == F32:
        return (2 if against_reference else 3) * 2.0**-24 * scale
    return (1e-12 if against_reference else 1e-13) * scale


def check_ln(what, got, ref, io, against_reference=False, cancellation=1.0):
    """cancellation: log_k_reference.cancellation of the pairs, where the case has pairs whose K cancels (times the bound)"""
    got, ref = np64(got), np.asarray(ref, np.float64)
    assert np.isfinite(ref).all(), (what, "the yardstick is not finite")
    worst = float((np.abs(got - ref) / (ln_bound(ref, io, against_reference) * cancellation)).max())
    print(f"    {what}: {worst:.2e} of its bound")
    assert worst <= 1.0, (what, worst)


def check_grad(what, got, ref):
    assert np.isfinite(np64(got)).all(), what
    err = rel_max(np64(got), ref)
    print(f"    {what}: {err:.2e} of the largest entry")
    assert err < BOUND, (what, err)


@functools.lru_cache(maxsize=None)
def _two_sided_reference(name, kind, sym, yx):
    X, Y, n = inputs(name, kind)
    Y = X if yx or sym else Y  # (sym weights K and its transpose alike: one batch in both slots, in two buffers without yx)
    w = signed_weights(len(X), len(Y), n + len(X))
    wr = w + w.T if sym else w
    ln, gX, gY = R.log_gram_backward(X, Y, wr, kind, 1.0, n)  # (yx: gX is the first-slot gradient, as without it)
    assert np.isfinite(ln).all(), "a pair of this case has K <= 0"
    return X, Y, n, w, ln, gX, gY


def two_sided_case(gpu, name, io, kind=RBF, want=(True, True), sym=False, yx=False):
    """the flagged two-sided launch of a case against the unflagged one and the reference"""
    X, Y, n, w, ln_ref, gX_ref, gY_ref = _two_sided_reference(name, kind, sym, yx)
    Xt, wt = dev(X, io, gpu), dev(w, io, gpu)
    Yt = Xt if yx else dev(Y, io, gpu)
    kw = dict(sym=sym, y_is_x=yx, want_gradX=want[0], want_gradY=want[1])
    ln, gX, gY = ops.gram_long_fwd_bwd2(Xt, Yt, 1.0, n, kind, wt, log_k=True, **kw)
    K = ops.gram_long_fwd_bwd2(Xt, Yt, 1.0, n, kind, None, y_is_x=yx, want_gradX=False, want_gradY=False)[0]
    assert torch.isfinite(K).all() and (K > 0).all()
    check_ln("ln K against log(unflagged K)", ln, np.log(np64(K)), io)
    check_ln("ln K against the reference", ln, ln_ref, io, True)
    if yx:
        assert torch.equal(ln, ln.T)  # the mirror store
    forward = ops.gram_long_fwd_bwd2(Xt, Yt, 1.0, n, kind, None, y_is_x=yx, want_gradX=False, want_gradY=False, log_k=True)[0]
    assert torch.equal(forward, ln)  # the forward-only kernel: the same bits
    wk = wt / K  # grad ln K = grad K / K: the unflagged launch with these weights (sym: K is symmetric)
    _, pX, pY = ops.gram_long_fwd_bwd2(Xt, Yt, 1.0, n, kind, wk, **kw)
    for what, got, plain, ref in (("gX", gX, pX, gX_ref), ("gY", gY, pY, gY_ref)):
        if got is not None:
            check_grad(f"{what} against the unflagged launch over K", got, np64(plain))
            check_grad(f"{what} against the reference", got, ref)
    assert (gX is None) == (not want[0]) and (gY is None) == (not want[1] or sym or yx)


# ---- small shapes: agreement with the unflagged launch -------------------------------------------------------------------------
SMALL = [(name, F64) for name in SHAPES] + [("P65_Q8_d7", F32), ("T131", F32)]


@pytest.mark.parametrize("name,io", SMALL, ids=[f"{n}-{'f64' if io == F64 else 'f32'}" for n, io in SMALL])
def test_two_sided_small(gpu, name, io):
    two_sided_case(gpu, name, io)


@pytest.mark.parametrize("mode", ["row", "col", "yx", "yx_sym", "sym"])
@pytest.mark.parametrize("name", SQUARE)
def test_two_sided_modes(gpu, name, mode):
    want = {"row": (True, False), "col": (False, True)}.get(mode, (True, False))
    two_sided_case(gpu, name, F64, want=want, sym="sym" in mode, yx="yx" in mode)


@pytest.mark.parametrize("kind", KINDS)
def test_every_kind(gpu, kind):
    two_sided_case(gpu, "P65_Q8_d7", F64, kind)
    paired_case(gpu, "order2_T18", F64, kind)


def paired_case(gpu, name, io, kind=RBF):
    X, Y, n = inputs(name, kind)
    A = min(len(X), len(Y))
    X, Y = X[:A], Y[:A]
    w = signed_weights(1, A, 3)[0]
    ln_ref, gX_ref, gY_ref = R.log_pair_backward(X, Y, w, kind, 1.0, n)
    assert np.isfinite(ln_ref).all(), "a pair of this case has K <= 0"
    Xt, Yt, wt = dev(X, io, gpu), dev(Y, io, gpu), dev(w, io, gpu)
    ln, gX, gY = ops.pair_fwd_bwd(Xt, Yt, 1.0, n, kind, wt, log_k=True)
    K = ops.pair_fwd(Xt, Yt, 1.0, n, kind)
    check_ln("paired ln K against log(unflagged K)", ln, np.log(np64(K)), io)
    check_ln("paired ln K against the reference", ln, ln_ref, io, True)
    assert torch.equal(ops.pair_fwd(Xt, Yt, 1.0, n, kind, log_k=True), ln)
    two = ops.gram_long_fwd_bwd2(Xt, Yt, 1.0, n, kind, None, want_gradX=False, want_gradY=False, log_k=True)[0]
    assert torch.equal(two.diagonal(), ln)  # the two-sided launch gives ln K the same bits
    _, pX, pY = ops.pair_fwd_bwd(Xt, Yt, 1.0, n, kind, wt / K)
    for what, got, plain, ref in (("gX", gX, pX, gX_ref), ("gY", gY, pY, gY_ref)):
        check_grad(f"paired {what} against the unflagged launch over K", got, np64(plain))
        check_grad(f"paired {what} against the reference", got, ref)
    only_y = ops.pair_fwd_bwd(Xt, Yt, 1.0, n, kind, wt, want_x=False, log_k=True)
    assert only_y[1] is None and torch.equal(only_y[2], gY)


PAIRED = [("P64_Q7", F64), ("P65_Q8_d7", F64), ("P65_Q8_d7", F32), ("P129_Q8", F64), ("T131", F64), ("T131", F32), ("order2_T18", F64)]


@pytest.mark.parametrize("name,io", PAIRED, ids=[f"{n}-{'f64' if io == F64 else 'f32'}" for n, io in PAIRED])
def test_paired_small(gpu, name, io):
    paired_case(gpu, name, io)


def test_tiles_of_several_pairs(gpu):
    """items of several pairs both ways with ragged last tiles and more items than resident waves (the shape of
    tests/test_gpu_long2.py): the per-pair exponents and 1 / K must not leak from one pair of a wavefront into the next"""
    from plans import device_cus, long2_plan

    A, B, T, d = 131, 151, 12, 2
    pl = long2_plan(A, B, T, T, d, 0, True, True, False, device_cus())
    assert pl["IC"] > 1 and pl["JC"] > 1 and pl["items"] > pl["grid"], pl
    X, Y = rough(5, A, T, d, step=0.1), rough(6, B, T, d, step=0.1)  # (among 19781 rough pairs some K would be negative)
    w = signed_weights(A, B, 7)
    ln_ref, gX_ref, gY_ref = R.log_gram_backward(X, Y, w)
    assert np.isfinite(ln_ref).all()
    Xt, Yt = dev(X, F64, gpu), dev(Y, F64, gpu)
    ln, gX, gY = ops.gram_long_fwd_bwd2(Xt, Yt, 1.0, 0, RBF, dev(w, F64, gpu), log_k=True)
    check_ln("ln K against the reference", ln, ln_ref, F64, True)
    check_grad("gX against the reference", gX, gX_ref)
    check_grad("gY against the reference", gY, gY_ref)


# ---- forced rescaling: steps of 2.0, the running exponent changes in most blocks and across the bands ------------------------------
# name -> (T, n): 131 and 200 points, P = 129 = 2 * 64 + 1 rows, and dyadic order 1 (P = 200).  A = 2 paths x with Y = x: the
# pairs (x, x) on the diagonal and (x, y) off it.  ln K(x, x) is 58 to 91 here: finite unflagged in fp64, past fp32 at T = 200.
FORCED = {"T131": (131, 0), "T200": (200, 0), "P129": (130, 0), "order1_T101": (101, 1)}


@functools.lru_cache(maxsize=None)
def _forced_reference(name, step=2.0, d=3, A=2):
    T, n = FORCED.get(name) or PAST[name]
    X = rough(sum(map(ord, name)), A, T, d, step=step)
    w = signed_weights(A, A, T)
    ln, gX, gY = R.log_gram_backward(X, X, w, RBF, 1.0, n)
    lp, pX, pY = R.log_pair_backward(X, X, w[0], RBF, 1.0, n)
    assert np.isfinite(ln).all(), "a pair of this case has K <= 0"
    return X, n, w, ln, gX, gX + gY, lp, pX, pY, R.cancellation(X, X, RBF, 1.0, n)


def forced_case(gpu, name, io, step=2.0, plain_gradient=True):
    X, n, w, ln_ref, gX_ref, g_ref, lp_ref, pX_ref, pY_ref, cancel = _forced_reference(name, step)
    Xt, wt = dev(X, io, gpu), dev(w, io, gpu)
    ln, gX, _ = ops.gram_long_fwd_bwd2(Xt, Xt, 1.0, n, RBF, wt, y_is_x=True, log_k=True)
    check_ln("ln K against the reference", ln, ln_ref, io, True, cancel)
    check_grad("gX (first slot, each unordered pair once) against the reference", gX, gX_ref)
    lp, pX, pY = ops.pair_fwd_bwd(Xt, Xt, 1.0, n, RBF, wt[0], log_k=True)
    assert torch.equal(lp, ln.diagonal())
    check_grad("paired gX against the reference", pX, pX_ref)
    check_grad("paired gY against the reference", pY, pY_ref)
    # two batches: the ordered pairs, both gradients
    lo, oX, oY = ops.gram_long_fwd_bwd2(Xt, Xt.clone(), 1.0, n, RBF, wt, log_k=True)
    assert torch.equal(lo.triu(), ln.triu())  # (below the diagonal the ordered launch solves (x_j, x_i), not the mirror image)
    check_grad("ordered gX + gY against the reference", oX + oY, g_ref)
    if io == F64 and ln_ref.max() < 700:  # still finite unflagged in fp64
        K = ops.gram_long_fwd_bwd2(Xt, Xt, 1.0, n, RBF, None, y_is_x=True, want_gradX=False, want_gradY=False)[0]
        check_ln("ln K against log(unflagged K)", ln, np.log(np64(K)), io)
        if plain_gradient:
            _, plain, _ = ops.gram_long_fwd_bwd2(Xt, Xt, 1.0, n, RBF, wt / K, y_is_x=True)
            check_grad("gX against the unflagged launch over K", gX, np64(plain))
    return ln_ref


@pytest.mark.parametrize("name", list(FORCED))
def test_forced_rescaling(gpu, name):
    ln_ref = forced_case(gpu, name, F64, plain_gradient=name != "T200")
    assert ln_ref.max() > 40  # the running exponent has passed the drift threshold many times
    assert (ln_ref.max() > 88.7) == (name == "T200")  # (only there is the unflagged stored solution past fp32)


# ---- past fp32 and past fp64 -------------------------------------------------------------------------------------------------------
PAST = {"T400": (400, 0)}


@pytest.mark.parametrize("io", [F64, F32], ids=["f64", "f32"])
def test_past_fp32(gpu, io):
    """T = 400 at steps of 0.5: K(x, x) is about 1e44, past fp32.  The unflagged gradient of the same launch is printed, not
    asserted (DESIGN.md section 5.21 records what it returned)."""
    ln_ref = forced_case(gpu, "T400", io, step=0.5, plain_gradient=False)
    assert ln_ref.max() > 88.8
    X = _forced_reference("T400", 0.5)[0]
    Xt = dev(X, F64, gpu)
    K, g, _ = ops.gram_long_fwd_bwd2(Xt, Xt, 1.0, 0, RBF, None, y_is_x=True)
    print(f"    unflagged fp64 launch: K finite {bool(torch.isfinite(K).all())}, "
          f"gradient entries not finite {int((~torch.isfinite(g)).sum())} of {g.numel()}")


def test_past_fp64(gpu):
    """one pair (x, x) of 1700 points at steps of 2.0: ln K is past ln(DBL_MAX) = 709.78"""
    X = rough(3, 1, 1700, 3, step=2.0)
    ln_ref, gX_ref, gY_ref = R.log_pair_backward(X, X)
    assert ln_ref[0] > 709.79
    Xt = dev(X, F64, gpu)
    ln, gX, gY = ops.pair_fwd_bwd(Xt, Xt, 1.0, 0, RBF, None, log_k=True)
    check_ln("ln K against the reference", ln, ln_ref, F64, True)
    check_grad("gX against the reference", gX, gX_ref)
    check_grad("gY against the reference", gY, gY_ref)
    assert not torch.isfinite(ops.pair_fwd(Xt, Xt, 1.0, 0, RBF)).any()  # (the unflagged launch overflows, as it must)


# ---- graph capture ---------------------------------------------------------------------------------------------------------------
def test_flagged_launch_is_capturable(gpu):
    """no read-back and no host sync: the flagged launch is captured and replayed (on the cached workspace of `ops`, which the
    warm-up allocates before the capture)"""
    X, Y, n = inputs("order2_T18")
    Xt, Yt = dev(X, F64, gpu), dev(Y, F64, gpu)
    want = ops.gram_long_fwd_bwd2(Xt, Yt, 1.0, n, RBF, None, log_k=True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(gpu)
    with torch.cuda.stream(s):
        ops.gram_long_fwd_bwd2(Xt, Yt, 1.0, n, RBF, None, log_k=True)  # (warm-up on the capture stream)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        got = ops.gram_long_fwd_bwd2(Xt, Yt, 1.0, n, RBF, None, log_k=True)
    for t in got:
        t.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# ---- the surface: SigKernel(..., normalize=True) -----------------------------------------------------------------------------------
_normalized_torch = R.normalized_torch


SIGMA = 1.0


def _surface_inputs(gpu, A, B, T, d, step):
    X, Y = rough(11, A, T, d, step=step), rough(12, B, T, d, step=step)
    return X, Y, dev(X, F64, gpu), dev(Y, F64, gpu)


def test_normalized_diagonal_is_exactly_one(gpu):
    import sigsvgd_amd.sigkernel as sk

    kernel = sk.SigKernel(sk.RBFKernel(SIGMA), 0, normalize=True)
    for (A, T, step) in [(4, 300, 0.5), (6, 16, 0.5)]:
        Xt = dev(rough(11, A, T, 3, step=step), F64, gpu)
        Kh = kernel.compute_Gram(Xt, Xt, sym=True)
        assert torch.equal(Kh.diagonal(), torch.ones(A, dtype=F64, device=gpu))
        assert torch.equal(Kh, Kh.T) and (Kh > 0).all()


def test_normalized_small_against_torch(gpu):
    """(6, 5, 16, 3): values and gradients of compute_Gram, compute_kernel and compute_mmd(grad_Y=True) against the torch
    construction K / sqrt(K_xx K_yy) of the oracle's sweep (tests/test_log_k_cpu.py holds the composition to it as well)"""
    import sigsvgd_amd.sigkernel as sk

    A, B, T, d = 6, 5, 16, 3
    X, Y, Xt, Yt = _surface_inputs(gpu, A, B, T, d, 0.5)
    kernel = sk.SigKernel(sk.RBFKernel(SIGMA), 0, normalize=True)
    Xc, Yc = torch.tensor(X, requires_grad=True), torch.tensor(Y, requires_grad=True)
    W = torch.tensor(signed_weights(A, B, 1))
    # compute_Gram with grad_Y
    ref = _normalized_torch(Xc, Yc, SIGMA)
    rgX, rgY = torch.autograd.grad((W * ref).sum(), (Xc, Yc))
    Xg, Yg = Xt.clone().requires_grad_(True), Yt.clone().requires_grad_(True)
    Kh = kernel.compute_Gram(Xg, Yg, grad_Y=True)
    gX, gY = torch.autograd.grad((W.to(gpu) * Kh).sum(), (Xg, Yg))
    assert rel_max(Kh, ref.detach().numpy()) < 1e-12
    check_grad("normalised Gram gX", gX, rgX.numpy())
    check_grad("normalised Gram gY", gY, rgY.numpy())
    # compute_kernel
    refk = _normalized_torch(Xc[:B], Yc, SIGMA).diagonal()
    w = torch.tensor(signed_weights(1, B, 2)[0])
    rkX, rkY = torch.autograd.grad((w * refk).sum(), (Xc, Yc))
    Xg, Yg = Xt[:B].clone().requires_grad_(True), Yt.clone().requires_grad_(True)
    kh = kernel.compute_kernel(Xg, Yg)
    kX, kY = torch.autograd.grad((w.to(gpu) * kh).sum(), (Xg, Yg))
    assert rel_max(kh, refk.detach().numpy()) < 1e-12
    check_grad("normalised kernel gX", kX, rkX.numpy()[:B])
    check_grad("normalised kernel gY", kY, rkY.numpy())
    # compute_mmd(grad_Y=True)
    nt = lambda P, Q: _normalized_torch(P, Q, SIGMA)
    refm = nt(Xc, Xc).mean() + nt(Yc, Yc).mean() - 2 * nt(Xc, Yc).mean()
    rmX, rmY = torch.autograd.grad(refm, (Xc, Yc))
    Xg, Yg = Xt.clone().requires_grad_(True), Yt.clone().requires_grad_(True)
    m = kernel.compute_mmd(Xg, Yg, grad_Y=True)
    mX, mY = torch.autograd.grad(m, (Xg, Yg))
    assert abs(float(m.detach()) - float(refm.detach())) < 1e-12 * max(1.0, abs(float(refm.detach())))
    check_grad("normalised mmd gX", mX, rmX.numpy())
    check_grad("normalised mmd gY", mY, rmY.numpy())


def check_khat(what, got, ref, X, Y, paired=False):
    """Khat = exp(l - a / 2 - b / 2) entry by entry: each logarithm within the ln K bound of this file against the reference
    (1e-12 max(1, |ln K|), times the pair's cancellation for l), so Khat within their sum, relatively"""
    unit = lambda v: 1e-12 * np.maximum(1.0, np.abs(v))
    l, c = R.log_gram(X, Y), R.cancellation(X, Y)
    a, b = R.log_gram(X, X).diagonal(), R.log_gram(Y, Y).diagonal()
    tol = unit(l) * c + 0.5 * unit(a)[:, None] + 0.5 * unit(b)[None, :]
    if paired:
        tol = tol.diagonal()
    worst = float((np.abs(np64(got) - ref) / (np.abs(ref) * tol)).max())
    print(f"    {what}: {worst:.2e} of its bound (largest cancellation {c.max():.1f})")
    assert worst <= 1.0, (what, worst)


def test_normalized_long_against_reference(gpu):
    """(4, 5, 300, 3): K(x, x) is about 1e34 here, so the yardstick is the composition of test (d) of tests/test_log_k_cpu.py
    on the log-domain reference (which that test holds to the torch construction where K fits fp64)"""
    import sigsvgd_amd.sigkernel as sk

    A, B, T, d = 4, 5, 300, 3
    X, Y, Xt, Yt = _surface_inputs(gpu, A, B, T, d, 0.5)
    W = signed_weights(A, B, 1)
    ref, rgX, rgY = R.normalized_gram_and_grads(X, Y, W)
    kernel = sk.SigKernel(sk.RBFKernel(SIGMA), 0, normalize=True)
    Xg, Yg = Xt.clone().requires_grad_(True), Yt.clone().requires_grad_(True)
    Kh = kernel.compute_Gram(Xg, Yg, grad_Y=True)
    gX, gY = torch.autograd.grad((dev(W, F64, gpu) * Kh).sum(), (Xg, Yg))
    check_khat("normalised Gram", Kh, ref, X, Y)
    check_grad("normalised Gram gX", gX, rgX)
    check_grad("normalised Gram gY", gY, rgY)
    # compute_kernel and compute_mmd on the same batch
    refk = np.diagonal(R.normalized_gram_and_grads(X, Y[:A], np.eye(A))[0])
    kh = kernel.compute_kernel(Xt, Yt[:A])
    check_khat("normalised kernel", kh, refk, X, Y[:A], True)
    refs, sgX, _ = R.normalized_gram_and_grads(X, X, np.full((A, A), 1.0 / (A * A)), same=True)
    refc, cgX, cgY = R.normalized_gram_and_grads(X, Y, np.full((A, B), -2.0 / (A * B)))
    refy, ygY, _ = R.normalized_gram_and_grads(Y, Y, np.full((B, B), 1.0 / (B * B)), same=True)
    Xg, Yg = Xt.clone().requires_grad_(True), Yt.clone().requires_grad_(True)
    m = kernel.compute_mmd(Xg, Yg, grad_Y=True)
    mX, mY = torch.autograd.grad(m, (Xg, Yg))
    want = refs.mean() + refy.mean() - 2 * refc.mean()
    assert abs(float(m.detach()) - want) < 1e-9 * max(1.0, abs(want))  # (means of Khat entries, each within check_khat's bound: < 1e-10)
    check_grad("normalised mmd gX", mX, sgX + cgX)
    check_grad("normalised mmd gY", mY, ygY + cgY)


def test_log_gram_and_log_kernel_are_differentiable(gpu):
    import sigsvgd_amd.sigkernel as sk

    X, Y, n = inputs("P65_Q8_d7")
    w = signed_weights(len(X), len(Y), 3)
    ln_ref, gX_ref, gY_ref = R.log_gram_backward(X, Y, w)
    kernel = sk.SigKernel(sk.RBFKernel(SIGMA), 0)
    Xg, Yg = dev(X, F64, gpu).requires_grad_(True), dev(Y, F64, gpu).requires_grad_(True)
    L = kernel.compute_log_Gram(Xg, Yg, grad_Y=True)
    gX, gY = torch.autograd.grad((dev(w, F64, gpu) * L).sum(), (Xg, Yg))
    check_ln("compute_log_Gram", L, ln_ref, F64, True)
    check_grad("compute_log_Gram gX", gX, gX_ref)
    check_grad("compute_log_Gram gY", gY, gY_ref)
    lp = kernel.compute_log_kernel(Xg, Yg)
    assert torch.equal(lp, L.diagonal())
    pX, pY = torch.autograd.grad((dev(w[0], F64, gpu) * lp).sum(), (Xg, Yg))
    rp = R.log_pair_backward(X, Y, w[0])
    check_grad("compute_log_kernel gX", pX, rp[1])
    check_grad("compute_log_kernel gY", pY, rp[2])


def test_default_sigkernel_keeps_its_bits(gpu):
    """normalize=False, the default, changes no call: the same bits as the launches it always made"""
    import sigsvgd_amd.sigkernel as sk

    X, Y, n = inputs("T131")
    Xt, Yt = dev(X, F64, gpu), dev(Y, F64, gpu)
    for kernel in (sk.SigKernel(sk.RBFKernel(SIGMA), 0), sk.SigKernel(sk.RBFKernel(SIGMA), 0, normalize=False)):
        Xg = Xt.clone().requires_grad_(True)
        K = kernel.compute_Gram(Xg, Yt)
        (g,) = torch.autograd.grad(K.sum(), Xg)
        K0, g0 = ops.gram_long_fwd_bwd(Xt, Yt, 1.0 / SIGMA, 0, RBF, None) if not ops.gram_takes(2, 2, 131, 2) else \
            ops.gram_fwd_bwd(Xt, Yt, 1.0 / SIGMA, 0, RBF, None)
        assert torch.equal(K, K0) and torch.equal(g, g0)
