"""The band-parallel schedule of the paired solver (csrc/pair_bands.hip): under
SIGSVGD_PAIR_MODE=bands K and both gradients are bit-identical to SIGSVGD_PAIR_MODE=serial (the one-wavefront kernel of
csrc/gram_long.hip) and within the project's tolerances of the oracle, at the smallest shapes at which each mechanism of the
schedule can fail; `ops.pair_schedule` shows that the cooperative kernel ran."""
import numpy as np
import pytest
import torch

import radial_reference as RR
from oracle import c_oracle
from parity import np64, rel_entry, rel_max, sized_walks

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
RBF, LINEAR, IMQ, RQ = 0, 1, 2, 3
H = 0.5


def c_pair_first_slot(X, Y, h, n, naive, kind, w):
    """C oracle per pair: (K [A], d(w_i k(X_i, Y_i))/dX_i [A, TX, d]), the shorter path of a pair padded with its last point
    (exact) and the gradient of a padded X folded back onto its points."""
    from sigsvgd_amd import ops

    A, TX = X.shape[:2]
    T = max(TX, Y.shape[1])
    pad = lambda P: ops.pad_to_length(torch.as_tensor(P), T).numpy()
    Xp, Yp = pad(X), pad(Y)
    K, g = np.empty(A), np.empty((A, T, X.shape[2]))
    nthreads = 2 if (T - 1) << n > 4096 else 0
    for i in range(A):
        Ki, gi = c_oracle.gram_fwd_bwd(Xp[i:i + 1], Yp[i:i + 1], h=h, n=n, naive=naive, kind=kind, grad_out=w[i:i + 1, None],
                                       nthreads=nthreads)
        K[i], g[i] = Ki[0, 0], gi[0]
    return K, ops.fold_padded_grad(torch.as_tensor(g), TX).numpy()


def reference(X, Y, n, naive, kind, w):
    """(K, gX, gY) of the oracle: the C oracle for RBF and linear (the second slot is the first slot of the swapped pair), the
    radial reference for IMQ and rational quadratic, which the C oracle does not have"""
    if kind in (IMQ, RQ):
        return RR.pair_backward(X, Y, w, kind, H, n)
    Kr, gXr = c_pair_first_slot(X, Y, H, n, naive, kind, w)
    _, gYr = c_pair_first_slot(Y, X, H, n, naive, kind, w)
    return Kr, gXr, gYr


def run_pairs(monkeypatch, mode, Xt, Yt, n, kind, wt, naive):
    """every launch form under one schedule: (K forward only, (K, gX, gY), (K, gX) alone, (K, gY) alone)"""
    from sigsvgd_amd import ops

    monkeypatch.setenv("SIGSVGD_PAIR_MODE", mode)
    K0 = ops.pair_fwd(Xt, Yt, 1.0 / H, n, kind, naive)
    K, gX, gY = ops.pair_fwd_bwd(Xt, Yt, 1.0 / H, n, kind, wt, naive)
    Kx, gx, none_y = ops.pair_fwd_bwd(Xt, Yt, 1.0 / H, n, kind, wt, naive, want_y=False)
    Ky, none_x, gy = ops.pair_fwd_bwd(Xt, Yt, 1.0 / H, n, kind, wt, naive, want_x=False)
    assert none_x is None and none_y is None
    return K0, K, gX, gY, Kx, gx, Ky, gy


def assert_bands_ran(monkeypatch, A, TX, TY, d, n, kind):
    from sigsvgd_amd import ops

    monkeypatch.setenv("SIGSVGD_PAIR_MODE", "bands")
    for want_grad in (False, True):
        waves = ops.pair_schedule(A, TX, TY, d, n, kind, want_grad)[0]
        assert waves > 1, f"the launch stays on the serial kernel ({waves} wave per pair)"
    monkeypatch.setenv("SIGSVGD_PAIR_MODE", "serial")
    assert ops.pair_schedule(A, TX, TY, d, n, kind)[0] == 1


# (A, TX, TY, d, n, kind, naive, io)
CASES = [
    (3, 130, 130, 2, 0, RBF, False, F64),     # three bands, the last of one row (P = 129)
    (2, 322, 322, 3, 0, RBF, False, F64),     # six bands, the last of one row
    (2, 322, 322, 3, 0, RBF, False, F32),
    (2, 260, 260, 3, 2, RBF, False, F64),     # 17 bands at order 2: a wave's further bands, the seam, idle waves in the tail
    (2, 700, 700, 2, 0, RBF, False, F64),     # 11 bands on 8 waves at order 0: the seam row and its column differences, a
    (2, 700, 700, 2, 0, RBF, False, F32),     # second round of three bands with five waves idle; the last band has 59 rows
    (2, 400, 6, 2, 0, RBF, False, F64),       # a sweep shorter than one phase and than the pipeline's fill: Q = 5
    (2, 70, 600, 2, 0, RBF, False, F64),      # two bands, many phases, TX != TY
    (2, 9, 9, 2, 8, RBF, False, F64),         # nrow = 1
    (3, 150, 140, 3, 1, LINEAR, True, F64),   # linear static kernel, naive stencil
    (2, 200, 200, 3, 0, IMQ, False, F64),
    (2, 200, 200, 3, 1, RQ, False, F64),
    (2, 300, 300, 17, 0, RBF, False, F64),    # channels past the 16 held in registers, a larger per-wave LDS share
    (2, 1024, 1024, 2, 0, RBF, False, F64),   # the one long case: 16 bands on 8 waves at order 0, the seam's full row
]


def _case_id(c):
    A, TX, TY, d, n, kind, naive, io = c
    return (f"A{A}-T{TX}x{TY}-d{d}-n{n}-{('rbf', 'lin', 'imq', 'rq')[kind]}{'-naive' if naive else ''}-"
            f"{'f32' if io == F32 else 'f64'}")


@pytest.mark.parametrize("A,TX,TY,d,n,kind,naive,io", CASES, ids=[_case_id(c) for c in CASES])
def test_bands_match_serial_bit_for_bit_and_the_oracle(gpu, monkeypatch, A, TX, TY, d, n, kind, naive, io):
    rng = np.random.default_rng(A * 1000 + TX * 7 + TY + 31 * d + n + 5 * kind + naive)
    X, Y = sized_walks(rng, A, TX, d, d**-0.5), sized_walks(rng, A, TY, d, d**-0.5)
    w = rng.uniform(-1.5, 1.5, A)
    Xt, Yt = torch.as_tensor(X, dtype=io, device=gpu), torch.as_tensor(Y, dtype=io, device=gpu)
    wt = torch.as_tensor(w, device=gpu)
    assert_bands_ran(monkeypatch, A, TX, TY, d, n, kind)
    serial = run_pairs(monkeypatch, "serial", Xt, Yt, n, kind, wt, naive)
    bands = run_pairs(monkeypatch, "bands", Xt, Yt, n, kind, wt, naive)
    names = ("K fwd", "K", "gX", "gY", "K (x alone)", "gX alone", "K (y alone)", "gY alone")
    for name, s, b in zip(names, serial, bands):
        assert b.dtype == io and b.shape == s.shape
        diff = (np64(b) - np64(s))
        assert torch.equal(b, s), f"{name}: {np.count_nonzero(diff)} of {diff.size} entries differ, max {np.abs(diff).max()}"
    K0, K, gX, gY = bands[:4]
    assert torch.equal(K0, K) and torch.equal(bands[4], K) and torch.equal(bands[6], K)
    assert torch.equal(bands[5], gX) and torch.equal(bands[7], gY)
    Kr, gXr, gYr = reference(X, Y, n, naive, kind, w)
    print("pair bands", _case_id((A, TX, TY, d, n, kind, naive, io)), rel_entry(np64(K), Kr, 0.0), rel_max(np64(gX), gXr),
          rel_max(np64(gY), gYr))
    assert rel_entry(np64(K), Kr, 0.0) < (1e-9 if io == F64 else 2.0**-23)
    assert rel_max(np64(gX), gXr) < 1e-5
    assert rel_max(np64(gY), gYr) < 1e-5


def test_more_pairs_than_resident_workgroups(gpu, monkeypatch):
    """The per-workgroup item loop: LDS windows and scratch slots reused from pair to pair."""
    from sigsvgd_amd import ops

    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    A, T, d, n = 8 * cus + 3, 66, 2, 0
    rng = np.random.default_rng(77)
    X, Y = sized_walks(rng, A, T, d, d**-0.5), sized_walks(rng, A, T, d, d**-0.5)
    w = rng.uniform(-1.5, 1.5, A)
    Xt, Yt, wt = (torch.as_tensor(v, dtype=F64, device=gpu) for v in (X, Y, w))
    assert_bands_ran(monkeypatch, A, T, T, d, n, RBF)
    monkeypatch.setenv("SIGSVGD_PAIR_MODE", "bands")
    assert ops.pair_schedule(A, T, T, d, n)[1] < A  # every workgroup takes several pairs
    serial = run_pairs(monkeypatch, "serial", Xt, Yt, n, RBF, wt, False)
    bands = run_pairs(monkeypatch, "bands", Xt, Yt, n, RBF, wt, False)
    for s, b in zip(serial, bands):
        assert torch.equal(b, s)
    pick = np.sort(np.random.default_rng(5).choice(A, 8, replace=False))
    Kr, gXr, gYr = reference(X[pick], Y[pick], n, False, RBF, w[pick])
    K, gX, gY = bands[1:4]
    assert rel_entry(np64(K)[pick], Kr, 0.0) < 1e-9
    assert rel_max(np64(gX)[pick], gXr) < 1e-5 and rel_max(np64(gY)[pick], gYr) < 1e-5


def test_bands_reproducible(gpu, monkeypatch):
    from sigsvgd_amd import ops

    rng = np.random.default_rng(9)
    X = torch.as_tensor(sized_walks(rng, 5, 322, 3, 3**-0.5), dtype=F64, device=gpu)
    Y = torch.as_tensor(sized_walks(rng, 5, 300, 3, 3**-0.5), dtype=F64, device=gpu)
    assert_bands_ran(monkeypatch, 5, 322, 300, 3, 0, RBF)
    monkeypatch.setenv("SIGSVGD_PAIR_MODE", "bands")
    a = ops.pair_fwd_bwd(X, Y, 1.0 / H, 0)
    b = ops.pair_fwd_bwd(X, Y, 1.0 / H, 0)
    for s, t in zip(a, b):
        assert torch.equal(s, t)


@pytest.mark.parametrize("surface", ["compute_kernel", "compute_distance"])
def test_autograd_surface_is_schedule_independent(gpu, monkeypatch, surface):
    import sigsvgd_amd.sigkernel as sk

    A, T, d = 3, 200, 3
    rng = np.random.default_rng(4)
    X = torch.as_tensor(sized_walks(rng, A, T, d, d**-0.5), dtype=F64, device=gpu)
    Y = torch.as_tensor(sized_walks(rng, A, T, d, d**-0.5), dtype=F64, device=gpu)
    w = torch.as_tensor(rng.uniform(-1.5, 1.5, A), device=gpu)
    assert_bands_ran(monkeypatch, A, T, T, d, 0, RBF)
    out = {}
    for mode in ("serial", "bands"):
        monkeypatch.setenv("SIGSVGD_PAIR_MODE", mode)
        Xg, Yg = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
        k = sk.SigKernel(sk.RBFKernel(0.8), 0)
        if surface == "compute_kernel":
            v = k.compute_kernel(Xg, Yg)
            (v * w).sum().backward()
        else:
            v = k.compute_distance(Xg, Yg)
            (v * w).sum().backward() if v.dim() else v.backward()
        out[mode] = (v.detach(), Xg.grad, Yg.grad)
    for s, b in zip(out["serial"], out["bands"]):
        assert s is not None and torch.equal(s, b)
