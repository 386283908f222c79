"""The distance select on the device (`ops.path_sqdist_select`, csrc/sqdist_select.hip) against sorted oracle tensors and
exact counts, and the default (median) bandwidth of `SignatureKernel` through it."""
import numpy as np
import pytest
import torch

from oracle import sigkernel_oracle as O
from sigsvgd_amd import ops

pytestmark = pytest.mark.gpu
TOL = 1e-5  # the suite's per-entry bound on K (tests/test_gpu_api.py)


def _int_paths(shape, lim, seed):
    return np.random.default_rng(seed).integers(-lim, lim + 1, size=shape).astype(np.float64)


def _ranks(n, seed):
    med = (n - 1) // 2
    fixed = [0, n - 1, med, max(med - 1, 0), min(med + 1, n - 1)]
    return fixed + [int(r) for r in np.random.default_rng(seed).integers(0, n, 12)]


def _bits(v):
    return np.asarray(v, np.float64).view(np.int64)


def _select(X, Y, rank, dev, dtype):
    Xt = torch.as_tensor(X, dtype=dtype, device=dev)
    Yt = None if Y is None else torch.as_tensor(Y, dtype=dtype, device=dev)
    out = ops.path_sqdist_select(Xt, Yt, rank)
    assert out.dtype == torch.float64 and out.dim() == 0 and out.device.type == "cuda"
    return float(out)


# the last three rows are this file's own: channels past one staged block (the channel-block loop), without and with Y = X,
# and more rows than one workgroup's 256 with TY no multiple of the column block
EXACT_SHAPES = [(1, 1, 2, 2, 1, False), (5, 7, 9, 4, 3, False), (3, 3, 64, 64, 7, False), (2, 3, 65, 130, 17, False),
                (9, 9, 33, 33, 2, True), (2, 3, 70, 9, 45, False), (2, 2, 300, 5, 3, False), (4, 4, 7, 7, 50, True)]


@pytest.mark.parametrize("A,B,TX,TY,d,y_is_x", EXACT_SHAPES)
def test_exact_with_ties(gpu, A, B, TX, TY, d, y_is_x):
    """Integer coordinates in [-3, 3]: both distance forms are exact, so the select equals the sorted oracle tensor's entry
    bit for bit, at every rank tried, for fp32 and fp64 storage."""
    X = _int_paths((A, TX, d), 3, 10 * A + d)
    Y = X if y_is_x else _int_paths((B, TY, d), 3, 10 * B + d + 1)
    ref = np.sort(O.pairwise_sqdist(X, Y).ravel())
    n = A * B * TX * TY
    assert ref.size == n
    for dtype in (torch.float32, torch.float64):
        for rank in _ranks(n, n):
            got = _select(X, None if y_is_x else Y, rank, gpu, dtype)
            assert _bits(got) == _bits(ref[rank]), (rank, got, ref[rank], dtype)
        # the default rank is the lower median, torch.median's
        got = _select(X, None if y_is_x else Y, None, gpu, dtype)
        assert _bits(got) == _bits(ref[(n - 1) // 2])
        assert got == float(torch.median(torch.as_tensor(O.pairwise_sqdist(X, Y))))


def _delta(X, Y, d):
    """The bound of the real-valued comparisons: an order statistic is 1-Lipschitz in the sup norm of the elements, and
    4 (d + 3) 2^-53 (max |x|^2 + max |y|^2) is a safe envelope over the rounding of both distance forms."""
    return 4 * (d + 3) * 2.0**-53 * (float((X**2).sum(-1).max()) + float((Y**2).sum(-1).max()))


@pytest.mark.parametrize("shift", [0.0, 100.0])
def test_real_valued_paths(gpu, shift):
    A, B, T, d = 6, 5, 20, 3
    X = O.synthetic_inputs(A, T, d, 0, 1)[0].numpy() + np.float32(shift)
    Y = O.synthetic_inputs(B, T, d, 2, 3)[0].numpy() + np.float32(shift)
    assert X.dtype == np.float32
    X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
    ref = np.sort(O.pairwise_sqdist(X64, Y64).ravel())
    n = ref.size
    delta = _delta(X64, Y64, d)
    for (P, Q, dtype) in [(X, Y, torch.float32), (X64, Y64, torch.float64)]:
        for rank in _ranks(n, 7):
            got = _select(P, Q, rank, gpu, dtype)
            print(f"shift {shift} rank {rank}: |m - m_ref| = {abs(got - ref[rank]):.3e}, bound {delta:.3e}")
            assert abs(got - ref[rank]) <= delta, (rank, got, ref[rank], delta)
    refx = np.sort(O.pairwise_sqdist(X64, X64).ravel())
    deltax = _delta(X64, X64, d)
    for rank in _ranks(refx.size, 8):
        assert abs(_select(X, None, rank, gpu, torch.float32) - refx[rank]) <= deltax


def test_all_points_equal(gpu):
    """Every distance is 0: no digit ever splits the bucket, the select runs its six passes and ends with 0.0 exactly."""
    X = torch.full((20, 64, 3), 1.25, dtype=torch.float32, device=gpu)
    n = 20 * 20 * 64 * 64  # (more than the select's candidate buffer holds: every pass recomputes)
    for Y in (X.clone(), None):
        for rank in (0, (n - 1) // 2, n - 1):
            out = ops.path_sqdist_select(X, Y, rank)
            assert _bits(float(out)) == _bits(0.0)
            assert ops.path_sqdist_select_passes(gpu) == 6
    small = torch.full((2, 3, 2), -7.0, dtype=torch.float64, device=gpu)  # fits the candidate buffer from the start
    assert _bits(float(ops.path_sqdist_select(small))) == _bits(0.0)
    assert ops.path_sqdist_select_passes(gpu) == 1


@pytest.mark.parametrize("A,T,d", [(9, 33, 2), (6, 40, 5), (801, 8, 1), (1, 5, 3), (2, 70, 47)])
def test_y_is_x_equals_the_unflagged_call(gpu, A, T, d):
    """One buffer in both slots: the flagged call (each unordered pair once, counted twice) returns the unflagged call's
    bits.  Odd and even A; A = 801, T = 8 has 3204 (flagged) and 5607 (unflagged) work items for at most 768 resident
    workgroups."""
    g = torch.Generator().manual_seed(A)
    X = (0.3 * torch.randn(A, T, d, generator=g, dtype=torch.float64)).cumsum(1).float().to(gpu)
    n = A * A * T * T
    for rank in [None, 0, n - 1] + [int(r) for r in np.random.default_rng(A).integers(0, n, 4)]:
        a, b = ops.path_sqdist_select(X, None, rank), ops.path_sqdist_select(X, X, rank)
        assert torch.equal(a, b), (rank, float(a), float(b))
    if n <= 1 << 22:
        Xn = X.double().cpu().numpy()
        ref = np.sort(O.pairwise_sqdist(Xn, Xn).ravel())
        assert abs(float(ops.path_sqdist_select(X)) - ref[(n - 1) // 2]) <= _delta(Xn, Xn, d)


def _counts(X, Y, lo, hi):
    """(#{dist < lo}, #{dist <= hi}) over all |X_ip - Y_jq|^2, with torch in fp64 over row chunks [1, B, TX, TY] (expansion
    form, as the reference's tensor)"""
    X, Y = X.double(), Y.double()
    Yf = Y.reshape(-1, Y.shape[2])
    ys = (Yf**2).sum(1)
    below = torch.zeros((), dtype=torch.int64, device=X.device)
    upto = torch.zeros((), dtype=torch.int64, device=X.device)
    for i in range(X.shape[0]):
        D = (X[i]**2).sum(1)[:, None] + ys[None, :] - 2.0 * (X[i] @ Yf.T)
        below += (D < lo).sum()
        upto += (D <= hi).sum()
    return int(below), int(upto)


def test_counts_past_2_to_32(gpu):
    """n = 2^33 elements: the totals and prefix sums of the select pass 2^32.  Integer coordinates in [-8, 8], so the
    counting reference has no rounding: #{dist < m} <= rank < #{dist <= m}."""
    A = B = 1024
    TX, TY, d = 64, 128, 2
    X = torch.as_tensor(_int_paths((A, TX, d), 8, 1), dtype=torch.float32, device=gpu)
    Y = torch.as_tensor(_int_paths((B, TY, d), 8, 2), dtype=torch.float32, device=gpu)
    n = A * B * TX * TY
    assert n == 2**33
    for rank in ((n - 1) // 2, n - 1):
        m = float(ops.path_sqdist_select(X, Y, rank))
        below, upto = _counts(X, Y, m, m)
        print(f"rank {rank}: m = {m}, #(< m) = {below}, #(<= m) = {upto}")
        assert m == int(m) and below <= rank < upto, (rank, m, below, upto)


def test_capture_and_replay(gpu):
    g = torch.Generator().manual_seed(5)
    X = (0.3 * torch.randn(7, 40, 3, generator=g, dtype=torch.float64)).cumsum(1).float().to(gpu)
    X2 = (0.5 * torch.randn(7, 40, 3, generator=g, dtype=torch.float64)).cumsum(1).float().to(gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        ops.path_sqdist_select(X)  # warm-up: loads the code objects
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.path_sqdist_select(X)
    graph.replay()
    torch.cuda.synchronize(gpu)
    first = out.clone()
    assert torch.equal(first, ops.path_sqdist_select(X))
    X.copy_(X2)
    graph.replay()
    torch.cuda.synchronize(gpu)
    eager = ops.path_sqdist_select(X2)
    assert torch.equal(out, eager) and not torch.equal(out, first)


def test_default_bandwidth_end_to_end_small(gpu, monkeypatch):
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd.kernels import SignatureKernel

    N, T, d = 24, 20, 3
    X = O.synthetic_inputs(N, T, d)[0]
    calls = []
    real = ops.path_sqdist_select

    def spy(*a, **k):
        calls.append("select")
        return real(*a, **k)

    def refuse(*a, **k):
        raise AssertionError("the distance tensor was formed")

    monkeypatch.setattr(ops, "path_sqdist_select", spy)
    monkeypatch.setattr(sk, "gram_sqdist", refuse)
    Xd = X.to(gpu)
    K = SignatureKernel(depth=0)(Xd, Xd)
    assert calls == ["select"]
    Xn = X.double().numpy()
    Kr = O.gram(Xn, Xn, O.RBF, O.bw_median(O.pairwise_sqdist(Xn, Xn)), 0)
    err = float((np.abs(K.double().cpu().numpy() - Kr) / np.maximum(np.abs(Kr), 1e-6)).max())
    print(f"max relative error of K: {err:.3e}")
    assert err < TOL


def test_default_bandwidth_where_the_tensor_would_not_fit(gpu):
    """N = 384, T = 64: the [N, N, T, T] fp64 tensor would be 4.5 GiB, past what the torch path forms."""
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd.kernels import SignatureKernel
    from sigsvgd_amd.utils.math import bw_from_median

    N, T, d = 384, 64, 3
    X = O.synthetic_inputs(N, T, d)[0].to(gpu)
    n = N * N * T * T
    assert n * 8 > sk._MAX_DIST_BYTES
    kern = SignatureKernel(depth=0)
    K = kern(X, X)
    assert K.shape == (N, N) and bool(torch.isfinite(K).all())
    m = ops.path_sqdist_select(X)
    assert kern.kernel.static_kernel.inv_bandwidth(X, X) == 1.0 / float(bw_from_median(m, N))
    Xn = X.double().cpu().numpy()
    delta = _delta(Xn, Xn, d)
    rank = (n - 1) // 2
    below, upto = _counts(X, X, float(m) - delta, float(m) + delta)
    print(f"m = {float(m)!r}, delta = {delta:.3e}, #(< m - delta) = {below}, #(<= m + delta) = {upto}, rank = {rank}")
    assert below <= rank < upto
