"""The numpy reference of the radial static kernels (tests/radial_reference.py) against the oracle where the oracle knows
the kernel (RBF), against finite differences and its own symmetry, the torch restatements of the new static kernels against
it, and the property the kernels are for: paths far apart keep a signature-kernel gradient under IMQ and lose it under RBF.
No device needed."""
import numpy as np
import pytest
import torch

import radial_reference as RR
from oracle import sigkernel_oracle as O


def _synthetic(A, T, d, seed):
    return O.synthetic_inputs(A, T, d, seed_x=seed)[0].double().numpy()


@pytest.mark.parametrize("n,sym", [(0, False), (1, False), (2, True)])
def test_helper_reproduces_the_oracle_for_rbf(n, sym):
    X, Y = _synthetic(3, 9, 3, 0), _synthetic(3, 9 if sym else 7, 3, 5)
    w = np.random.default_rng(1).standard_normal((3, 3))
    Kr, gr = O.gram_backward(X, Y, w, O.RBF, 0.7, n, sym=sym)
    K, gX, _ = RR.gram_backward(X, Y, w, RR.RBF, 0.7, n, sym=sym)
    assert np.abs(K - Kr).max() / np.abs(Kr).max() < 1e-12
    assert np.abs(gX - gr).max() / np.abs(gr).max() < 1e-12


@pytest.mark.parametrize("kind", [RR.RBF, RR.IMQ, RR.RQ])
def test_slope_matches_central_differences(kind):
    s = np.linspace(0.0, 40.0, 801)
    e = 1e-5
    fd = (RR.phi(kind, s + e) - RR.phi(kind, np.maximum(s - e, -e))) / (s + e - np.maximum(s - e, -e))
    assert np.abs(-fd - RR.neg_dphi(kind, s)).max() < 1e-9


@pytest.mark.parametrize("kind", [RR.IMQ, RR.RQ])
def test_second_slot_is_the_first_slot_of_the_swapped_call(kind):
    X, Y = _synthetic(3, 8, 2, 0), _synthetic(4, 6, 2, 5)
    w = np.random.default_rng(2).standard_normal((3, 4))
    K, gX, gY = RR.gram_backward(X, Y, w, kind, 1.3, 1)
    Kt, gXt, gYt = RR.gram_backward(Y, X, w.T, kind, 1.3, 1)
    assert np.abs(K - Kt.T).max() < 1e-13
    assert np.abs(gY - gXt).max() <= 1e-13 * np.abs(gY).max() and np.abs(gX - gYt).max() <= 1e-13 * np.abs(gX).max()
    # the gradient is the derivative of sum(w K) (the GG convention is exact to O(increment^2): a loose bound)
    e = 1e-6
    Xp, Xm = X.copy(), X.copy()
    Xp[1, 3, 0] += e
    Xm[1, 3, 0] -= e
    fd = ((w * RR.gram(Xp, Y, kind, 1.3, 1)).sum() - (w * RR.gram(Xm, Y, kind, 1.3, 1)).sum()) / (2 * e)
    assert abs(fd - gX[1, 3, 0]) < 2e-2 * np.abs(gX).max()


@pytest.mark.parametrize("kind", [RR.IMQ, RR.RQ])
def test_pairs_are_the_diagonal(kind):
    X, Y = _synthetic(3, 8, 2, 0), _synthetic(3, 6, 2, 5)
    K, gX, gY = RR.pair_backward(X, Y, np.array([1.0, -2.0, 0.5]), kind, 0.9, 1)
    Kg, gXg, gYg = RR.gram_backward(X, Y, np.diag([1.0, -2.0, 0.5]), kind, 0.9, 1)
    assert np.allclose(K, np.diag(Kg), rtol=0, atol=1e-14)
    assert np.allclose(gX, gXg, rtol=0, atol=1e-14) and np.allclose(gY, gYg, rtol=0, atol=1e-14)


def test_torch_restatements_match_the_helper():
    from sigsvgd_amd import _lib
    from sigsvgd_amd.kernels import BatchIMQKernel, BatchRationalQuadraticKernel
    from sigsvgd_amd.sigkernel import IMQStaticKernel, RationalQuadraticKernel, _resolve_static

    X, Y = _synthetic(3, 8, 2, 0), _synthetic(3, 6, 2, 5)
    Xt, Yt = torch.as_tensor(X), torch.as_tensor(Y)
    for kind, cls, bcls in [(RR.IMQ, IMQStaticKernel, BatchIMQKernel), (RR.RQ, RationalQuadraticKernel, BatchRationalQuadraticKernel)]:
        G = RR.static_gram(X, Y, kind, 0.8)
        for k in (cls(0.8), bcls(lambda _: 0.8)):
            assert np.abs(k.Gram_matrix(Xt, Yt).numpy() - G).max() < 1e-13
            assert np.abs(k.batch_kernel(Xt, Yt).numpy() - G[np.arange(3), np.arange(3)]).max() < 1e-13
            assert _resolve_static(k, Xt, Yt) == (kind, 1.0 / 0.8)
        assert (cls.static_kind, bcls.static_kind) == (kind, kind)
    assert (_lib.STATIC_IMQ, _lib.STATIC_RQ) == (2, 3)
    # a data-dependent bandwidth on CPU tensors: the reference's median of the distance tensor
    h = O.bw_median(O.pairwise_sqdist(X, Y))
    kind, inv_h = _resolve_static(BatchIMQKernel(), Xt, Yt)
    assert kind == RR.IMQ and abs(inv_h * h - 1.0) < 1e-6


def test_signature_kernel_takes_a_static_kernel():
    from sigsvgd_amd.kernels import BatchGaussianKernel, BatchIMQKernel, BatchRationalQuadraticKernel, SignatureKernel
    from sigsvgd_amd.sigkernel import IMQStaticKernel, SigKernel

    for arg, cls in [(None, BatchGaussianKernel), ("rbf", BatchGaussianKernel), ("imq", BatchIMQKernel),
                     ("rq", BatchRationalQuadraticKernel)]:
        k = SignatureKernel(lambda _: 0.5, depth=2, static_kernel=arg)
        assert isinstance(k.kernel, SigKernel) and type(k.kernel.static_kernel) is cls and k.kernel.dyadic_order == 2
        assert k.kernel.static_kernel.get_bandwidth(None) == 0.5
    own = IMQStaticKernel(2.0)
    assert SignatureKernel(depth=1, static_kernel=own).kernel.static_kernel is own
    with pytest.raises(ValueError):
        SignatureKernel(static_kernel="cauchy")


def test_distant_bundles_repel_under_imq_and_not_under_rbf():
    """Two bundles of 4 smooth paths, 30 apart in every coordinate, h from the median heuristic: RBF's static kernel
    underflows between the bundles, so their signature kernel is exactly 1 and its gradient exactly 0; IMQ's is not."""
    X = RR.separated_bundles()
    h = O.bw_median(O.pairwise_sqdist(X, X))
    cross = np.zeros((8, 8))
    cross[:4, 4:] = cross[4:, :4] = 1.0
    K, gX, _ = RR.gram_backward(X, X, cross, RR.RBF, h, 0)
    assert np.all(K[:4, 4:] == 1.0) and np.all(K[4:, :4] == 1.0) and np.all(gX == 0.0)
    Ko, go = O.gram_backward(X, X, cross, O.RBF, h, 0)
    assert np.all(Ko[:4, 4:] == 1.0) and np.all(go == 0.0)
    for kind in (RR.IMQ, RR.RQ):
        K, gX, _ = RR.gram_backward(X, X, cross, kind, h, 0)
        assert np.all(K[:4, 4:] != 1.0) and np.abs(gX).max() > 0.0
        assert np.all(np.abs(gX).max(axis=(1, 2)) > 0.0)  # every path is pushed
