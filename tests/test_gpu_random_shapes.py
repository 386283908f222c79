"""GPU differential test: random shapes across all three solvers against the fp64 C oracle."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from parity import rel_entry, rel_max

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        T = int(rng.choice([3, 4, 5, 8, 16, 17, 31, 32, 33, 48, 63, 64, 65, 66, 96, 127, 128]))
        d = int(rng.integers(1, 17))
        A, B = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        n_dy = int(rng.choice([0, 0, 0, 1, 2])) if T <= 17 else 0
        out.append((A, B, T, d, n_dy, float(rng.choice([0.3, 1.0, 4.0])), int(rng.integers(0, 1 << 30))))
    return out


@pytest.mark.parametrize("A,B,T,d,n,h,seed", _cases(48, 2026))
def test_random_shape_vs_oracle(gpu, A, B, T, d, n, h, seed):
    from sigsvgd_amd import ops

    rng = np.random.default_rng(seed)
    scale = 0.05 if T > 64 else 0.08
    X = np.cumsum(scale * rng.standard_normal((A, T, d)), axis=1).astype(np.float32)
    Y = np.cumsum(scale * rng.standard_normal((B, T, d)), axis=1).astype(np.float32)
    go = rng.uniform(0.5, 1.5, (A, B)).astype(np.float32)
    Kref, gref = C.gram_fwd_bwd(X, Y, h, n, grad_out=go.astype(np.float64))
    Xg, Yg, gog = (torch.as_tensor(t, device=gpu) for t in (X, Y, go))
    K, g = ops.gram_fwd_bwd(Xg, Yg, 1.0 / h, n, grad_out=gog)
    assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < TOL and rel_max(g.cpu().numpy(), gref) < TOL
    assert rel_max(ops.gram_fwd(Xg, Yg, 1.0 / h, n).cpu().numpy(), Kref) < TOL
    if A == B:  # the symmetric solve on X itself
        Ks, gs = C.gram_fwd_bwd(X, X, h, n, grad_out=go.astype(np.float64))
        K2, g2 = ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, n, grad_out=gog, y_is_x=True)
        assert rel_entry(K2.cpu().numpy(), Ks, 1e-6) < TOL and rel_max(g2.cpu().numpy(), gs) < TOL
