"""GPU: the half-offset twin that stages its columns from images formed once per launch (gram_fast_kernel.h, HALF = 2;
fast_column_image_kernel in gram_fast.hip) against the half-offset twin that forms them in every item (HALF = 1).

A symmetric launch of N paths stages about N^2 / 16 items and has N distinct columns.  What a workgroup forms of a column when
it stages it -- the points centred on the first one, in fp64; the scaled norm of every point; the first point -- depends on the
column and the bandwidth alone, so a small kernel forms it once per column into the workspace and the pair kernel copies it.
SIGSVGD_COLUMN_IMAGES=off keeps the launch on the HALF = 1 twin.  Every number is formed from the same operands by the same
operations (the norm: `column_norm` in gram_fast.hip states the contraction hipcc applies in the twin), so K and the gradient
must be EQUAL byte for byte: torch.equal below, on the shapes of tests/test_gpu_half_offset.py -- N = 200 (ranges of several
items that cross row tiles, both buffer parities), 8 (one tile, the diagonal pair first), 9 (a last tile of one row), 17 with
signed weights, 17 with fp64 inputs (the image holds the inputs themselves, not their conversions) -- and on one launch of the
fused partial solve per tile stride.  One launch is also held to the fp64 C oracle at the tolerance
tests/test_gpu_fixed_windows.py has for this kernel."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from parity import rel_entry, rel_max, signed_weights, walks
from plans import gram_multi_item_regime
from test_gpu_half_offset import H, T, TOL, _family

pytestmark = pytest.mark.gpu

HOOK = "SIGSVGD_COLUMN_IMAGES"
D = 7


def _both(monkeypatch, run):
    """run() on the default path and with the launch kept on the twin without the images -> (default, off)"""
    monkeypatch.delenv("SIGSVGD_HALF_OFFSET", raising=False)
    monkeypatch.delenv("SIGSVGD_SWEEP_WINDOWS", raising=False)
    monkeypatch.delenv(HOOK, raising=False)
    a = run()
    torch.cuda.synchronize()
    monkeypatch.setenv(HOOK, "off")
    b = run()
    torch.cuda.synchronize()
    monkeypatch.delenv(HOOK, raising=False)
    return a, b


def _on_off(gpu, monkeypatch, N, seed, weights=None, dtype=np.float32):
    from sigsvgd_amd import ops

    Xg = torch.as_tensor(walks(N, T, D, seed, 0.05).astype(dtype), device=gpu)
    gog = None if weights is None else torch.as_tensor(weights, device=gpu, dtype=Xg.dtype)
    (K, gx), (Ko, gxo) = _both(monkeypatch, lambda: ops.gram_fwd_bwd(Xg, Xg, 1.0 / H, 0, grad_out=gog, y_is_x=True))
    assert K.shape == (N, N) and gx.shape == (N, T, D) and K.dtype == Xg.dtype
    assert bool(torch.isfinite(K).all()) and bool(torch.isfinite(gx).all())
    assert float(gx.abs().max()) > 0.0
    assert torch.equal(K, Ko)
    assert torch.equal(gx, gxo)
    assert torch.equal(K, K.T)


def test_ranges_of_several_items_equal_the_twin_without_images(gpu, monkeypatch):
    """N = 200: 25 row tiles, 2,600 items; every workgroup loops over items and some ranges cross into the next tile"""
    N = 200
    g = _family(N, D)
    r = gram_multi_item_regime(N, N, g, True)
    print(f"Y is X {N} x {N}, T={T} d={D}: {g['items']} items on {g['grid']} workgroups, {r}")
    assert g["items"] >= 2 * g["grid"] + 1 and r["multi"] and r["crosses"], (g, r)
    _on_off(gpu, monkeypatch, N, 261)


def test_one_tile_diagonal_first_equals_the_twin_without_images(gpu, monkeypatch):
    """N = 8: one tile; the first item is the diagonal pair"""
    g = _family(8, D)
    assert g["items"] == 8, g
    _on_off(gpu, monkeypatch, 8, 271)


def test_last_tile_of_one_row_equals_the_twin_without_images(gpu, monkeypatch):
    """N = 9: the second tile holds row 8 alone"""
    _family(9, D)
    _on_off(gpu, monkeypatch, 9, 273)


def test_signed_weights_equal_the_twin_without_images(gpu, monkeypatch):
    N = 17
    _family(N, D)
    _on_off(gpu, monkeypatch, N, 281, weights=signed_weights(N, N, 283))


def test_fp64_inputs_equal_the_twin_without_images(gpu, monkeypatch):
    """fp64 paths with bits below fp32: the image's differences and first points are those of the inputs themselves"""
    N = 17
    _family(N, D)
    rng = np.random.default_rng(285)
    X = walks(N, T, D, 287, 0.05).astype(np.float64) * (1.0 + 1e-9 * rng.standard_normal((N, T, D)))
    assert not np.array_equal(X, X.astype(np.float32).astype(np.float64))
    from sigsvgd_amd import ops

    Xg = torch.as_tensor(X, device=gpu)
    (K, gx), (Ko, gxo) = _both(monkeypatch, lambda: ops.gram_fwd_bwd(Xg, Xg, 1.0 / H, 0, y_is_x=True))
    assert K.dtype == torch.float64 and bool(torch.isfinite(K).all()) and float(gx.abs().max()) > 0.0
    assert torch.equal(K, Ko)
    assert torch.equal(gx, gxo)


@pytest.mark.parametrize("stride", [2, 3])
def test_partial_solve_equals_the_twin_without_images(gpu, monkeypatch, stride):
    """N = 24, three tiles: one launch of the fused partial solve that owns every `stride`-th tile from the last offset on"""
    from sigsvgd_amd import ops

    N = 24
    _family(N, D)
    Xg = torch.as_tensor(walks(N, T, D, 291, 0.05), device=gpu)
    (Kp, gp), (Kpo, gpo) = _both(monkeypatch, lambda: ops.gram_sym_partial(Xg, 1.0 / H, stride - 1, stride))
    assert Kp.shape == (N, N) and gp.shape == (N, T, D)
    assert float(Kp.abs().max()) > 0.0 and float(gp.abs().max()) > 0.0
    assert torch.equal(Kp, Kpo)
    assert torch.equal(gp, gpo)


def test_image_twin_against_the_oracle(gpu, monkeypatch):
    """N = 24, T = 64, d = 7 on the default path: K per entry (floor 1e-6) and the gradient of its maximum"""
    from sigsvgd_amd import ops

    for hook in (HOOK, "SIGSVGD_HALF_OFFSET", "SIGSVGD_SWEEP_WINDOWS"):
        monkeypatch.delenv(hook, raising=False)
    N = 24
    _family(N, D)
    X = walks(N, T, D, 293, 0.05)
    Xg = torch.as_tensor(X, device=gpu)
    K, gx = ops.gram_fwd_bwd(Xg, Xg, 1.0 / H, 0, y_is_x=True)
    torch.cuda.synchronize()
    Kref, gref = C.gram_fwd_bwd(X, X, H, 0)
    eK, eg = rel_entry(K.cpu().numpy(), Kref, 1e-6), rel_max(gx.cpu().numpy(), gref)
    print(f"against the oracle: K {eK:.2e} gradient {eg:.2e}")
    assert eK < TOL and eg < TOL
