"""GPU: the half-offset twin of the symmetric 7-channel Gram + gradient kernel (gram_fast_kernel.h, HALF = 1) against the kernel
it replaces.

Symmetric Gram + gradient launches of 64-point paths in 7 channels run the fixed-window kernel whose younger half of a workgroup
(waves 4..7) passes the pair's sync block between the forward and the reverse sweep, half a pair behind the older half;
SIGSVGD_HALF_OFFSET=off sends the same launch to the wave-balance twin.  The schedule changes when a wave runs a phase and where
the column's fp32 copy, the younger half's parked column sums and the older half's partial block sum wait in LDS; every value is
formed from the same operands in the same order, so K and the gradient must be EQUAL byte for byte: torch.equal below.
Shapes: N = 200 (about 2,600 items: ranges of several items that cross row tiles -- the tile's closing sync, the first interval
of a tile, and the column buffers of both parities -- asserted from the launch geometry); N = 8 (one tile, the first item is the
diagonal pair, and on column j waves j+1..7 have no pair and still pass both sync sites); N = 9 (a last tile of one row); N = 17
with signed weights.  d = 8, 3 and 4 keep their kernels: the switch changes nothing there.  One launch is also held to the fp64
C oracle at the tolerance tests/test_gpu_fixed_windows.py has for this kernel."""
import pytest
import torch

from oracle import c_oracle as C
from parity import rel_entry, rel_max, signed_weights, walks
from plans import device_cus, gram_geometry, gram_multi_item_regime

pytestmark = pytest.mark.gpu

TOL = 1e-5  # tests/test_gpu_fixed_windows.py
HOOK = "SIGSVGD_HALF_OFFSET"
T, H = 64, 1.1


def _both(monkeypatch, run):
    """run() on the default path and with the launch kept on the kernel without the offset -> (default, off)"""
    monkeypatch.delenv(HOOK, raising=False)
    a = run()
    torch.cuda.synchronize()
    monkeypatch.setenv(HOOK, "off")
    b = run()
    torch.cuda.synchronize()
    monkeypatch.delenv(HOOK, raising=False)
    return a, b


def _family(N, d):
    g = gram_geometry(N, N, T, d, 0, True, True, device_cus())
    assert g is not None and g["family"] == "fast" and g["rows_per_tile"] == 8, g
    return g


def _on_off(gpu, monkeypatch, N, d, seed, weights=None):
    from sigsvgd_amd import ops

    Xg = torch.as_tensor(walks(N, T, d, seed, 0.05), device=gpu)
    gog = None if weights is None else torch.as_tensor(weights, device=gpu, dtype=torch.float32)
    (K, gx), (Ko, gxo) = _both(monkeypatch, lambda: ops.gram_fwd_bwd(Xg, Xg, 1.0 / H, 0, grad_out=gog, y_is_x=True))
    assert K.shape == (N, N) and gx.shape == (N, T, d)
    assert bool(torch.isfinite(K).all()) and bool(torch.isfinite(gx).all())
    assert float(gx.abs().max()) > 0.0
    assert torch.equal(K, Ko)
    assert torch.equal(gx, gxo)
    assert torch.equal(K, K.T)


@pytest.mark.parametrize("d", [7, 8, 3, 4])
def test_ranges_of_several_items_equal_the_kernel_without_offset(gpu, monkeypatch, d):
    """N = 200: 25 row tiles, 2,600 items; every workgroup loops over items and some ranges cross into the next tile (d = 7: the
    twin; d = 8, 3, 4: the kernels they had, on either setting of the switch)"""
    N = 200
    g = _family(N, d)
    r = gram_multi_item_regime(N, N, g, True)
    print(f"Y is X {N} x {N}, T={T} d={d}: {g['items']} items on {g['grid']} workgroups, {r}")
    assert g["items"] >= 2 * g["grid"] + 1 and r["multi"] and r["crosses"], (g, r)
    _on_off(gpu, monkeypatch, N, d, 161 + d)


def test_one_tile_diagonal_first_equals_the_kernel_without_offset(gpu, monkeypatch):
    """N = 8: one tile; the first item is the diagonal pair (no column side), column j has pairs in waves 0..j only"""
    g = _family(8, 7)
    assert g["items"] == 8, g
    _on_off(gpu, monkeypatch, 8, 7, 171)


def test_last_tile_of_one_row_equals_the_kernel_without_offset(gpu, monkeypatch):
    """N = 9: the second tile holds row 8 alone, waves 1..7 of its workgroup have no pair"""
    _family(9, 7)
    _on_off(gpu, monkeypatch, 9, 7, 173)


def test_signed_weights_equal_the_kernel_without_offset(gpu, monkeypatch):
    N = 17
    _family(N, 7)
    _on_off(gpu, monkeypatch, N, 7, 181, weights=signed_weights(N, N, 183))


def test_half_offset_kernel_against_the_oracle(gpu, monkeypatch):
    """N = 24, T = 64, d = 7 on the default path: K per entry (floor 1e-6) and the gradient of its maximum"""
    from sigsvgd_amd import ops

    monkeypatch.delenv(HOOK, raising=False)
    N, d = 24, 7
    _family(N, d)
    X = walks(N, T, d, 191, 0.05)
    Xg = torch.as_tensor(X, device=gpu)
    K, gx = ops.gram_fwd_bwd(Xg, Xg, 1.0 / H, 0, y_is_x=True)
    torch.cuda.synchronize()
    Kref, gref = C.gram_fwd_bwd(X, X, H, 0)
    eK, eg = rel_entry(K.cpu().numpy(), Kref, 1e-6), rel_max(gx.cpu().numpy(), gref)
    print(f"against the oracle: K {eK:.2e} gradient {eg:.2e}")
    assert eK < TOL and eg < TOL
