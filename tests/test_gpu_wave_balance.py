"""GPU: the wave-balance twins of the symmetric 4- and 8-channel Gram + gradient kernels (gram_fast.hip, BAL != 0) against
the kernels without the schedule.

Symmetric Gram + gradient launches of 64-point paths in up to 8 channels run the fixed-window kernel whose two halves of
the workgroup hold `s_setprio 1` on different stretches of a pair; SIGSVGD_WAVE_BALANCE=off sends the same launch to the
kernel without those instructions.  A priority changes when an instruction issues and nothing it computes, and every
reduction has a fixed order, so K and the gradient must be EQUAL byte for byte: the comparisons below are torch.equal.
Shapes: N = 200 at d = 7 and d = 8 (the padded d = DPAD - 1 form and the unpadded one of the 8-channel kernel) and at d = 3
and d = 4 (the same two of the 4-channel kernel, with its flag pass); about 2,600 items, so every workgroup takes a range of
several items and ranges cross row tiles -- asserted from the launch geometry; d = 7 again with signed weights, and N = 9 (a
last tile of one row: seven of its waves have no pair and never raise their priority).
One launch is also held to the fp64 C oracle at the tolerance tests/test_gpu_fixed_windows.py has for this kernel."""
import pytest
import torch

from oracle import c_oracle as C
from parity import rel_entry, rel_max, signed_weights, walks
from plans import device_cus, gram_geometry, gram_multi_item_regime

pytestmark = pytest.mark.gpu

TOL = 1e-5  # tests/test_gpu_fixed_windows.py
HOOK = "SIGSVGD_WAVE_BALANCE"
T, H = 64, 1.1


def _both(monkeypatch, run):
    """run() with the schedule (the default) and with the launch sent to the twin without it -> (default, off)"""
    monkeypatch.delenv(HOOK, raising=False)
    a = run()
    torch.cuda.synchronize()
    monkeypatch.setenv(HOOK, "off")
    b = run()
    torch.cuda.synchronize()
    monkeypatch.delenv(HOOK, raising=False)
    return a, b


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
def test_ranges_of_several_items_equal_the_twin_without_schedule(gpu, monkeypatch, d):
    """N = 200: 25 row tiles, 2,600 items; every workgroup loops over items and some ranges cross into the next tile"""
    N = 200
    g = gram_geometry(N, N, T, d, 0, True, True, device_cus())
    assert g is not None and g["family"] == "fast" and g["rows_per_tile"] == 8, g
    r = gram_multi_item_regime(N, N, g, True)
    print(f"Y is X {N} x {N}, T={T} d={d}: {g['items']} items on {g['grid']} workgroups, {r}")
    assert g["items"] >= 2 * g["grid"] + 1 and r["crosses"], (g, r)
    _on_off(gpu, monkeypatch, N, d, 61 + d)


def test_last_tile_of_one_row_equals_the_twin_without_schedule(gpu, monkeypatch):
    """N = 9: the second tile holds row 8 alone, waves 1..7 of its workgroups have no pair"""
    _on_off(gpu, monkeypatch, 9, 7, 71)


def test_signed_weights_equal_the_twin_without_schedule(gpu, monkeypatch):
    N = 200
    _on_off(gpu, monkeypatch, N, 7, 81, weights=signed_weights(N, N, 83))


def test_scheduled_kernel_against_the_oracle(gpu, monkeypatch):
    """N = 24, T = 64, d = 7 on the default path: K per entry (floor 1e-6) and the gradient of its maximum"""
    from sigsvgd_amd import ops

    monkeypatch.delenv(HOOK, raising=False)
    N, d = 24, 7
    X = walks(N, T, d, 91, 0.05)
    Xg = torch.as_tensor(X, device=gpu)
    K, gx = ops.gram_fwd_bwd(Xg, Xg, 1.0 / H, 0, y_is_x=True)
    torch.cuda.synchronize()
    Kref, gref = C.gram_fwd_bwd(X, X, H, 0)
    eK, eg = rel_entry(K.cpu().numpy(), Kref, 1e-6), rel_max(gx.cpu().numpy(), gref)
    print(f"against the oracle: K {eK:.2e} gradient {eg:.2e}")
    assert eK < TOL and eg < TOL
