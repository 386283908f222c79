"""GPU: the fixed-window twin of the register-resident Gram kernel (gram_fast.hip, PFIX = 63) against its table form.

Gram + gradient launches of 64-point paths run the kernel whose PDE sweeps write their EXEC lane windows from immediates;
SIGSVGD_SWEEP_WINDOWS=table sends the same launch to the kernel that reads the windows from the constant table, which is what
every other path length runs.  The two differ in how a window reaches EXEC and in nothing else -- same instructions, same
order, same lanes and slots, fixed-order reductions -- so K and the gradient must be EQUAL bit for bit: the comparisons
below are torch.equal.  Shapes: d = 3, 7, 14 (the 4-, 8- and 16-channel instantiations; 3 and 7 are their padded d = DPAD - 1
forms, 14 the unpadded one), ordered and Y-is-X launches with signed weights, sizes at which a workgroup takes several items
(asserted from the launch geometry), and both shares of a two-rank partial solve.  One launch per shape is also held to the
fp64 C oracle at the neighbouring files' 1e-5.  At T = 63 and T = 65, and for forward-only launches at T = 64, the variable
changes nothing."""
import pytest
import torch

from oracle import c_oracle as C
from parity import rel_entry, rel_max, signed_weights, walks
from plans import device_cus, gram_geometry

pytestmark = pytest.mark.gpu

TOL = 1e-5  # tests/test_gpu_partition.py, tests/test_gpu_fast.py
HOOK = "SIGSVGD_SWEEP_WINDOWS"
DS = [3, 7, 14]


def _both(monkeypatch, run):
    """run() on the default path and with the table path forced -> (default, table)"""
    monkeypatch.delenv(HOOK, raising=False)
    a = run()
    torch.cuda.synchronize()
    monkeypatch.setenv(HOOK, "table")
    b = run()
    torch.cuda.synchronize()
    monkeypatch.delenv(HOOK, raising=False)
    return a, b


def _several_items(A, B, T, d, sym):
    g = gram_geometry(A, B, T, d, 0, True, sym, device_cus())
    assert g is not None and g["family"] == "fast", g
    print(f"{'Y is X' if sym else 'ordered'} {A} x {B}, T={T} d={d}: {g['rows_per_tile']} rows per tile, {g['items']} items on "
          f"{g['grid']} workgroups")
    assert g["items"] >= 2 * g["grid"] + 1, g  # every workgroup loops over items
    return g


@pytest.mark.parametrize("d", DS)
def test_ordered_launch_equals_table_path(gpu, monkeypatch, d):
    """X != Y, 67 x 131 with signed weights; this launch is also the shape's oracle case"""
    from sigsvgd_amd import ops

    A, B, T, h = 67, 131, 64, 0.9
    _several_items(A, B, T, d, False)
    X, Y = walks(A, T, d, 11, 0.05), walks(B, T, d, 12, 0.05)
    go = signed_weights(A, B, 13)
    Xg, Yg = torch.as_tensor(X, device=gpu), torch.as_tensor(Y, device=gpu)
    gog = torch.as_tensor(go, device=gpu, dtype=torch.float32)
    (K, gx), (Kt, gxt) = _both(monkeypatch, lambda: ops.gram_fwd_bwd(Xg, Yg, 1.0 / h, 0, grad_out=gog))
    assert torch.equal(K, Kt)
    assert torch.equal(gx, gxt)
    Kref, gref = C.gram_fwd_bwd(X, Y, h, 0, grad_out=go)
    eK, eg = rel_entry(K.cpu().numpy(), Kref, 1e-6), rel_max(gx.cpu().numpy(), gref)
    print(f"against the oracle: K {eK:.2e} gradient {eg:.2e}")
    assert eK < TOL and eg < TOL


@pytest.mark.parametrize("weights", ["signed", "signed-sym", "ones"])
@pytest.mark.parametrize("d", DS)
def test_symmetric_launch_equals_table_path(gpu, monkeypatch, d, weights):
    """Y is X at N = 264: 33 (d = 14: 66) row tiles, about 17 items a workgroup on 256 CUs"""
    from sigsvgd_amd import ops

    N, T, h = 264, 64, 1.1
    _several_items(N, N, T, d, True)
    X = walks(N, T, d, 21, 0.05)
    Xg = torch.as_tensor(X, device=gpu)
    gog = None if weights == "ones" else torch.as_tensor(signed_weights(N, N, 23), device=gpu, dtype=torch.float32)
    sym = weights == "signed-sym"
    (K, gx), (Kt, gxt) = _both(monkeypatch, lambda: ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, 0, grad_out=gog, sym=sym, y_is_x=True))
    assert torch.equal(K, Kt)
    assert torch.equal(gx, gxt)
    assert torch.equal(K, K.T)


@pytest.mark.parametrize("d", DS)
def test_fp64_io_equals_table_path(gpu, monkeypatch, d):
    """the same kernels with fp64 inputs and outputs (a run-time switch of the loads and stores)"""
    from sigsvgd_amd import ops

    N, T, h = 93, 64, 1.0
    Xg = torch.as_tensor(walks(N, T, d, 25, 0.05), device=gpu).double()
    gog = torch.as_tensor(signed_weights(N, N, 26), device=gpu, dtype=torch.float64)
    (K, gx), (Kt, gxt) = _both(monkeypatch, lambda: ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, 0, grad_out=gog, y_is_x=True))
    assert K.dtype == torch.float64 and torch.equal(K, Kt)
    assert torch.equal(gx, gxt)


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("d", DS)
def test_partial_shares_equal_table_path(gpu, monkeypatch, d, fold):
    """the sharded partial entry point at world size 2: each share bit for bit, and the shares' K adds up to the full launch's"""
    from sigsvgd_amd import ops

    N, T, h, world = 264, 64, 1.0, 2
    X = walks(N, T, d, 31, 0.05)
    Xg = torch.as_tensor(X, device=gpu)
    gog = torch.as_tensor(signed_weights(N, N, 33), device=gpu, dtype=torch.float32)
    Ks = None
    for r in range(world):
        (Kp, gp), (Kpt, gpt) = _both(monkeypatch, lambda: ops.gram_sym_partial(Xg, 1.0 / h, r, world, grad_out=gog, fold=fold))
        assert torch.equal(Kp, Kpt)
        assert torch.equal(gp, gpt)
        Ks = Kp if Ks is None else Ks + Kp
    K, _ = ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, 0, grad_out=gog, y_is_x=True)
    torch.cuda.synchronize()
    assert torch.equal(Ks, K)


@pytest.mark.parametrize("T", [63, 65])
@pytest.mark.parametrize("d", DS)
def test_hook_changes_nothing_at_other_lengths(gpu, monkeypatch, T, d):
    """T = 63 stays on the table form of the same kernel, T = 65 is the quadrant kernel's: the variable is not looked at"""
    from sigsvgd_amd import ops

    N, h = 93, 1.0
    X = walks(N, T, d, 41, 0.05)
    Xg = torch.as_tensor(X, device=gpu)
    go = signed_weights(N, N, 43)
    gog = torch.as_tensor(go, device=gpu, dtype=torch.float32)
    (K, gx), (Kt, gxt) = _both(monkeypatch, lambda: ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, 0, grad_out=gog, y_is_x=True))
    assert torch.equal(K, Kt)
    assert torch.equal(gx, gxt)
    (Ko, gxo), (Kot, gxot) = _both(monkeypatch, lambda: ops.gram_fwd_bwd(Xg, Xg.clone(), 1.0 / h, 0, grad_out=gog))
    assert torch.equal(Ko, Kot)
    assert torch.equal(gxo, gxot)
    Kref, gref = C.gram_fwd_bwd(X, X, h, 0, grad_out=go)
    assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < TOL and rel_max(gx.cpu().numpy(), gref) < TOL


@pytest.mark.parametrize("d", DS)
def test_forward_only_launch_has_the_table_path_only(gpu, monkeypatch, d):
    from sigsvgd_amd import ops

    N, T, h = 109, 64, 1.0
    Xg = torch.as_tensor(walks(N, T, d, 51, 0.05), device=gpu)
    K, Kt = _both(monkeypatch, lambda: ops.gram_fwd(Xg, Xg, 1.0 / h, 0, y_is_x=True))
    assert torch.equal(K, Kt)
