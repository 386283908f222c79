"""The gradient reduction with four elements per thread, and the window of gram_fast_kernel's RAW_STAGE instantiations
(csrc/sweep_host.hip: `grad_reduce_kernel<V>`; csrc/gram_fast_kernel.h: "the window between two pairs").

grad_reduce_kernel<4> serves launches whose T*d is a multiple of 4 with 16-byte loads (a thread owns 4 consecutive
elements of a column block); every other T*d runs grad_reduce_kernel<1>.  Either adds the same fp64 terms per element in
the same order.  The symmetric Gram + gradient launches below are the RAW_STAGE kernels (T = 64, d = 7 and 8) at sizes
where a workgroup walks several items, ranges cross tile boundaries, the last tile is partly empty, and -- the partial
entry point -- the reduction inverts a strided or folded tile map.  Every launch runs twice and must return the same
bytes.  Tolerances: tests/test_gpu_partition.py (K per entry, the gradient relative to its largest entry).
"""
import pytest
import torch

from oracle import c_oracle as C
from parity import rel_entry, rel_max, walks
from plans import device_cus, gram_geometry

pytestmark = pytest.mark.gpu

TOL = 1e-5
H = 1.1


_cache = {}


def _case(N, T, d, gpu):
    """inputs, the oracle's result and the full symmetric launch, once per shape"""
    key = (N, T, d)
    if key not in _cache:
        from sigsvgd_amd import ops

        X = walks(N, T, d, 51, 0.05)
        Kref, gref = C.gram_fwd_bwd(X, X, H, 0)
        Xg = torch.as_tensor(X, device=gpu)
        K, g = ops.gram_fwd_bwd(Xg, Xg, 1.0 / H, 0, y_is_x=True)
        torch.cuda.synchronize()
        _cache[key] = dict(Xg=Xg, Kref=Kref, gref=gref, K=K, g=g)
    return _cache[key]


@pytest.mark.parametrize("N,T,d", [(96, 64, 7), (96, 64, 8), (20, 64, 7), (24, 63, 7), (24, 33, 3)],
                         ids=["N96-d7", "N96-d8", "N20-d7", "T63-d7-scalar-reduction", "T33-d3-scalar-reduction"])
def test_full_launch_against_the_oracle_twice(gpu, N, T, d):
    from sigsvgd_amd import ops

    geom = gram_geometry(N, N, T, d, 0, True, True, device_cus())
    assert geom is not None and geom["family"] == "fast", geom
    if (N, T) == (96, 64):  # 12 row tiles, 624 items: more than one item per workgroup, ranges that cross tile boundaries
        assert geom["rows_per_tile"] == 8 and geom["items"] == 624 and geom["items"] > geom["grid"], geom
    if T == 64:
        assert (T * d) % 4 == 0  # the 16-byte reduction
    else:
        assert (T * d) % 4 != 0  # one element per thread
    s = _case(N, T, d, gpu)
    eK, eg = rel_entry(s["K"].cpu().numpy(), s["Kref"], 1e-6), rel_max(s["g"].cpu().numpy(), s["gref"])
    print(f"N={N} T={T} d={d}: {geom['items']} items on {geom['grid']} workgroups, K {eK:.2e} gradient {eg:.2e}")
    K2, g2 = ops.gram_fwd_bwd(s["Xg"], s["Xg"], 1.0 / H, 0, y_is_x=True)
    torch.cuda.synchronize()
    sameK, sameg = torch.equal(K2, s["K"]), torch.equal(g2, s["g"])
    print(f"second launch: K equal {sameK}, gradient equal {sameg}")
    assert eK < TOL and eg < TOL
    assert torch.equal(s["K"], s["K"].T)
    assert sameK and sameg


@pytest.mark.parametrize("fold", [False, True], ids=["cyclic", "folded"])
def test_two_owners_add_up_to_the_full_launch(gpu, fold):
    from sigsvgd_amd import ops

    N, T, d, stride = 96, 64, 7, 2
    s = _case(N, T, d, gpu)
    nw = ops.sym_tile_rows(T, d)
    ntile = (N + nw - 1) // nw
    owned = [ops.owned_tiles(ntile, r, stride, fold) for r in range(stride)]
    assert sorted(t for o in owned for t in o) == list(range(ntile)) and all(len(o) == ntile // stride for o in owned), owned
    Ks = torch.zeros_like(s["K"])
    gs = torch.zeros(N, T, d, device=gpu, dtype=torch.float64)
    for r in range(stride):
        Kp, gp = ops.gram_sym_partial(s["Xg"], 1.0 / H, r, stride, fold=fold)
        Kq, gq = ops.gram_sym_partial(s["Xg"], 1.0 / H, r, stride, fold=fold)
        torch.cuda.synchronize()
        sameK, sameg = torch.equal(Kp, Kq), torch.equal(gp, gq)
        print(f"owner {r} ({'folded' if fold else 'cyclic'}, tiles {owned[r]}): second launch K equal {sameK}, gradient equal {sameg}")
        assert sameK and sameg
        Ks += Kp
        gs += gp
    eK, eg = rel_entry(Ks.cpu().numpy(), s["Kref"], 1e-6), rel_max(gs.cpu().numpy(), s["gref"])
    es = rel_max(gs.cpu().numpy(), s["g"].double().cpu().numpy())
    print(f"sum of the shares: K {eK:.2e} gradient {eg:.2e} against the oracle, gradient {es:.2e} against the full launch")
    assert torch.equal(Ks, s["K"])
    assert eK < TOL and eg < TOL and es < TOL
