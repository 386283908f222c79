"""The long route's partial solve on the device (`ops.gram_long_sym_partial`, csrc/gram_long.hip's partial mode, DESIGN.md
section 5.13) and the sharded SVGD step that runs on it (`distributed.ShardedSigSVGD`).  References and tolerances are the
long route's own (tests/test_gpu_long.py): K within 1e-9 per entry with fp64 I/O and 2^-23 with fp32 I/O, a gradient within
1e-5 of its largest entry, against the C oracle; against the full Y-is-X launch, whose pairs and products the shares
repeat, K bit for bit and the fp64 gradient within 1e-9 (another order of the same fp64 sums)."""
import os

import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle import sigkernel_oracle as O
from parity import np64, rel_entry, rel_max, signed_weights, sized_walks
from plans import device_cus, item_size, part_items, part_plan

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
RBF, LINEAR = 0, 1


def touched_rows(N, R, owned):
    """rows of grad_partial a share adds to: its own tiles' rows (row side) and every row past the first row of one of its
    tiles (column side)"""
    own = {i for t in owned for i in range(t * R, min(N, (t + 1) * R))}
    first = min((t * R for t in owned), default=N)
    return own | set(range(first + 1, N))


# (N, T, d, order, kind, io, stride)
CASES = [
    (20, 300, 3, 0, RBF, F64, 3),
    (33, 200, 4, 2, RBF, F32, 4),
    (9, 257, 5, 0, LINEAR, F64, 2),
    (5, 300, 2, 0, RBF, F64, 8),    # more ranks than tiles
    (70, 140, 20, 0, RBF, F64, 2),  # channels past 16
]
_ORACLE = {}


def _oracle(case, weights, X, W):
    key = (case, weights)
    if key not in _ORACLE:
        N, T, d, n, kind, io, stride = case
        go = {"ones": None, "signed": W, "sym": W + W.T}[weights]
        _ORACLE[key] = c_oracle.gram_fwd_bwd(X, X.copy(), h=0.5, n=n, kind=kind, grad_out=go)
    return _ORACLE[key]


@pytest.mark.parametrize("weights", ["ones", "signed", "sym"])
@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d-T%d-d%d-n%d-k%d-%s-G%d" % (c[0], c[1], c[2], c[3], c[4], "f64" if c[5] == F64 else "f32", c[6]))
def test_shares_add_up(gpu, case, fold, weights):
    from sigsvgd_amd import ops

    N, T, d, n, kind, io, stride = case
    rng = np.random.default_rng(N * 100 + T + n + kind)
    h = 0.5
    X = sized_walks(rng, N, T, d)
    W = signed_weights(N, N, N + T)
    Kr, gr = _oracle(case, weights, X, W)
    Xt = torch.as_tensor(X, dtype=io, device=gpu)
    got = None if weights == "ones" else torch.as_tensor(W, dtype=io, device=gpu)
    sym = weights == "sym"
    assert ops.gram_long_partial_takes(N, T, d, n, kind, stride)
    R, JC = ops.gram_long_partial_tiles(N, T, d, n, kind, stride)
    ntile = -(-N // R)

    Kf, gf, _ = ops.gram_long_fwd_bwd2(Xt, Xt, 1.0 / h, n, kind, got, sym=sym, y_is_x=True)
    K1 = ops.gram_long_fwd(Xt, Xt, 1.0 / h, n, kind)
    Ksum = torch.zeros_like(Kf)
    gsum = torch.zeros((N, T, d), dtype=F64, device=gpu)
    all_owned = []
    for off in range(stride):
        owned = ops.owned_tiles(ntile, off, stride, fold)
        all_owned += owned
        out = (torch.full((N, N), float("nan"), dtype=io, device=gpu), torch.full((N, T, d), float("nan"), dtype=F64, device=gpu))
        Kp, gp = ops.gram_long_sym_partial(Xt, 1.0 / h, off, stride, n, kind, got, sym=sym, out=out, fold=fold)
        assert Kp is out[0] and gp is out[1] and Kp.dtype == io and gp.dtype == F64
        assert bool(torch.isfinite(Kp).all()) and bool(torch.isfinite(gp).all())
        # the share's non-zero rows of the upper triangle are the rows of its tiles, whole
        rows = {i for t in owned for i in range(t * R, min(N, (t + 1) * R))}
        up = np.triu((Kp != 0).cpu().numpy())
        for i in range(N):
            assert up[i, i:].all() if i in rows else not up[i].any(), (off, i)
        assert torch.equal(Kp, Kp.T)
        # rows that received nothing are exact zeros (the buffer held NaN)
        touched = touched_rows(N, R, owned)
        for k in range(N):
            if k not in touched:
                assert not bool(gp[k].any()), (off, k)
        Ksum += Kp
        gsum += gp
    assert sorted(all_owned) == list(range(ntile))
    assert torch.equal(Ksum, Kf)
    assert torch.equal(torch.triu(Ksum), torch.triu(K1))
    assert rel_entry(np64(Ksum), Kr, 0.0) < (1e-9 if io == F64 else 2.0**-23)
    assert rel_max(np64(gsum), gr) < 1e-5
    if io == F64:
        assert rel_max(np64(gsum), np64(gf)) < 1e-9


def _multi_item_case(gpu, N, T, d, stride, several_rounds):
    """a share whose items hold several pairs, first rectangle ragged by the diagonal over several rows, a ragged last one,
    JC not a power of two, in one round of the grid or past it -- asserted from the plan -- against the full Y-is-X launch"""
    from sigsvgd_amd import ops

    R, JC = ops.gram_long_partial_tiles(N, T, d, 0, RBF, stride)
    pl = part_plan(N, T, d, 0, 0, stride, True, device_cus())
    assert (R, JC) == (pl["R"], pl["JC"])
    assert R > 1 and JC > 1 and JC & (JC - 1), (R, JC)
    sizes = [item_size(N, R, JC, pl["owned"][k], c) for (k, c) in part_items(N, R, JC, pl["owned"])]
    assert max(sizes) == R * JC and min(sizes) < R * JC
    assert any((N - t * R) % JC for t in pl["owned"])  # a last rectangle cut by the matrix edge
    if several_rounds:  # waves of the first round take a second item, which starts past the full rectangles
        assert pl["grid"] < pl["items"] < 2 * pl["grid"], (pl["items"], pl["grid"])
    else:
        assert pl["items"] == pl["grid"], (pl["items"], pl["grid"])

    rng = np.random.default_rng(N + T)
    Xt = torch.as_tensor(sized_walks(rng, N, T, d), dtype=F64, device=gpu)
    Kf, gf, _ = ops.gram_long_fwd_bwd2(Xt, Xt, 2.0, y_is_x=True)
    Ksum, gsum = torch.zeros_like(Kf), torch.zeros_like(gf)
    for off in range(stride):
        Kp, gp = ops.gram_long_sym_partial(Xt, 2.0, off, stride, fold=True)
        Ksum += Kp
        gsum += gp
    assert torch.equal(Ksum, Kf)
    assert rel_max(np64(gsum), np64(gf)) < 1e-9


def test_items_of_several_pairs_one_round(gpu):
    """512 paths of 16 points on 2 ranks: 4 x 9 rectangles, one per wave"""
    _multi_item_case(gpu, 512, 16, 2, 2, several_rounds=False)


def test_items_of_several_pairs_past_one_item_per_wave(gpu):
    """4096 paths of 8 points on 2 ranks: 4.2 million pairs a share, more 32 x 35 rectangles than the 8 waves per CU the
    short paths allow, so the persistent loop takes a second item on most waves (short paths keep it cheap)"""
    _multi_item_case(gpu, 4096, 8, 2, 2, several_rounds=True)


def test_reproducible(gpu):
    from sigsvgd_amd import ops

    rng = np.random.default_rng(11)
    Xt = torch.as_tensor(sized_walks(rng, 40, 140, 3), dtype=F32, device=gpu)
    a = ops.gram_long_sym_partial(Xt, 2.0, 1, 2, fold=True)
    junk = torch.full((1 << 22,), float("nan"), device=gpu)  # (other bytes in the allocator's pools in between)
    b = ops.gram_long_sym_partial(Xt, 2.0, 1, 2, fold=True)
    del junk
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_sharded_step_on_the_long_route(gpu):
    """The sharded step under nccl (= RCCL) with one rank.  At T = 300 the fused kernels refuse the launch for LDS (before
    the long partial existed this step raised that RuntimeError) and the step takes the long partial by itself; at order 2,
    T = 100, and at T = 150 it takes it on request (`long_partial=True`).  Each case pins its route; the Gram of a
    long-partial step has the bits of the single-GPU Y-is-X launch."""
    import torch.distributed as dist

    from sigsvgd_amd import ops
    from sigsvgd_amd.distributed import ShardedSigSVGD

    def rel(a, b):
        b = np.asarray(b, np.float64)
        return float(np.abs(np64(a) - b).max() / np.abs(b).max())

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = "29561"
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=gpu)
    try:
        for (N, T, d, n, kw) in [(24, 300, 3, 0, {}), (24, 100, 3, 2, {"dyadic_order": 2, "long_partial": True}),
                                 (24, 150, 3, 0, {"long_partial": True})]:
            X, s = O.synthetic_inputs(N, T, d)
            Xg, sg = X.to(gpu), s.to(gpu)
            sh = ShardedSigSVGD(1.0, 1e-3, **kw)
            Xa = sh.step(Xg, sg)
            assert sh.last_route == "long_partial", (T, n, sh.last_route)
            K, g, _ = ops.gram_long_fwd_bwd2(Xg, Xg, 1.0, n, y_is_x=True)
            _, Xb = ops.svgd_phi(K, sg, g, X=Xg, lr=1e-3)
            assert rel(Xa, np64(Xb)) < 1e-6
            assert torch.equal(sh.gather_gram(), K)
            ref = O.svgd_iteration(X.numpy(), s.numpy(), h=1.0, n=n, lr=1e-3)
            assert rel(Xa, ref["X_new"]) < 1e-5
    finally:
        dist.destroy_process_group()


def test_sharded_step_default_routes_stay_rowwise_where_the_fused_kernels_run(gpu):
    """T = 150 at order 0 and T = 100 at order 2 are launches the fused kernels take: without `long_partial=True` the step
    stays row-wise there, at the step's dyadic order, and agrees with the long route's step within the fused kernels' 1e-5"""
    import torch.distributed as dist

    from sigsvgd_amd.distributed import ShardedSigSVGD

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = "29563"
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=gpu)
    try:
        for (T, kw) in [(150, {}), (100, {"dyadic_order": 2})]:
            X, s = O.synthetic_inputs(8, T, 3)
            Xg, sg = X.to(gpu), s.to(gpu)
            sh = ShardedSigSVGD(1.0, 1e-3, **kw)
            Xa = sh.step(Xg, sg)
            assert sh.last_route == "rowwise"
            Ka = sh.gather_gram()
            lp = ShardedSigSVGD(1.0, 1e-3, long_partial=True, **kw)
            Xl = lp.step(Xg, sg)
            assert lp.last_route == "long_partial"
            assert rel_entry(np64(Ka), np64(lp.gather_gram()), 0.0) < 1e-5
            assert rel_max(np64(Xa), np64(Xl)) < 1e-6
    finally:
        dist.destroy_process_group()
