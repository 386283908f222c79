"""The sharded SVGD step on the long route, without a GPU: gloo at world size 2 and 4 with an oracle-backed double of
`ops.gram_long_sym_partial` (the ownership taken from the library's own plan query, `ops.gram_long_partial_tiles`), at a
dyadic order and static kernel of the caller's, against the single-process oracle iteration; and which of its routes
`ShardedSigSVGD.step` takes for a shape.  On the GPU box the same class runs with the HIP partial solve
(tests/test_gpu_long_partial.py)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def long_sym_partial(X, inv_h, tile_offset, tile_stride, dyadic_order=0, static_kind=0, grad_out=None, naive=False,
                     sym=False, out=None, fold=False):
    """`helpers.gram_sym_partial` on the long route's ownership: unordered pairs {i <= j} whose row tile of i --
    `ops.gram_long_partial_tiles(...)[0]` rows -- is one of `ops.owned_tiles(...)`, at the caller's order and kernel."""
    from oracle import sigkernel_oracle as O
    from sigsvgd_amd import ops

    Xn = X.detach().cpu().numpy().astype(np.float64)
    N, T, d = Xn.shape
    R, _ = ops.gram_long_partial_tiles(N, T, d, dyadic_order, static_kind, tile_stride)
    owned = set(ops.owned_tiles((N + R - 1) // R, tile_offset, tile_stride, fold))
    Kp, gp = np.zeros((N, N)), np.zeros((N, T, d))
    for i in range(N):
        if (i // R) not in owned:
            continue
        for j in range(i, N):
            Kij, gi = O.gram_backward(Xn[i:i + 1], Xn[j:j + 1], None, static_kind, 1.0 / inv_h, dyadic_order, naive)
            Kp[i, j] = Kp[j, i] = Kij[0, 0]
            gp[i] += gi[0]
            if j != i:
                gp[j] += O.gram_backward(Xn[j:j + 1], Xn[i:i + 1], None, static_kind, 1.0 / inv_h, dyadic_order, naive)[1][0]
    Kt, gt = torch.as_tensor(Kp, dtype=X.dtype), torch.as_tensor(gp, dtype=torch.float64)
    if out is not None:
        out[0].copy_(Kt)
        out[1].copy_(gt)
        return out
    return Kt, gt


def _worker(rank, world, port, N, T, d, steps, order, kind, fold, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import helpers
        from oracle import sigkernel_oracle as O
        from sigsvgd_amd.distributed import ShardedSigSVGD, shard_rows

        X, score = O.synthetic_inputs(N, T, d)
        r0, r1 = shard_rows(N, rank, world)
        Xs, ss = X[r0:r1].clone(), score[r0:r1].clone()
        sh = ShardedSigSVGD(1.0, 0.05, phi_fn=lambda K, s, gk: helpers.svgd_phi(K, s, gk), fold=fold, dyadic_order=order,
                            static_kind=kind, long_partial=True, long_partial_fn=long_sym_partial)
        for _ in range(steps):
            Xs = sh.step(Xs, ss)
            assert sh.last_route == "long_partial"
        K = sh.gather_gram()
        q.put((rank, Xs.numpy(), K.numpy() if rank == 0 else None))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,N,order,kind,fold", [(2, 16, 0, 0, True), (4, 16, 1, 0, True), (2, 12, 0, 1, False),
                                                      (4, 12, 0, 0, False)])
def test_sharded_long_iteration_matches_single_process(world, N, order, kind, fold):
    from oracle import sigkernel_oracle as O

    T, d, steps = 6, 2, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 30600 + (os.getpid() % 1000) + world + 17 * order + 29 * kind + (13 if not fold else 0)
    procs = [ctx.Process(target=_worker, args=(r, world, port, N, T, d, steps, order, kind, fold, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = []
    for _ in range(world):  # (a rank that raised never puts: fail as soon as one has exited non-zero)
        for _ in range(300):
            try:
                outs.append(q.get(timeout=1))
                break
            except Exception:
                assert all(p.exitcode in (None, 0) for p in procs), [p.exitcode for p in procs]
        else:
            raise AssertionError("timeout waiting for the ranks")
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    outs.sort(key=lambda t: t[0])
    X_sharded = np.concatenate([o[1] for o in outs], axis=0)
    K_last = outs[0][2]

    X, score = O.synthetic_inputs(N, T, d)
    Xr = X.numpy().astype(np.float64)
    Kprev = None
    for _ in range(steps):
        Kprev = O.gram(Xr.astype(np.float32), Xr.astype(np.float32), kind, 1.0, order)
        Xr = O.svgd_iteration(Xr.astype(np.float32), score.numpy(), h=1.0, n=order, lr=0.05, kind=kind)["X_new"]
    assert np.abs(X_sharded - Xr).max() / np.abs(Xr).max() < 5e-6
    assert np.abs(K_last - Kprev).max() / np.abs(Kprev).max() < 5e-6  # Gram of the last step's input


def test_long_partials_sum_to_full():
    from oracle import sigkernel_oracle as O

    X, _ = O.synthetic_inputs(11, 5, 3)
    for (order, kind) in [(0, 0), (1, 1)]:
        Kf, gf = O.gram_backward(X.numpy(), X.numpy(), None, kind, 1.0, order)
        for fold in (False, True):
            for stride in (1, 2, 3):
                parts = [long_sym_partial(X, 1.0, off, stride, order, kind, fold=fold) for off in range(stride)]
                assert np.allclose(sum(p[0].numpy().astype(np.float64) for p in parts), Kf, rtol=1e-6)
                assert np.allclose(sum(p[1].numpy() for p in parts), gf, rtol=1e-9, atol=1e-12)


# ---- routing -----------------------------------------------------------------------------------------------------------
@pytest.fixture
def gloo_single():
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(31700 + os.getpid() % 1000)
    dist.init_process_group("gloo", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


def _doubles(monkeypatch, calls):
    """shape-only doubles of the four ops a step can reach (zeros: the routes are the subject, not the numbers)"""
    from sigsvgd_amd import ops

    def partial(X, inv_h, off, stride, static_kind=0, grad_out=None, sym=False, out=None, fold=False):
        calls.append(("partial", {}))
        N, T, d = X.shape
        return torch.zeros(N, N), torch.zeros(N, T, d, dtype=torch.float64)

    def long_partial(X, inv_h, off, stride, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False, out=None,
                     fold=False):
        calls.append(("long_partial", dict(order=dyadic_order, kind=static_kind, fold=fold, out=out is not None)))
        N, T, d = X.shape
        return torch.zeros(N, N), torch.zeros(N, T, d, dtype=torch.float64)

    def rows(Xs, Xf, inv_h, dyadic_order=0, static_kind=0, **kw):
        calls.append(("rowwise", dict(order=dyadic_order, kind=static_kind)))
        return torch.zeros(Xs.shape[0], Xf.shape[0]), torch.zeros_like(Xs)

    def phi(K, s, gk, **kw):
        return torch.zeros_like(s)

    for name, fn in [("gram_sym_partial", partial), ("gram_long_sym_partial", long_partial), ("gram_fwd_bwd", rows),
                     ("svgd_phi", phi)]:
        monkeypatch.setattr(ops, name, fn)


ROUTES = {  # (T, order) -> route for long_partial None / True / False (the real library's host-only queries decide)
    (64, 0): ("partial", "long_partial", "partial"),
    (150, 0): ("rowwise", "long_partial", "rowwise"),
    (300, 0): ("long_partial", "long_partial", "rowwise"),
    (20, 2): ("rowwise", "long_partial", "rowwise"),
}


@pytest.mark.parametrize("T,order", list(ROUTES))
def test_step_routes(monkeypatch, gloo_single, T, order):
    from sigsvgd_amd.distributed import ShardedSigSVGD

    X, s = torch.zeros(4, T, 2), torch.zeros(4, T, 2)
    for setting, want in zip((None, True, False), ROUTES[(T, order)]):
        calls = []
        _doubles(monkeypatch, calls)
        sh = ShardedSigSVGD(1.0, 0.1, dyadic_order=order, long_partial=setting)
        out = sh.step(X, s)
        assert out.shape == X.shape
        assert [c[0] for c in calls] == [want] and sh.last_route == want, (T, order, setting, calls)
        if want != "partial":
            assert calls[0][1]["order"] == order and calls[0][1]["kind"] == 0
        if want == "long_partial":
            assert calls[0][1]["fold"] is True and calls[0][1]["out"] is True
            assert sh.last_K_partial is not None and sh.gather_gram().shape == (4, 4)
    calls = []
    _doubles(monkeypatch, calls)
    ShardedSigSVGD(1.0, 0.1, dyadic_order=order, long_partial=True, rowwise=True).step(X, s)  # rowwise=True comes first
    assert [c[0] for c in calls] == ["rowwise"]


def test_a_callers_rows_fn_keeps_its_launches(monkeypatch, gloo_single):
    """With a row solver of the caller's own (the CPU doubles, a rehearsal) the step does not move to the long partial by
    itself at a shape the fused kernels refuse: it calls rows_fn, as before.  long_partial=True or a long_partial_fn of the
    caller's asks for it."""
    from sigsvgd_amd.distributed import ShardedSigSVGD

    X, s = torch.zeros(4, 300, 2), torch.zeros(4, 300, 2)
    mine = []

    def my_rows(Xs, Xf, inv_h):
        mine.append("rows")
        return torch.zeros(Xs.shape[0], Xf.shape[0]), torch.zeros_like(Xs)

    def my_long(Xf, inv_h, off, stride, dyadic_order=0, static_kind=0, out=None, fold=False):
        mine.append("long")
        return torch.zeros(4, 4), torch.zeros(4, 300, 2, dtype=torch.float64)

    for kw, want, called in [({}, "rowwise", ["rows"]), ({"long_partial": False}, "rowwise", ["rows"]),
                             ({"long_partial": True}, "long_partial", []), ({"long_partial_fn": my_long}, "long_partial", ["long"])]:
        calls = []
        _doubles(monkeypatch, calls)
        del mine[:]
        sh = ShardedSigSVGD(1.0, 0.1, rows_fn=my_rows, **kw)
        sh.step(X, s)
        assert sh.last_route == want and mine == called, (kw, sh.last_route, mine)
        assert [c[0] for c in calls] == (["long_partial"] if kw == {"long_partial": True} else [])


def test_linear_kernel_leaves_the_fused_partial(monkeypatch, gloo_single):
    """the fused partial solve is RBF at order 0 only: the linear kernel at T = 64 goes row-wise, and to the long partial
    when asked"""
    from sigsvgd_amd import _lib
    from sigsvgd_amd.distributed import ShardedSigSVGD

    X, s = torch.zeros(4, 64, 2), torch.zeros(4, 64, 2)
    for setting, want in ((None, "rowwise"), (True, "long_partial")):
        calls = []
        _doubles(monkeypatch, calls)
        ShardedSigSVGD(1.0, 0.1, static_kind=_lib.STATIC_LINEAR, long_partial=setting).step(X, s)
        assert [c[0] for c in calls] == [want] and calls[0][1]["kind"] == _lib.STATIC_LINEAR


def test_four_argument_partial_fn_still_works(monkeypatch, gloo_single):
    from sigsvgd_amd.distributed import ShardedSigSVGD

    calls = []
    _doubles(monkeypatch, calls)
    seen = []

    def four(X, inv_h, off, stride):
        seen.append((off, stride))
        return torch.zeros(4, 4), torch.zeros(4, 64, 2, dtype=torch.float64)

    sh = ShardedSigSVGD(1.0, 0.1, partial_fn=four)
    sh.step(torch.zeros(4, 64, 2), torch.zeros(4, 64, 2))
    assert seen == [(0, 1)] and calls == [] and sh.last_route == "partial" and sh.fold is False
    # ... and the long route of the same object keeps the folded ownership it was built with
    sh.step(torch.zeros(4, 300, 2), torch.zeros(4, 300, 2))
    assert [c[0] for c in calls] == ["long_partial"] and calls[0][1]["fold"] is True
