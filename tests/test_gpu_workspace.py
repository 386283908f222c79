"""Every launch that takes a workspace, on a workspace of exactly the queried size, at the worst alignment, poisoned, between
guards (tests/guarded_workspace.py) -- the three promises of include/sigsvgd_hip.h and INTEGRATION.md about a caller's buffer:

  1. the size a `*_workspace_bytes` query reports is enough;
  2. the pointer may have any alignment (a plan's total carries 256 B of slack, the launcher aligns up);
  3. its contents do not matter (no launch needs a zeroed workspace).

The rest of the GPU suite launches through the buffer `ops._workspace` caches, which is a quarter larger than the largest
query so far, 256-B aligned, and holds the last launch's values: an overrun of a plan, a misaligned base and a read of a word
the launch did not write all pass there.  Here each launch form runs once through unpatched `ops` (the reference run; the
other files hold those outputs to the oracles) and then under the harness with (fill, offset) = (zeros, 0), (zeros, 1),
(0xFF, 1), (random, 1).  After each run both guards must be intact and every output must have the reference run's bits: the
launches are documented as bit-reproducible and independent of the workspace's contents, so any tolerance would hide what
this file looks for.  `test_short_workspace_is_refused` gives one form of each of the ten queries a buffer one byte short.

Shapes come from the tables the other files use (plans.PARTITION_CASES, plans.BRANCH_CASES, the cases of test_gpu_matern,
test_gpu_bandwidth_grad, test_gpu_pair_bands, test_gpu_pde, test_gpu_vector, test_gpu_select, test_gpu_long_partial): the
smallest at which each workspace area is cut raggedly.

Words of a workspace that a kernel reads as an index, count, loop bound or pointer offset, and where this launch writes them
before that read (read off the code; values that are only summed or compared are not listed):

  * gram_generic.hip `next_item` (the 8-byte work counter at the aligned base, symmetric solve): `generic_launch` clears it
    with hipMemsetAsync on the launch's stream in front of the kernel; items past `total_items` end the loop.
  * sqdist_select.hip `SelState` (prefix, rank, count, mode, passes, ncand, total) and the 6 x 4096 histogram bins:
    `select_init_kernel`, the first launch of every call, stores every field and clears every bin.  `ncand` is raised by
    returning atomics and bounds the candidate loop as min(ncand, 2^20); every store to the candidate arrays is guarded by
    `< kCandCap`, and each slot below min(ncand, 2^20) was stored by the lane that claimed it.
  * the [A][B] flag bytes (gram_fast / gram_quad / gram_dyad / gram_band): a branch only.  Every solved pair stores its
    byte unconditionally; the fp64 pass reads the bytes of rows of owned tiles, columns j >= i of a symmetric launch, and a
    set byte selects the column j it belongs to (bounded by the row's own j1 <= B), never an address of its own.
  * everything else (row segments, column slabs and records, row accumulators, increment scratch, stored forward solutions
    and S, per-split partial dK, the long route's slabs) holds floating-point values.  gram_quad's global row accumulator
    (d = 15, 16), the one area that is accumulated into, is zeroed by the kernel for every segment before its atomics.
  * `sigsvgd_vec_kernel_fused` was the one launcher that used the caller's pointer as it came (no aligning, no slack in its
    query): fixed with this file, its blocks now start at the pointer aligned up to 256 B like every other launch's.

Left out: `GraphedSigSVGD` captures a workspace pointer at construction (the harness would have to outlive the graph and
cannot re-poison between replays), and the sharded classes add collectives between ranks; both launch through the same
entry points as the forms here."""
import numpy as np
import pytest
import torch

import plans
from guarded_workspace import GuardedWorkspace
from oracle import sigkernel_oracle as O
from parity import signed_weights, sized_walks, walks

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
RBF, LINEAR, IMQ, RQ, MATERN52 = 0, 1, 2, 3, 7
RUNS = [("zeros", 0), ("zeros", 1), ("ones", 1), ("random", 1)]


def dev(a, gpu, io=None):
    return torch.as_tensor(a, dtype=io, device=gpu)


def synth(A, T, d, seed, gpu, io=F64):
    return O.synthetic_inputs(A, T, d, seed_x=seed)[0].to(device=gpu, dtype=io)


def weights(A, B, gpu, io=F64, seed=11):
    return dev(np.random.default_rng(seed).standard_normal((A, B)), gpu, io)  # signed


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8),
                                                                     b.contiguous().reshape(-1).view(torch.uint8))


def flat(outs):
    """the outputs of a form as one tuple of tensors and Nones"""
    res = []
    for o in outs:
        res.extend(o if isinstance(o, (tuple, list)) else (o,))
    return tuple(res)


# ---- the launch forms: name -> make(gpu, monkeypatch) -> run() -> outputs -----------------------------------------------------
FORMS = {}


def form(name):
    def deco(make):
        assert name not in FORMS
        FORMS[name] = make
        return make
    return deco


def forms_of(table, ident):
    """register `make(case)` for every row of `table`"""
    def deco(make):
        for c in table:
            form(ident(c))(lambda gpu, mp, c=c: make(gpu, mp, c))
        return make
    return deco


# fp32-sweep families: every row of the partition matrix, ordered and Y-is-X, gradient and forward only, signed weights; the
# regimes asserted as tests/test_gpu_partition.py does: (tiles + grid) row segments, the column slab, the band kernels'
# forward-solution scratch, gram_quad's column records, row accumulators (d = 15, 16) and increment scratch are all in play
@forms_of(plans.PARTITION_CASES, lambda c: "partition-" + plans.case_id(c))
def make_partition(gpu, mp, c):
    from sigsvgd_amd import ops

    plans.set_band_mode(mp, c.mode)
    T, d, n, h = c.T, c.d, c.n, 0.9
    cus = plans.device_cus()

    def claim(A, B, grad, sym, own_size):
        g = plans.gram_geometry(A, B, T, d, n, True, sym, cus)
        gf = plans.gram_geometry(A, B, T, d, n, False, sym, cus)
        if grad or own_size or (gf["rows_per_tile"], gf["grid"]) == (g["rows_per_tile"], g["grid"]):
            plans.claim_regime(A, B, T, d, n, grad, sym, c.regime)

    (A, B), N = c.AB, c.N
    (Af, Bf), Nf = c.ABf or c.AB, c.Nf or c.N
    claim(A, B, True, False, True), claim(N, N, True, True, True)
    claim(Af, Bf, False, False, bool(c.ABf)), claim(Nf, Nf, False, True, bool(c.Nf))
    g = plans.gram_geometry(A, B, T, d, n, True, False, cus)
    assert (g["family"], g["rows_per_tile"]) == (c.family, c.rows), g
    s = plans.step_scale(n)
    X, Y, Xs = dev(walks(A, T, d, 11, s), gpu), dev(walks(B, T, d, 12, s), gpu), dev(walks(N, T, d, 21, s), gpu)
    Xf, Yf, Xsf = dev(walks(Af, T, d, 11, s), gpu), dev(walks(Bf, T, d, 12, s), gpu), dev(walks(Nf, T, d, 21, s), gpu)
    go, gos = dev(signed_weights(A, B, 13), gpu, F32), dev(signed_weights(N, N, 23), gpu, F32)

    def run():
        return flat([ops.gram_fwd_bwd(X, Y, 1.0 / h, n, grad_out=go), ops.gram_fwd(Xf, Yf, 1.0 / h, n),
                     ops.gram_fwd_bwd(Xs, Xs, 1.0 / h, n, grad_out=gos, y_is_x=True),
                     ops.gram_fwd(Xsf, Xsf, 1.0 / h, n, y_is_x=True)])
    return run


# the flag array and the fp64 pass behind it: the rough few-channel inputs of
# test_gpu_determinism.py::test_flagged_pairs_and_their_exact_pass_are_reproducible.  The flag bytes are the first area of the
# register-resident kernel's plan (fast_plan), so a zero-filled interior shows, at offset 0, the bytes the kernel stored: the
# case is known to flag when one of them is set.  (The Y-is-X gradient launch of one-channel paths runs on the coverage kernel
# with fp64 sweeps and has no flags: the symmetric solve's work counter instead.)
@forms_of([(40, 64, 1, 0.2, 0.1), (48, 32, 3, 0.1, 0.1)], lambda c: "flagged-N%d-T%d-d%d" % c[:3])
def make_flagged(gpu, mp, c):
    from sigsvgd_amd import ops

    N, T, d, scale, h = c
    rng = np.random.default_rng(N + T)
    X = dev(np.cumsum(scale * rng.standard_normal((N, T, d)), axis=1).astype(np.float32), gpu)
    Y = X.clone()  # the ordered launch: a separate tensor with X's values, as in that test

    def flags_set(launch, nflags):
        with mp.context() as m:
            ws = GuardedWorkspace("zeros", 0).install(m)
            launch()
            torch.cuda.synchronize()
            assert len(ws.requests) == 1
            nset = int(ws.interior(0)[:nflags].count_nonzero())
            ws.check()
        return nset

    nset = flags_set(lambda: ops.gram_fwd(X, Y, 1.0 / h, 0), N * N)
    print(f"forward, ordered {N} x {N}: {nset} pairs flagged for the fp64 pass")
    assert nset > 0
    if d > 1:
        nsym = flags_set(lambda: ops.gram_fwd_bwd(X, X, 1.0 / h, 0, y_is_x=True), N * N)
        print(f"gradient, Y is X: {nsym} pairs flagged")
        assert nsym > 0

    def run():
        return flat([ops.gram_fwd_bwd(X, X, 1.0 / h, 0, y_is_x=True), ops.gram_fwd(X, Y, 1.0 / h, 0)])
    return run


# the coverage kernel's own launches
@form("coverage-symmetric-counter-matern52")
def make_cov_sym(gpu, mp):
    from sigsvgd_amd import ops

    N, T, d = 64, 6, 2  # 4,096 pairs, each unordered pair once: items pulled from the work counter
    X, go = synth(N, T, d, 0, gpu), weights(N, N, gpu)
    return lambda: flat([ops.gram_fwd_bwd(X, X, 1.0, 0, MATERN52, go, y_is_x=True), ops.gram_fwd(X, X, 1.0, 0, MATERN52, y_is_x=True)])


@forms_of([("big-linear", 5, 5, 100, 2, 0, LINEAR, False), ("refined-imq", 5, 6, 10, 3, 2, IMQ, False),
           ("force-generic-rbf", 5, 6, 20, 17, 0, RBF, True)], lambda c: "coverage-" + c[0])
def make_cov(gpu, mp, c):
    from sigsvgd_amd import ops

    _, A, B, T, d, n, kind, force = c  # "big": S of the long-path layout in the launch's scratch
    X, Y, go = synth(A, T, d, 0, gpu), synth(B, T, d, 5, gpu), weights(A, B, gpu)
    return lambda: flat([ops.gram_fwd_bwd(X, Y, 1.0, n, kind, go, force_generic=force),
                         ops.gram_fwd(X, Y, 1.0, n, kind, force_generic=force)])


@form("gram_sym_partial-40x32x3-stride3")
def make_sym_partial(gpu, mp):
    from sigsvgd_amd import ops

    X = O.synthetic_inputs(40, 32, 3)[0].to(gpu)
    go = weights(40, 40, gpu, F32)
    return lambda: flat([ops.gram_sym_partial(X, 1.0, r, 3, grad_out=go) for r in range(3)]
                        + [ops.gram_sym_partial(X, 1.0, 1, 3, fold=True)])


# the long route: gram_long_fwd, gram_long_fwd_bwd (ordered; sym where the batches have one shape) and gram_long_fwd_bwd2 (both
# slots, each alone, Y is X) on the plan's branches, RBF with the default stencil
BRANCH_ROWS = [(2, 2, 129, 129, 2, 0, RBF, False, "full"), (2, 2, 130, 130, 2, 0, RBF, False, "wrap"),
               (2, 2, 66, 66, 2, 0, RBF, False, "L1"), (2, 2, 300, 2, 2, 0, RBF, False, "Q1"), (2, 2, 2, 300, 2, 0, RBF, False, "P1"),
               (2, 3, 60, 100, 3, 2, RBF, False, "short_x"), (2, 2, 300, 300, 17, 0, RBF, False, "channels"),
               (1, 2, 9, 9, 2, 7, RBF, False, "nrow1")]
assert all(c in plans.BRANCH_CASES for c in BRANCH_ROWS)
LONG_ROWS = BRANCH_ROWS + [(67, 70, 5, 6, 2, 0, RBF, False, "tiles"),      # several pairs per tile (test_gpu_bandwidth_grad.py)
                           (3, 4, 70, 66, 3, 0, MATERN52, False, "kind")]  # the Matern instantiations' translation unit


@forms_of(LONG_ROWS, lambda c: "long-" + (plans.branch_id(c) if c[6] < 2 else "%s-%dx%d-T%dx%d-d%d-n%d-k%d" % ((c[8],) + c[:7])))
def make_long(gpu, mp, c):
    from sigsvgd_amd import ops

    A, B, TX, TY, d, n, kind, naive, tag = c
    pl = plans.long2_plan(A, B, TX, TY, d, n, True, True, False, plans.device_cus())
    assert pl is not None
    if tag == "tiles":
        assert pl["IC"] * pl["JC"] > 1 and pl["items"] > pl["grid"], pl
    elif tag != "kind":
        assert plans.branch_regime(tag, pl, TX, TY), pl
    rng = np.random.default_rng(TX * 7 + TY + 100 * d + n)
    X, Y = dev(sized_walks(rng, A, TX, d, d**-0.5), gpu, F64), dev(sized_walks(rng, B, TY, d, d**-0.5), gpu, F64)
    W = weights(A, B, gpu)
    square = A == B and TX == TY

    def run():
        outs = [ops.gram_long_fwd(X, Y, 2.0, n, kind), ops.gram_long_fwd_bwd(X, Y, 2.0, n, kind, W),
                ops.gram_long_fwd_bwd2(X, Y, 2.0, n, kind, W), ops.gram_long_fwd_bwd2(X, Y, 2.0, n, kind, W, want_gradY=False),
                ops.gram_long_fwd_bwd2(X, Y, 2.0, n, kind, W, want_gradX=False)]
        if square:
            outs += [ops.gram_long_fwd_bwd(X, X, 2.0, n, kind, W, sym=True),
                     ops.gram_long_fwd_bwd2(X, X, 2.0, n, kind, W, y_is_x=True)]
        return flat(outs)
    return run


@forms_of([(fold,) for fold in (False, True)], lambda c: "gram_long_sym_partial-12x70x3-world2" + ("-fold" if c[0] else ""))
def make_long_partial(gpu, mp, c):
    from sigsvgd_amd import ops

    N, T, d, n = 12, 70, 3, 0
    X, W = synth(N, T, d, 0, gpu), weights(N, N, gpu)
    return lambda: flat([ops.gram_long_sym_partial(X, 1.0, off, 2, n, RBF, W, fold=c[0]) for off in range(2)])


@form("gram_long_fwd_bwd_h")
def make_long_h(gpu, mp):
    from sigsvgd_amd import ops

    A, B, TX, TY, d, n = 3, 4, 70, 66, 3, 0
    X, Y, W = synth(A, TX, d, 0, gpu), synth(B, TY, d, 5, gpu), weights(A, B, gpu)
    Xs, Ws = synth(5, 34, 2, 0, gpu), weights(5, 5, gpu)
    return lambda: flat([ops.gram_long_fwd_bwd_h(X, Y, 1.0, n, RBF, W),
                         ops.gram_long_fwd_bwd_h(X, Y, 1.0, n, RBF, None, want_gradX=False, want_gradY=False),
                         ops.gram_long_fwd_bwd_h(Xs, Xs, 1.0, 1, RBF, Ws, y_is_x=True)])


@form("pair_fwd_bwd_h")
def make_pair_h(gpu, mp):
    from sigsvgd_amd import ops

    A, TX, TY, d, n = 5, 70, 66, 3, 0
    X, Y, w = synth(A, TX, d, 0, gpu), synth(A, TY, d, 5, gpu), weights(A, A, gpu)[0].contiguous()
    return lambda: flat([ops.pair_fwd_bwd_h(X, Y, 1.0, n, RBF, w),
                         ops.pair_fwd_bwd_h(X, Y, 1.0, n, RBF, None, want_x=False, want_y=False)])


# the paired solver under both schedules (test_gpu_pair_bands.py's cases): the second round and the seam, the per-wave ring,
# a sweep shorter than one phase, channels past 16, the Matern translation unit, the item loop
PAIR_ROWS = [(2, 700, 700, 2, 0, RBF), (2, 260, 260, 3, 2, RBF), (2, 400, 6, 2, 0, RBF), (2, 300, 300, 17, 0, RBF),
             (3, 300, 130, 3, 0, MATERN52), (None, 66, 66, 2, 0, RBF)]


@forms_of([r + (mode,) for r in PAIR_ROWS for mode in ("serial", "bands")],
          lambda c: "pair-%s-A%s-T%dx%d-d%d-n%d-k%d" % ((c[6], "8cus+3" if c[0] is None else c[0]) + c[1:6]))
def make_pair(gpu, mp, c):
    from sigsvgd_amd import ops

    A, TX, TY, d, n, kind, mode = c
    A = 8 * plans.device_cus() + 3 if A is None else A
    mp.setenv("SIGSVGD_PAIR_MODE", mode)
    for want_grad in (False, True):
        waves, grid, _ = ops.pair_schedule(A, TX, TY, d, n, kind, want_grad)
        assert (waves > 1) == (mode == "bands"), f"{waves} waves per pair under SIGSVGD_PAIR_MODE={mode}"
    if c[0] is None:
        assert ops.pair_schedule(A, TX, TY, d, n, kind)[1] < A  # every workgroup takes several pairs
    rng = np.random.default_rng(A * 1000 + TX * 7 + TY + 31 * d + n)
    X, Y = dev(sized_walks(rng, A, TX, d, d**-0.5), gpu, F64), dev(sized_walks(rng, A, TY, d, d**-0.5), gpu, F64)
    w = dev(rng.uniform(-1.5, 1.5, A), gpu)
    return lambda: flat([ops.pair_fwd(X, Y, 2.0, n, kind), ops.pair_fwd_bwd(X, Y, 2.0, n, kind, w),
                         ops.pair_fwd_bwd(X, Y, 2.0, n, kind, w, want_y=False), ops.pair_fwd_bwd(X, Y, 2.0, n, kind, w, want_x=False)])


# sig_pde on a caller's grids: more grids than resident wavefronts (2500 of 10 x 10), and the smallest grid of two bands
@forms_of([("2500x10x10", 50, 10, 10, 0), ("4x66x40", 2, 66, 40, 0)], lambda c: "pde-" + c[0])
def make_pde(gpu, mp, c):
    from sigsvgd_amd import ops

    _, side, M, N, n = c
    pl = plans.pde_plan(side * side, M, N, n, True, plans.device_cus())
    assert pl["grid"] < side * side if side == 50 else pl["P"] > 64, pl
    rng = np.random.default_rng(M * 1000 + N * 10 + n)
    X, Y = np.cumsum(0.15 * rng.standard_normal((side, M, 3)), axis=1), np.cumsum(0.15 * rng.standard_normal((side, N, 3)), axis=1)
    G = dev(O.static_gram(X, Y, O.RBF, 2.0).reshape(side * side, M, N), gpu)
    go = dev(rng.uniform(0.5, 1.5, G.shape[0]), gpu)
    return lambda: flat([ops.pde_fwd(G, n), ops.pde_fwd_bwd(G, n, go)])


# vec_kernel_fused on its reproducible route: per-split partial dK
@forms_of([(130, 130, 129, "gaussian", False), (130, 130, 129, "imq", True), (700, 513, 64, "gaussian", False),
           (700, 513, 64, "imq", False)], lambda c: "vec_fused-%dx%dx%d-%s%s" % (c[:4] + ("-metric" if c[4] else "",)))
def make_vec(gpu, mp, c):
    from sigsvgd_amd import _lib, ops

    A, B, D, kind, metric = c
    rng = np.random.default_rng(A * 1000 + B + D)
    X, Y = dev(rng.normal(size=(A, D)).astype(np.float32), gpu), dev((rng.normal(size=(B, D)) * 0.9 + 0.1).astype(np.float32), gpu)
    go = dev(rng.uniform(0.5, 1.5, size=(A, B)).astype(np.float32), gpu)
    XM = YM = None
    if metric:
        R = rng.normal(size=(D, D))
        M = dev((R @ R.T / D + np.eye(D)).astype(np.float32), gpu)
        XM, YM = X @ M, Y @ M
    k, h2 = (_lib.VEC_GAUSSIAN if kind == "gaussian" else _lib.VEC_IMQ), float(D)
    return lambda: flat([ops.vec_kernel_fused(X, Y, k, 1 / h2, -1 / h2, XM=XM, YM=YM, grad_out=go),
                         ops.vec_kernel_fused(X, Y, k, 1 / h2, -1 / h2, XM=XM, YM=YM, grad_out=go, want_K=False)])


@form("sqdist_select-real-shift100")
def make_select_real(gpu, mp):
    from sigsvgd_amd import ops

    A, B, T, d = 6, 5, 20, 3
    X = dev(O.synthetic_inputs(A, T, d, 0, 1)[0].numpy() + np.float32(100.0), gpu)
    Y = dev(O.synthetic_inputs(B, T, d, 2, 3)[0].numpy() + np.float32(100.0), gpu)
    n = A * B * T * T
    return lambda: flat([ops.path_sqdist_select(X, Y, (n - 1) // 2), ops.path_sqdist_select(X, Y, n // 2),
                         ops.path_sqdist_select(X, None)])


@form("sqdist_select-all-equal")
def make_select_equal(gpu, mp):
    from sigsvgd_amd import ops

    X = torch.full((20, 64, 3), 1.25, dtype=F32, device=gpu)  # more elements than the candidate buffer holds: six passes
    Y = X.clone()
    return lambda: flat([ops.path_sqdist_select(X, Y), ops.path_sqdist_select(X, None, 20 * 20 * 64 * 64 - 1)])


# the public surface
@form("SigKernel.compute_Gram-learnable-sigma")
def make_public_gram(gpu, mp):
    import sigsvgd_amd.sigkernel as sk

    A, B, TX, TY, d, n = 3, 4, 20, 17, 3, 1  # PUB of tests/test_gpu_bandwidth_grad.py
    X0, Y, W = synth(A, TX, d, 0, gpu), synth(B, TY, d, 5, gpu), weights(A, B, gpu)

    def run():
        sigma = torch.tensor(1.3, dtype=F64, device=gpu, requires_grad=True)
        X = X0.clone().requires_grad_(True)
        K = sk.SigKernel(sk.RBFKernel(sigma), n).compute_Gram(X, Y)
        (W * K).sum().backward()
        assert sigma.grad is not None and X.grad is not None
        return K.detach(), X.grad, sigma.grad
    return run


@form("SigKernel.compute_distance-bands")
def make_public_distance(gpu, mp):
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd import ops

    A, T, d = 3, 200, 3
    mp.setenv("SIGSVGD_PAIR_MODE", "bands")
    assert ops.pair_schedule(A, T, T, d, 0, RBF, True)[0] > 1
    rng = np.random.default_rng(4)
    X0, Y0 = dev(sized_walks(rng, A, T, d, d**-0.5), gpu, F64), dev(sized_walks(rng, A, T, d, d**-0.5), gpu, F64)

    def run():
        X, Y = X0.clone().requires_grad_(True), Y0.clone().requires_grad_(True)
        v = sk.SigKernel(sk.RBFKernel(0.8), 0).compute_distance(X, Y)
        v.sum().backward()
        return v.detach(), X.grad, Y.grad
    return run


# forms whose launches include forward-only ones with a query of 0 bytes (the long route and sig_pde keep nothing on the
# forward sweep): those requests must have received NULL, which the harness answers with (None, 0) as `ops._workspace` does
NEEDS_NO_WORKSPACE = ("long-", "pair-", "pde-")


@pytest.mark.parametrize("name", list(FORMS))
def test_launch_form(gpu, monkeypatch, name):
    run = FORMS[name](gpu, monkeypatch)
    ref = run()
    torch.cuda.synchronize()
    assert len(ref) and all(r is None or bool(torch.isfinite(r).all()) for r in ref)
    for fill, offset in RUNS:
        with monkeypatch.context() as m:
            ws = GuardedWorkspace(fill, offset).install(m)
            out = run()
            live = [r["nbytes"] for r in ws.requests]
            ws.check()
        print(f"{name} [{fill}, offset {offset}]: workspace requests {ws.sizes}")
        assert ws.count > 0 and sum(ws.sizes) > 0, "the form never asked for a workspace"
        assert live == [s for s in ws.sizes if s], "a request of 0 bytes must get no buffer"
        if name.startswith(NEEDS_NO_WORKSPACE):
            assert ws.sizes[0] == 0, "the forward-only launch of this route needs no workspace"
        assert len(out) == len(ref)
        for k, (a, b) in enumerate(zip(out, ref)):
            assert (a is None) == (b is None), f"output {k}: None in one run only"
            if b is not None:
                assert bits_equal(a, b), (f"output {k} depends on the workspace ({fill}, offset {offset}): "
                                          f"{int((a != b).sum())} of {b.numel()} entries differ")


# ---- a workspace one byte short is refused before any device work ------------------------------------------------------------
def _short_gram(gpu):
    from sigsvgd_amd import ops

    X, Y = dev(walks(9, 20, 5, 11, 0.05), gpu), dev(walks(7, 20, 5, 12, 0.05), gpu)  # A != B: the query is this launch's plan
    return lambda: ops.gram_fwd_bwd(X, Y, 1.0, 0), None


def _short_long(gpu):
    from sigsvgd_amd import ops

    X, Y = synth(3, 70, 3, 0, gpu), synth(4, 66, 3, 5, gpu)
    return lambda: ops.gram_long_fwd_bwd(X, Y, 1.0, 0), None


def _short_long2(gpu):
    from sigsvgd_amd import ops

    X, Y = synth(3, 70, 3, 0, gpu), synth(4, 66, 3, 5, gpu)
    return lambda: ops.gram_long_fwd_bwd2(X, Y, 1.0, 0), None


def _short_long_h(gpu):
    from sigsvgd_amd import ops

    X, Y = synth(3, 70, 3, 0, gpu), synth(4, 66, 3, 5, gpu)
    return lambda: ops.gram_long_fwd_bwd_h(X, Y, 1.0, 0), None


def _short_pair(gpu):
    from sigsvgd_amd import ops

    X, Y = synth(5, 70, 3, 0, gpu), synth(5, 66, 3, 5, gpu)
    return lambda: ops.pair_fwd_bwd(X, Y, 1.0, 0), None


def _short_pair_h(gpu):
    from sigsvgd_amd import ops

    X, Y = synth(5, 70, 3, 0, gpu), synth(5, 66, 3, 5, gpu)
    return lambda: ops.pair_fwd_bwd_h(X, Y, 1.0, 0), None


def _short_long_partial(gpu):
    from sigsvgd_amd import ops

    X = synth(12, 70, 3, 0, gpu)
    out = (torch.full((12, 12), 7.0, dtype=F64, device=gpu), torch.full((12, 70, 3), 7.0, dtype=F64, device=gpu))
    return lambda: ops.gram_long_sym_partial(X, 1.0, 0, 2, 0, RBF, out=out), out


def _short_pde(gpu):
    from sigsvgd_amd import ops

    rng = np.random.default_rng(3)
    X = np.cumsum(0.15 * rng.standard_normal((2, 66, 2)), axis=1)
    G = dev(O.static_gram(X, X[:, :40], O.RBF, 2.0).reshape(4, 66, 40), gpu)
    return lambda: ops.pde_fwd_bwd(G, 0), None


def _short_vec(gpu):
    from sigsvgd_amd import _lib, ops

    rng = np.random.default_rng(5)
    X, Y = dev(rng.normal(size=(130, 129)).astype(np.float32), gpu), dev(rng.normal(size=(130, 129)).astype(np.float32), gpu)
    return lambda: ops.vec_kernel_fused(X, Y, _lib.VEC_GAUSSIAN, 1 / 129.0, -1 / 129.0), None  # (the short buffer, not NULL)


def _short_select(gpu):
    from sigsvgd_amd import ops

    X = synth(6, 20, 3, 0, gpu, F32)
    return lambda: ops.path_sqdist_select(X), None


SHORT = {"gram": _short_gram, "gram_long": _short_long, "gram_long2": _short_long2, "gram_long_h": _short_long_h,
         "pair": _short_pair, "pair_h": _short_pair_h, "gram_long_partial": _short_long_partial, "pde": _short_pde,
         "vec_fused": _short_vec, "sqdist_select": _short_select}


@pytest.mark.parametrize("query", list(SHORT))
def test_short_workspace_is_refused(gpu, monkeypatch, query):
    """One form of each workspace query on a buffer reported one byte short of the query (the allocation is whole, so a
    launcher that wrongly accepts it harms nothing): the library's workspace error naming the required bytes, intact guards,
    an interior that still holds its fill -- no memset and no kernel ran before the size check -- and untouched outputs.
    `ops.gram_long_sym_partial` itself zeroes a caller's K_partial before it calls the library (the entry point wants it
    zeroed), so that buffer must hold exact zeros, and grad_partial, which only the library writes, its sentinel."""
    launch, out = SHORT[query](gpu)
    ws = GuardedWorkspace("random", 1, short=1).install(monkeypatch)
    with pytest.raises(RuntimeError, match=r"rc=-3\b") as e:
        launch()
    torch.cuda.synchronize()
    assert len(ws.requests) == 1
    need = ws.requests[0]["nbytes"]
    print(f"{query}: {e.value}")
    assert f"{need - 1} B" in str(e.value) and f"required {need} B" in str(e.value)
    assert ws.interior_untouched(), "device work ran before the size check"
    ws.check()
    if out is not None:
        assert not bool(out[0].any()) and bool((out[1] == 7.0).all())


def test_harness_notices_an_overrun_on_the_device(gpu):
    """tests/test_support.py shows on CPU tensors that `check()` can fail; the same on the device buffers the launches get:
    one float stored across the interior's end (in memory the test owns) is reported with its offsets."""
    ws = GuardedWorkspace("ones", 1)
    t, n = ws(gpu, 4096)
    assert t.is_cuda and t.data_ptr() % 256 == 1
    r = ws.requests[0]
    end = r["start"] + n
    r["buf"][end - 2:end + 2] = r["buf"][end - 2:end + 2] ^ 0x55
    with pytest.raises(AssertionError, match=r"request 1 of the test \(nbytes=4096.*back guard changed in 2 bytes, lowest at \+0, highest at \+1 "):
        ws.check()
