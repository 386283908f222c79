"""`signature_kernel` (csrc/vec_kernels.hip) and `signature_bwd_kernel` (csrc/sig_backward.hip) on every branch of their
launchers, PER LEVEL against the oracle (`VO.signature`, `VO.signature_vjp`), in fp64 and fp32.

Level k of a signature is smaller than level 1 by about 1/k!, so an error taken over the whole vector checks the top level at
a fraction of the stated tolerance.  Here every level is compared over its own largest magnitude, at the tolerances
tests/test_gpu_vector.py uses for the whole vector: 1e-13 / 1e-6 forwards, 1e-11 / 1e-5 backwards (fp64 / fp32).  The
backward is linear in grad_sig: it runs once per level with grad_sig zero elsewhere, so each level's share of dL/dX is
compared over its own largest magnitude.

One case per branch.  Each case's branch is computed here from the launcher's formulas (`forward_plan`, `backward_plan`,
restated from `signature_launch` and `signature_bwd_launch`) and asserted, so a shape cannot drift off its branch:
  forward   sigdim = C + ... + C^depth; table = 4 depth sigdim bytes; staged (the whole path's increments in LDS) where
            8 (2 sigdim + L C) + table <= 150 KB, else one increment per point (8 (2 sigdim + C) + table); above 64 KB of
            LDS the launcher raises the kernel's limit first; 64 / 128 / 256 threads for sigdim <= 64 / <= 128 / more; one
            element per thread where depth <= 4 and sigdim <= threads, else the general loop
  backward  zeros by memset where L < 2 without basepoint; the one-thread-per-path kernel for eight small (C, depth); else
            lds0 = 8 (6 sigdim + 2 C + C depth (depth + 1) / 2), with the index table (+ 4 depth sigdim) where that still fits
            150 KB; depth 2, 3, 4 unrolled, any other at run time; without the table always at run time"""
import numpy as np
import pytest
import torch

from oracle import vector_oracle as VO
from parity import sized_walks

pytestmark = pytest.mark.gpu

KB150, KB64 = 150 * 1024, 64 * 1024
SMALL_BACKWARD = {(2, 2), (2, 3), (3, 2), (4, 2), (2, 4), (5, 2), (3, 3), (6, 2)}


def threads_for(sigdim):
    return 64 if sigdim <= 64 else 128 if sigdim <= 128 else 256


def forward_plan(L, C, depth):
    sigdim = VO.signature_channels(C, depth)
    table = 4 * depth * sigdim
    lds_min, lds_staged = 8 * (2 * sigdim + C) + table, 8 * (2 * sigdim + L * C) + table
    assert lds_min <= KB150
    staged = lds_staged <= KB150
    threads = threads_for(sigdim)
    lds = lds_staged if staged else lds_min
    return dict(sigdim=sigdim, staged=staged, lds=lds, over_64_kb=lds > KB64, threads=threads,
                one_per_thread=depth <= 4 and sigdim <= threads)


def backward_plan(L, C, depth, basepoint):
    sigdim = VO.signature_channels(C, depth)
    units = C * depth * (depth + 1) // 2
    lds0 = 8 * (6 * sigdim + 2 * C + units)
    assert lds0 <= KB150
    threads = threads_for(sigdim)
    ldst = lds0 + 4 * depth * sigdim
    table = ldst <= KB150 and units <= 4 * threads
    if not basepoint and L < 2:
        form = "memset"
    elif (C, depth) in SMALL_BACKWARD:
        form = "thread per path"
    elif not table:
        form = "no table"
    else:
        form = f"unrolled {depth}" if depth in (2, 3, 4) else "run time"
    return dict(sigdim=sigdim, form=form, lds=ldst if table else lds0, threads=threads)


def levels(C, depth):
    off = 0
    for k in range(1, depth + 1):
        yield k, slice(off, off + C ** k)
        off += C ** k


def paths(N, L, C, seed):
    """[N, L, C] random walks of overall size about 1 (increments scaled by 1 / sqrt(L)), exactly representable in fp32 so
    both I/O types share one reference"""
    return sized_walks(np.random.default_rng(seed), N, L, C).astype(np.float64)


def per_level_error(got, ref, C, depth, where):
    """-> the largest over the levels of max |got - ref| / max |ref|, each level over its own largest magnitude"""
    worst = 0.0
    for k, sl in levels(C, depth):
        top = np.abs(ref[:, sl]).max()
        assert top > 0, (where, k)
        err = float(np.abs(got[:, sl] - ref[:, sl]).max() / top)
        print(f"{where}: level {k} error {err:.3e} of its largest magnitude {top:.3e}")
        worst = max(worst, err)
    return worst


_FORWARD_REF = {}

# id, N, L, C, depth, basepoint, and what `forward_plan` must say
FORWARD = [
    ("per-point increments", 2, 9592, 2, 2, True, dict(staged=False, threads=64, one_per_thread=True)),
    ("staged, one point fewer: the most LDS the kernel takes", 2, 9591, 2, 2, True, dict(staged=True, lds=KB150, threads=64)),
    ("LDS above 64 KB", 2, 6, 14, 3, True, dict(sigdim=2954, staged=True, threads=256, one_per_thread=False)),
    ("128 threads, general form; 126 channels, below the 128 step", 3, 7, 2, 6, False, dict(sigdim=126, threads=128, one_per_thread=False)),
    ("256 threads, one element per thread", 3, 6, 5, 3, True, dict(sigdim=155, threads=256, one_per_thread=True)),
    ("the same, more paths than one workgroup's worth", 70, 5, 5, 3, False, dict(sigdim=155, threads=256, one_per_thread=True)),
    ("62 channels, below the 64 step", 3, 9, 2, 5, True, dict(sigdim=62, threads=64, one_per_thread=False)),
    ("72 channels, above the 64 step", 3, 8, 8, 2, False, dict(sigdim=72, threads=128, one_per_thread=True)),
    ("132 channels, above the 128 step", 2, 5, 11, 2, True, dict(sigdim=132, threads=256, one_per_thread=True)),
    ("depth 1", 3, 6, 3, 1, False, dict(sigdim=3, threads=64, one_per_thread=True)),
]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", FORWARD, ids=[c[0] for c in FORWARD])
def test_forward_branch_per_level(gpu, case, dtype):
    from sigsvgd_amd import ops

    name, N, L, C, depth, bp, want = case
    plan = forward_plan(L, C, depth)
    assert {k: plan[k] for k in want} == want, plan
    assert plan["over_64_kb"] == (name.startswith("LDS above") or L == 9591)  # the launcher raises the kernel's limit there
    if L > 9000:  # the two sides of the staging threshold: 8 (2 sigdim + L C) + table against 150 KB
        assert forward_plan(9591, C, depth)["staged"] and not forward_plan(9592, C, depth)["staged"]
    X = paths(N, L, C, seed=1000 * C + 10 * depth + L % 97)
    key = (N, L, C, depth, bp)
    if key not in _FORWARD_REF:
        _FORWARD_REF[key] = VO.signature(X, depth, bp)
    ref = _FORWARD_REF[key]
    S = ops.signature(torch.as_tensor(X, dtype=dtype, device=gpu), depth, basepoint=bp)
    assert S.dtype == dtype and tuple(S.shape) == (N, plan["sigdim"])
    worst = per_level_error(S.double().cpu().numpy(), ref, C, depth, f"forward, {name}")
    assert worst < (1e-13 if dtype == torch.float64 else 1e-6)


# id, N, L, C, depth, basepoint, and what `backward_plan` must say
BACKWARD = [
    ("no index table", 2, 4, 14, 3, True, dict(form="no table", threads=256)),
    ("table and LDS above 64 KB", 2, 5, 10, 3, False, dict(form="unrolled 3", threads=256)),
    ("unrolled depth 2 outside the small kernel", 3, 6, 8, 2, True, dict(form="unrolled 2", threads=128)),
    ("unrolled depth 4 outside it", 3, 5, 3, 4, False, dict(form="unrolled 4", sigdim=120, threads=128)),
    ("run-time depth 5", 3, 6, 2, 5, True, dict(form="run time", sigdim=62, threads=64)),
    ("run-time depth 6", 2, 5, 2, 6, False, dict(form="run time", sigdim=126, threads=128)),
    ("depth 1", 3, 6, 3, 1, True, dict(form="run time", sigdim=3, threads=64)),
    ("L = 2 with basepoint", 3, 2, 3, 4, True, dict(form="unrolled 4")),
    ("L = 2 without basepoint", 3, 2, 3, 4, False, dict(form="unrolled 4")),
    ("L = 2, thread per path, without basepoint", 67, 2, 3, 3, False, dict(form="thread per path")),
]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", BACKWARD, ids=[c[0] for c in BACKWARD])
def test_backward_branch_per_level(gpu, case, dtype):
    from sigsvgd_amd import ops

    name, N, L, C, depth, bp, want = case
    plan = backward_plan(L, C, depth, bp)
    assert {k: plan[k] for k in want} == want, plan
    if name == "no index table":  # lds0 <= 150 KB < ldst, and the launch raises the kernel's LDS limit
        assert plan["lds"] == 8 * (6 * 2954 + 28 + 84) > KB64 and plan["lds"] + 4 * 3 * 2954 > KB150
    if name.startswith("table and LDS"):
        assert KB64 < plan["lds"] <= KB150
    rng = np.random.default_rng(100 * C + 10 * depth + L)
    X = paths(N, L, C, seed=77 + C + depth)
    W = rng.standard_normal((N, plan["sigdim"])).astype(np.float32).astype(np.float64)
    x = torch.as_tensor(X, dtype=dtype, device=gpu)
    tol = 1e-11 if dtype == torch.float64 else 1e-5
    worst = 0.0
    for k, sl in levels(C, depth):
        Wk = np.zeros_like(W)
        Wk[:, sl] = W[:, sl]
        _, g_ref = VO.signature_vjp(X, Wk, depth, bp)
        wk = torch.as_tensor(Wk, dtype=dtype, device=gpu)
        g = ops.signature_backward(x, wk, depth, bp)
        assert g.dtype == dtype and g.shape == x.shape
        assert torch.equal(g, ops.signature_backward(x, wk, depth, bp)), "not the same bits twice"
        top = np.abs(g_ref).max()
        assert top > 0
        err = float(np.abs(g.double().cpu().numpy() - g_ref).max() / top)
        print(f"backward, {name}: level {k} error {err:.3e} of its largest magnitude {top:.3e}")
        worst = max(worst, err)
    assert worst < tol
    # all levels at once, through autograd, is the sum of the shares to rounding
    xg = x.clone().requires_grad_(True)
    (g_all,) = torch.autograd.grad((ops.signature(xg, depth, basepoint=bp) * torch.as_tensor(W, dtype=dtype, device=gpu)).sum(), xg)
    _, g_ref = VO.signature_vjp(X, W, depth, bp)
    assert float(np.abs(g_all.double().cpu().numpy() - g_ref).max() / np.abs(g_ref).max()) < tol


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("C,depth", [(3, 3), (8, 2), (2, 5)])
def test_backward_of_a_single_point_without_basepoint_is_exactly_zero(gpu, C, depth, dtype):
    """no increment at all: the launcher fills dL/dX with zeros (memset) whatever kernel the signature would take"""
    from sigsvgd_amd import ops

    assert backward_plan(1, C, depth, False)["form"] == "memset" and backward_plan(1, C, depth, True)["form"] != "memset"
    N = 5
    x = torch.as_tensor(paths(N, 1, C, seed=5), dtype=dtype, device=gpu)
    w = torch.randn(N, VO.signature_channels(C, depth), dtype=dtype, device=gpu)
    g = ops.signature_backward(x, w, depth, False)
    assert g.shape == x.shape and g.dtype == dtype and int(torch.count_nonzero(g)) == 0
    assert torch.equal(g.view(torch.int64 if dtype == torch.float64 else torch.int32), torch.zeros_like(g, dtype=torch.int64 if dtype == torch.float64 else torch.int32))
