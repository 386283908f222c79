"""GPU: the fp32-sweep Gram kernels at EVERY path length, their gradient held per point class (tests/sweep_reference.py: the
inputs, the classes, the fp64 oracle, the restated fp32 arithmetic E comes from and the tolerance rule; all of it checked on the
CPU in tests/test_sweep_reference_cpu.py).

One test per length -- gram_fast T = 3 .. 64, gram_quad T = 65 .. 128 -- and per (T, order, band schedule) of the refined grids
(gram_dyad, gram_band on both schedules, wherever plans.gram_geometry sends a launch there); each loops over its channel counts
and launch forms: ordered gradient launch with signed weights, forward-only launch, Y-is-X gradient launch with asymmetric
signed weights (row and column side); fp32 I/O everywhere, fp64 I/O and SIGSVGD_FLAG_SYM at the lengths where an instantiation
changes.  Every launch asserts its family from the launch geometry, the contract (K per entry and rel_max of the gradient
within 1e-5), the class tolerances min(4 E_c + u_out, contract) and the same bits from a second call.  Where two families or
instantiations meet (32|33, 64|65, 112|113, 128|129) the T-point paths and the same paths with their last point repeated give
the same K within 4e-6 per entry."""
import numpy as np
import pytest
import torch

import plans
import sweep_reference as S
from parity import rel_entry

pytestmark = pytest.mark.gpu

IO = {"f32": torch.float32, "f64": torch.float64}
HOOK = "SIGSVGD_SWEEP_WINDOWS"  # tests/test_gpu_fixed_windows.py


def _modes_of(T, n):
    """[(band mode, family)]: both schedules where they lead to different families (a grid of 64 cells is gram_dyad's in both)"""
    out = []
    for mode in ("serial", "parallel"):
        fam = plans.gram_geometry(3, 2, T, 2, n, True, False, 256, mode)["family"]
        if fam not in [f for _, f in out]:
            out.append((mode, fam))
    return out


REFINED = [(T, n, mode, fam) for (T, n) in S.refined_tn() for (mode, fam) in _modes_of(T, n)]
WIDE_REFINED = {"dyad": (5, 5), "band serial": (10, 4), "band parallel": (10, 4)}  # fp64 I/O and FLAG_SYM: one per family


def _launches(gpu, T, d, n, io, wide, family, mode=None, where=""):
    """every launch form of one case; -> the largest error / tolerance of a class"""
    from sigsvgd_amd import ops

    X, Y, w, wyx = S.inputs(T, d)
    Xg, Yg, wg, wyxg = (torch.as_tensor(a, device=gpu).to(IO[io]) for a in (X, Y, w, wyx))
    cus, inv_h = plans.device_cus(), 1.0 / S.H

    def claim(A, B, grad, sym):
        g = plans.gram_geometry(A, B, T, d, n, grad, sym, cus, mode)
        assert g is not None and g["family"] == family, (T, d, n, mode, grad, sym, g)

    def twice(run):
        a, b = run(), run()
        a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
        torch.cuda.synchronize()
        for u, v in zip(a, b):
            assert u.dtype == IO[io] and torch.equal(u, v), (where, T, d, n, "second call")
        return [u.double().cpu().numpy() for u in a]

    worst = 0.0
    claim(3, 2, True, False)
    Kref, gref, _ = S.plain(T, d, n, "ordered")
    K, g = twice(lambda: ops.gram_fwd_bwd(Xg, Yg, inv_h, n, grad_out=wg))
    S.assert_contract(K, Kref, g, gref, (where, T, d, n, "ordered", io))
    worst = max(worst, *S.assert_classes(T, d, n, "ordered", io, g, gref, where, family).values())
    claim(3, 2, False, False)
    (Kf,) = twice(lambda: ops.gram_fwd(Xg, Yg, inv_h, n))
    S.assert_contract(Kf, Kref, where=(where, T, d, n, "forward", io))
    for form in ("yx", "yx-sym") if wide else ("yx",):
        claim(3, 3, True, True)
        Kref, gref, _ = S.plain(T, d, n, form)
        K, g = twice(lambda: ops.gram_fwd_bwd(Xg, Xg, inv_h, n, grad_out=wyxg, sym=form == "yx-sym", y_is_x=True))
        assert np.array_equal(K, K.T)
        S.assert_contract(K, Kref, g, gref, (where, T, d, n, form, io))
        worst = max(worst, *S.assert_classes(T, d, n, form, io, g, gref, where, family).values())
    return worst


def _case(gpu, T, n, ds, wide, family, mode=None, where=""):
    worst = max(_launches(gpu, T, d, n, io, wide, family, mode, where) for d in ds for io in (("f32", "f64") if wide else ("f32",)))
    print(f"T={T} n={n} {family} {where}: largest class error / tolerance {worst:.2f}")


@pytest.mark.parametrize("T", S.FAST_T, ids=[f"T{T}" for T in S.FAST_T])
def test_fast_every_length(gpu, monkeypatch, T):
    """gram_fast: the sweep statements of 8 steps over 2 P - 1 anti-diagonals, the 32-slot ring up to T = 32; d = 3 and 7 are the
    padded 4- and 8-channel forms; T = 64 also with the lane windows read from the table"""
    monkeypatch.delenv(HOOK, raising=False)
    _case(gpu, T, 0, S.fast_ds(T), T in S.WIDE_T, "fast")
    if T == 64:
        monkeypatch.setenv(HOOK, "table")
        _case(gpu, T, 0, S.fast_ds(T), False, "fast", where="windows-table")


QUAD_IDS = [f"T{T}-{'early' if T <= 112 else 'full'}" for T in S.QUAD_T]


@pytest.mark.parametrize("T,variant", [(T, i.split("-")[1]) for T, i in zip(S.QUAD_T, QUAD_IDS)], ids=QUAD_IDS)
def test_quad_every_length(gpu, T, variant):
    """gram_quad: second-half quadrants of T - 65 cells a side, the sweeps cut every 16 steps by the EARLY instantiations
    (T <= 112: `quad_launch_variant`), point row and column 64 done apart; d = 3: the few-channel forward launch, d = 16: the
    row accumulator (no EARLY form).  The instantiation is not observable from Python (no plan query reports it, and a build that sends T = 113 to the
    EARLY kernels returns the unconditional kernels' bits): the id restates the threshold of `quad_launch_variant`
    so that a run names the lengths on either side of it, and the line below only keeps the id and the constant together."""
    assert (T <= 112) == (variant == "early")
    _case(gpu, T, 0, S.QUAD_D, T in S.WIDE_T, "quad")


@pytest.mark.parametrize("T,n,mode,family", REFINED, ids=[f"T{T}-n{n}-{m}-{f.replace(' ', '_')}" for T, n, m, f in REFINED])
def test_refined_every_grid(gpu, monkeypatch, T, n, mode, family):
    """gram_dyad / gram_band: every (T, order) with 64 .. 256 refined cells, on both band schedules where they differ"""
    plans.set_band_mode(monkeypatch, mode)
    _case(gpu, T, n, S.REFINED_D, WIDE_REFINED[family] == (T, n), family, mode)


def test_every_length_and_grid_is_a_case():
    ts = [T for T in S.FAST_T] + [T for T in S.QUAD_T]
    assert ts == list(range(3, 129)) and len(QUAD_IDS) == 64
    assert {(T, n) for T, n, _, _ in REFINED} == set(S.refined_tn()) and {f for *_, f in REFINED} == set(WIDE_REFINED)
    for fam, tn in WIDE_REFINED.items():
        assert any((T, n) == tn and f == fam for T, n, _, f in REFINED), fam


@pytest.mark.parametrize("T", [32, 64, 112, 128])
def test_hand_over_between_families(gpu, monkeypatch, T):
    """32|33 (ring of 32 | 64 slots), 64|65 (gram_fast | gram_quad), 112|113 (EARLY | unconditional), 128|129 (gram_quad | the
    coverage kernel): the last point repeated adds zero increments, which every stencil copies through -- the same K from either
    side, within what two fp32 solves of one pair agree to (the host pads unequal lengths the same way)"""
    from sigsvgd_amd import ops

    monkeypatch.delenv(HOOK, raising=False)
    for d in (3, 7, 14):
        X, Y, w, _ = S.inputs(T, d)
        Xg, Yg, wg = (torch.as_tensor(a, device=gpu, dtype=torch.float32) for a in (X, Y, w))
        Xp, Yp = ops.pad_to_length(Xg, T + 1).contiguous(), ops.pad_to_length(Yg, T + 1).contiguous()
        fams = [plans.gram_geometry(3, 2, t, d, 0, True, False, plans.device_cus()) for t in (T, T + 1)]
        fams = tuple(f and f["family"] for f in fams)
        assert fams == {32: ("fast", "fast"), 64: ("fast", "quad"), 112: ("quad", "quad"), 128: ("quad", None)}[T], fams
        ffwd = tuple((f or {}).get("family") for f in (plans.gram_geometry(3, 2, t, d, 0, False, False, plans.device_cus()) for t in (T, T + 1)))
        assert ffwd == fams, (ffwd, fams)  # (the forward-only launches meet at the same lengths)
        Kref = S.plain(T, d, 0, "ordered")[0]
        for run in (lambda a, b: ops.gram_fwd(a, b, 1.0 / S.H), lambda a, b: ops.gram_fwd_bwd(a, b, 1.0 / S.H, grad_out=wg)[0]):
            K0, K1 = run(Xg, Yg).double().cpu().numpy(), run(Xp, Yp).double().cpu().numpy()
            e = rel_entry(K0, K1, 1e-6)
            print(f"T={T}|{T + 1} d={d}: {e:.2e}")
            S.assert_contract(K0, Kref)
            S.assert_contract(K1, Kref)
            assert e < S.SELF, (T, d, e)
