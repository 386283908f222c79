"""The coverage kernel (csrc/gram_generic.hip) per entry at its table, band, chunk and round edges, against the C oracle (the
numpy oracle for the kinds the C oracle does not take).

tests/generic_reference.py has the cases, each with the facts of its launch plan it is there for (asserted here with the
device's CU count before anything runs), and the tolerances: K of a launch whose increments are fp64 end to end within 1e-10
on fp64 I/O and 2e-7 on fp32 I/O; K on the fp32 increment table and every gradient within 4 E + u_out, E the error of the
oracle restated with the kernel's documented fp32 roundings (computed on the CPU per case), never above the 1e-5 / 1e-6 the
earlier tests hold them to.  tests/test_generic_reference_cpu.py shows on the CPU that this assertion fails for a stale S, a
dropped last column, a coarse cell credited to one band, fp32 increments under the fp64 table's claim and a channel loop that
stops after its first block.  Every test prints error / tolerance of each launch."""
import numpy as np
import pytest
import torch

import generic_reference as G
from parity import rel_entry
from plans import device_cus

pytestmark = pytest.mark.gpu

DTYPE = {"f32": torch.float32, "f64": torch.float64}


def launch_all(gpu, c, io):
    """every launch of a case: forward only, gradient with the signed weights, gradient with NULL weights where the row asks
    for it -- each asserted against the reference; -> (facts, {launch: K})"""
    from sigsvgd_amd import ops

    f = G.assert_claim(c, device_cus())
    X, Y, w = G.inputs(c)
    Xg = torch.as_tensor(X, device=gpu).to(DTYPE[io])
    Yg = Xg if c.sym else torch.as_tensor(Y, device=gpu).to(DTYPE[io])
    wg = torch.as_tensor(w, device=gpu).to(DTYPE[io])
    kw = dict(naive=c.naive, force_generic=c.route == "precise", y_is_x=c.sym)
    Kref, gref = G.reference(c)
    out = {}
    if f["table_fwd"]:
        out["forward"] = ops.gram_fwd(Xg, Yg, 1.0 / c.h, c.n, c.kind, **kw)
        G.assert_generic(c, f["table_fwd"], io, out["forward"], Kref, where="forward")
    if f["table_grad"]:
        out["gradient"], g = ops.gram_fwd_bwd(Xg, Yg, 1.0 / c.h, c.n, c.kind, grad_out=wg, **kw)
        G.assert_generic(c, f["table_grad"], io, out["gradient"], Kref, g, gref, where="gradient")
        if c.ones:
            out["ones"], g = ops.gram_fwd_bwd(Xg, Yg, 1.0 / c.h, c.n, c.kind, **kw)
            Kone, gone = G.reference(c, "ones")
            G.assert_generic(c, f["table_grad"], io, out["ones"], Kone, g, gone, weights="ones", where="ones")
    if c.sym:
        for name, K in out.items():
            assert torch.equal(K, K.T), (G.case_id(c), name)
    return f, out


@pytest.mark.parametrize("io", ["f32", "f64"])
@pytest.mark.parametrize("c", G.TABLE_CASES, ids=G.case_id)
def test_increment_tables(gpu, c, io):
    """one shape on each side of every switch between the fp64 table, the fp32 table, the per-band layout and the refusal, on
    the precise and the default route; the per-band layout with the IMQ and Matern instantiations"""
    f, _ = launch_all(gpu, c, io)
    if c.want == "fwd":  # the gradient launch of the shape is refused, and says so
        from sigsvgd_amd import ops

        X = torch.zeros((c.A, c.T, c.d), device=gpu, dtype=DTYPE[io])
        with pytest.raises(RuntimeError, match="LDS"):
            ops.gram_fwd_bwd(X, X[:c.B], 1.0 / c.h, c.n, c.kind, naive=c.naive, force_generic=True)


@pytest.mark.parametrize("io", ["f32", "f64"])
@pytest.mark.parametrize("c", G.SHORT_CASES + G.BAND_CASES, ids=G.case_id)
def test_grid_and_bands(gpu, c, io):
    """T = 2 (1, 8 and 128 cells); a last band of 63, 64 and one row at order 0; P = 64 through r = 2, 4, 32; a coarse row per
    band (r = 64) and a coarse cell across two bands (r = 128)"""
    launch_all(gpu, c, io)


@pytest.mark.parametrize("io", ["f32", "f64"])
@pytest.mark.parametrize("c", G.PARTS_CASES + G.CHANNEL_CASES, ids=G.case_id)
def test_gradient_assembly(gpu, c, io):
    """phase 4: 16, 8, 4 and 2 lanes to a point row, one and two passes of a row per lane; one, two and three blocks of 16
    channels, with and without the padding column"""
    launch_all(gpu, c, io)


@pytest.mark.parametrize("io", ["f32", "f64"])
@pytest.mark.parametrize("c", G.CHUNK_CASES, ids=G.case_id)
def test_chunks_rounds_and_the_counter(gpu, c, io):
    """several columns per item (the LDS accumulator carried across them, S re-zeroed per column, a short last chunk), more
    items than workgroups on the static round loop, and Y is X: ordered below 4096 pairs, unordered from there on with chunks
    left of the diagonal and the work counter, and on the one-channel route at any size -- K mirrored bit for bit"""
    launch_all(gpu, c, io)


def test_the_two_tables_are_told_apart(gpu):
    """fp64 I/O, one shape: K on the fp64 table (precise route) is within 1e-10 of the oracle, K on the fp32 table (default
    route) is not held to that -- and is not that good: it lies above 1e-9"""
    _, k64 = launch_all(gpu, G.HID_F64, "f64")
    _, k32 = launch_all(gpu, G.HID_F32, "f64")
    Kref, _ = G.reference(G.HID_F32)
    for name in ("forward", "gradient"):
        e64, e32 = rel_entry(k64[name], Kref, 0, min_ref=G.MIN_K), rel_entry(k32[name], Kref, 0, min_ref=G.MIN_K)
        print(f"{name}: fp64 table {e64:.2e}, fp32 table {e32:.2e}")
        assert e64 < 1e-10 and e32 > 1e-9
    assert np.isfinite(Kref).all()
