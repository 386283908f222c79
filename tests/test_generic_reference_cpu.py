"""The cases and the checker of the coverage kernel's edge tests, checked on the CPU (tests/generic_reference.py; the device
tests are tests/test_gpu_generic_edges.py).

Every row of the case tables reaches the branch it names on 256 compute units.  `solve` without a table is the oracle.  With a
table it carries the kernel's documented fp32 roundings and passes `assert_generic` at every case, launch and I/O type; each of
five wrong kernels restated on top of it fails that assertion at every case where the mistake can happen.  With an
`assert_generic` that always passes, 29 of the 36 tests here fail: the 28 mistake tests and the test of the pair of tables the
earlier tolerance could not tell apart (tried once).  The batches of tests/test_gpu_repair_flags.py are checked on the oracle
too: the targeted pairs at twice the thresholds of the flag rules, the smooth pairs far below them."""
import numpy as np
import pytest

import generic_reference as G
import matern_reference as MR
import radial_reference as RR
from oracle import sigkernel_oracle as O
from parity import rel_entry, rel_max, signed_weights, walks

IO = ("f32", "f64")


def by_edge(cases, text):
    out = [c for c in cases if text in c.edge]
    assert out, text
    return out


def test_every_case_reaches_the_branch_it_names():
    ids = [G.case_id(c) for c in G.ALL_CASES]
    assert len(set(G.ALL_CASES)) == len(G.ALL_CASES)
    seen = set()
    for c in G.ALL_CASES:
        f = G.assert_claim(c, 256)
        seen |= {(c.route, "fwd", f["table_fwd"]), (c.route, "grad", f["table_grad"])}
        if c.sym:
            assert c.A == c.B
    # every table on both routes and both launches; the fp32 table of a precise launch on a refined grid only
    assert {(r, l, t) for r in ("precise", "default") for l in ("fwd", "grad") for t in ("f64", "f32", "big")} <= seen, seen
    assert all(c.n >= 1 for c in G.ALL_CASES if c.route == "precise" and "f32" in (G.facts(c, 256)["table_fwd"], G.facts(c, 256)["table_grad"]))
    # the loop over the columns of an item, the rounds and the counter: what no earlier case of the kernel had
    f = {G.case_id(c): G.facts(c, 256) for c in G.CHUNK_CASES}
    assert {v["JC"] for v in f.values()} == {1, 2, 8, 32}
    assert f["1024x70-T5-d2-n0-rbf-precise"]["items"] == 3072 and f["1024x70-T5-d2-n0-rbf-precise"]["grid"] == 2048
    assert f["20x20-T128-d14-n0-rbf-precise"]["items"] == 400 and f["20x20-T128-d14-n0-rbf-precise"]["grid"] == 256
    assert f["190x190-yx-T5-d2-n0-rbf-precise"]["nchunks"] == 95 and f["190x190-yx-T5-d2-n0-rbf-precise"]["yx"]
    assert f["5x5-yx-T5-d1-n0-rbf-default"]["yx"] and not f["63x63-yx-T5-d2-n0-rbf-precise"]["yx"]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)


def test_inputs_are_as_described():
    for c in G.ALL_CASES:
        X, Y, w = G.inputs(c)
        assert X.dtype == Y.dtype == w.dtype == np.float32 and X.shape == (c.A, c.T, c.d) and w.shape == (c.A, c.B)
        assert (Y is X) == c.sym and 0.5 <= np.abs(w).min() and np.abs(w).max() <= 1.5 and (w > 0).any() and (w < 0).any()
    assert np.array_equal(G.inputs(G.TABLE_CASES[0])[0], walks(3, 98, 2, 1, 0.3))
    assert np.array_equal(G.inputs(G.TABLE_CASES[0])[2], signed_weights(3, 2, 3).astype(np.float32))


def test_plain_solve_is_the_oracle():
    """`solve` without a table against oracle.sigkernel_oracle (RBF, linear; both stencils; orders 0 and 2) and the radial and
    Matern references, K and gradient, with weights and without"""
    X, Y, w = walks(4, 9, 3, 5, 0.3), walks(3, 9, 3, 6, 0.3), signed_weights(4, 3, 7)
    for kind in (G.RBF, G.LINEAR):
        for (n, naive) in [(0, False), (2, False), (1, True)]:
            for ww in (w, None):
                K, g = G.solve(X, Y, ww, kind, 1.3, n, naive)
                Kr, gr = O.gram_backward(X, Y, ww, kind, 1.3, n, naive)
                assert rel_entry(K, Kr, 0) < 1e-12 and rel_max(g, gr) < 1e-12, (kind, n, naive)
                assert np.array_equal(G.solve(X, Y, ww, kind, 1.3, n, naive, want_grad=False)[0], K)
    for (ref, kind) in [(RR, G.IMQ), (RR, G.RQ), (MR, G.MATERN32), (MR, G.MATERN52)]:
        K, g = G.solve(X, Y, w, kind, 1.3, 1)
        Kr, gr, _ = ref.gram_backward(X, Y, w, kind, 1.3, 1)
        assert rel_entry(K, Kr, 0) < 1e-12 and rel_max(g, gr) < 1e-12, kind
    # two paths of T = 2 by hand: one cell, K = stencil(1, 1, 1, D)
    x, y = np.array([[[0.0], [1.0]]]), np.array([[[0.5], [0.25]]])
    Gm = np.exp(-(x[0] - y[0].T) ** 2 / 2.0)
    D = Gm[1, 1] + Gm[0, 0] - Gm[1, 0] - Gm[0, 1]
    assert abs(G.solve(x, y, None, G.RBF, 2.0, 0)[0][0, 0] - (2 * (1 + D / 2 + D * D / 12) - (1 - D * D / 12))) < 1e-15


def test_restatement_passes_at_every_case():
    """the unmodified restatement against the plain oracle: `assert_generic` passes for every launch of every case on both
    I/O types (E itself is below the 4 E of the tolerance, and below the caps where 4 E passes them), and the rows are not
    hidden: each row's largest gradient entry is at least 2 % of the launch's"""
    worst = {}
    for c in G.ALL_CASES:
        f = G.facts(c, 256)
        rows = G.e_rows(c)
        Kp, gp = G.plain(c, rows=rows)
        assert np.abs(gp).reshape(rows, -1).max(axis=1).min() >= 0.02 * np.abs(gp).max(), G.case_id(c)
        for io in IO:
            if f["table_fwd"]:
                K, _ = G.restated(c, f["table_fwd"], want_grad=False, rows=rows)
                G.assert_generic(c, f["table_fwd"], io, K, Kp, where="forward")
            if f["table_grad"]:
                K, g = G.restated(c, f["table_grad"], rows=rows)
                G.assert_generic(c, f["table_grad"], io, K, Kp, g, gp, where="gradient")
                tol_K, tol_g = G.tolerances(c, f["table_grad"], io)
                assert tol_K <= G.K_CAP and tol_g <= G.G_CAP, (G.case_id(c), tol_K, tol_g)
                worst[f["table_grad"]] = max(worst.get(f["table_grad"], 0), tol_g)
        if c.ones:
            K, g = G.restated(c, f["table_grad"], "ones", rows=rows)
            Ko, go = G.plain(c, "ones", rows)
            G.assert_generic(c, f["table_grad"], "f64", K, Ko, g, go, weights="ones", where="ones")
    print("largest gradient tolerance per table:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert max(worst.values()) <= G.G_CAP  # (a tenth of the earlier file's 1e-5)


def test_the_two_tables_are_told_apart():
    """One shape on both routes, fp64 I/O: the fp32 table's K has E >= 1e-8 and lies above 1e-9 (the device test asserts that
    of the kernel's), ten times what the fp64 table is held to -- and the fp32-table result fails the fp64 table's assertion."""
    a, b = G.HID_F32, G.HID_F64
    assert (a.A, a.B, a.T, a.d, a.n, a.kind, a.naive, a.seed) == (b.A, b.B, b.T, b.d, b.n, b.kind, b.naive, b.seed)
    assert G.facts(a, 256)["table_grad"] == "f32" and G.facts(b, 256)["table_grad"] == "f64"
    E_K, _ = G.restatement_error(a, "f32")
    print(f"E_K of the fp32 table: {E_K:.2e}")
    assert E_K >= 1e-8 and G.restatement_error(b, "f64")[0] == 0.0
    K32, g32 = G.restated(a, "f32")
    Kp, gp = G.plain(b)
    assert rel_entry(K32, Kp, 0) > 1e-9
    with pytest.raises(AssertionError):
        G.assert_generic(b, "f64", "f64", K32, Kp, g32, gp)


# ---- five wrong kernels -------------------------------------------------------------------------------------------------------
def fails(c, mistake, io="f64", table=None, only=None):
    """the mistake restated on top of the case's gradient launch fails `assert_generic`; only: "K" / "gradient" -- the other
    result is the correct one, so the named one fails on its own"""
    f = G.facts(c, 256)
    table = table or f["table_grad"]
    rows = G.e_rows(c)
    Kp, gp = G.plain(c, rows=rows)
    K, g = G.restated(c, table, mistake=mistake, JC=f["JC"], rows=rows)
    K0, g0 = G.restated(c, table, rows=rows)
    G.assert_generic(c, table, io, K0, Kp, g0, gp, where="unmodified")
    with pytest.raises(AssertionError):
        G.assert_generic(c, table, io, K0 if only == "gradient" else K, Kp, g0 if only == "K" else g, gp, where=mistake)


CHUNKED = [c for c in G.CHUNK_CASES if dict(c.claim).get("JC", 1) > 1 and not c.sym]


@pytest.mark.parametrize("c", CHUNKED, ids=G.case_id)
def test_mistake_S_not_rezeroed_per_column(c):
    for io in IO:
        fails(c, "stale_S", io)


@pytest.mark.parametrize("c", [c for c in CHUNKED if c.B % dict(c.claim)["JC"]], ids=G.case_id)
def test_mistake_last_column_of_a_short_chunk_dropped(c):
    for io in IO:
        fails(c, "short_chunk_last_dropped", io, only="K")
        fails(c, "short_chunk_last_dropped", io, only="gradient")


@pytest.mark.parametrize("c", [c for c in G.ALL_CASES if c.n == 7], ids=G.case_id)
def test_mistake_coarse_cell_of_r128_credited_to_one_band(c):
    for io in IO:
        fails(c, "r128_one_band", io)


@pytest.mark.parametrize("c", [c for c in G.ALL_CASES if c.d > 16], ids=G.case_id)
def test_mistake_channel_block_loop_stops_after_its_first_block(c):
    for io in IO:
        fails(c, "first_channel_block_only", io)


@pytest.mark.parametrize("c", [G.HID_F64] + by_edge(G.TABLE_CASES, "f64 last with gradient") + by_edge(G.BAND_CASES, "P = 6"), ids=G.case_id)
def test_mistake_fp32_increments_where_the_fp64_table_is_claimed(c):
    """fp64 I/O: K of the fp64 table is held to 1e-10, which fp32 increments miss (on fp32 I/O the 2e-7 of that table is of the
    size of the increments' rounding: the I/O type that tells the tables apart is fp64)"""
    fails(c, "f32_increments", "f64", only="K")


# ---- the batches of tests/test_gpu_repair_flags.py ------------------------------------------------------------------------------
def assert_flag_batch(fs, X, Y, targeted, smooth):
    """on the oracle: every targeted pair at twice the thresholds of both rules; every smooth pair far below them -- c1 < 75,
    the forward-only figure < 75, grid maximum <= 2 max(|K|, 0.1) (the one-channel ratio, the strictest) -- and |K| > 0.1"""
    K, c1, km, fwd = G.conditioning(X, Y, fs.h, fs.n)
    assert targeted.any() and smooth.any() and not (targeted & smooth).any()
    assert c1[targeted].min() >= G.C1_TARGET and fwd[targeted].min() >= G.FWD_TARGET and np.abs(K[targeted]).min() > 0.1
    assert c1[smooth].max() < G.C1_SMOOTH and fwd[smooth].max() < G.C1_SMOOTH and np.abs(K[smooth]).min() > 0.1
    assert (km <= 2.0 * np.maximum(np.abs(K), 0.1))[smooth].all()
    return c1


@pytest.mark.parametrize("fs", [G.FLAG_FAST, G.FLAG_QUAD], ids=["fast", "quad"])
def test_flag_batches_ordered(fs):
    X, Y, targeted, smooth = G.flag_batch(fs, 10, 130, G.ROWS, G.COLS)
    assert targeted.sum() == 24 and smooth.sum() == 6 * 124 and X.dtype == np.float32
    assert [list(np.flatnonzero(m)) for m in (targeted.any(axis=1), targeted.any(axis=0))] == [list(G.ROWS), list(G.COLS)]
    c1 = assert_flag_batch(fs, X, Y, targeted, smooth)
    assert np.ptp(c1[targeted]) == 0  # (copies of one pair)


def test_flag_batches_refined_and_symmetric():
    """the 256-cell batch on its first 4 x 6 pairs and the Y-is-X batch on 20 of its paths, the targeted ones among them"""
    fs = G.FLAG_BAND
    X, Y, targeted, smooth = G.flag_batch(fs, 10, 130, G.ROWS, G.COLS)
    assert_flag_batch(fs, X[:4], Y[:6], targeted[:4, :6], smooth[:4, :6])
    fs = G.FLAG_FAST
    X, targeted, smooth = G.flag_batch_sym(fs, 130, G.SYM_X, G.SYM_Y)
    assert np.array_equal(targeted, targeted.T) and np.triu(targeted, 1).sum() == np.tril(targeted, -1).sum() == 25
    keep = sorted(set(G.SYM_X) | set(G.SYM_Y) | set(range(20, 30)))
    assert_flag_batch(fs, X[keep], X[keep], targeted[np.ix_(keep, keep)], smooth[np.ix_(keep, keep)])
