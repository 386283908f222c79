"""The cases and the checker of the coverage kernel's edge tests (csrc/gram_generic.hip; the device tests are
tests/test_gpu_generic_edges.py, the checker is itself checked in tests/test_generic_reference_cpu.py).

Cases.  Every row names what it is there for as a `claim`: facts of its launch plan (`facts`, read off `plans.generic_plan`
with the device's CU count) that the tests assert before anything runs -- the increment table of the forward-only and of the
gradient launch, the refined grid, the bands, the chunking, the rounds.

Reference and tolerances.  `solve(..., table=None)` is the fp64 numpy oracle (oracle/sigkernel_oracle.py, the radial kinds of
tests/radial_reference.py and tests/matern_reference.py) evaluated on paths centred on x_i's first point.  With `table` it
carries the kernel's documented fp32 roundings and nothing else:
    "f32"            the increments D are stored in fp32;
    every table      the forward solution K_fwd is parked in fp32 before GG = K_fwd * K_rev is formed;
    "big"            S = GG (dyadic order 0) is stored in fp32.
E is the restatement's error against the plain oracle on the case's own inputs; the tolerance of a device result is
    K, table "f64" / "big":   1e-10 on fp64 I/O, 2e-7 on fp32 I/O (tests/test_gpu_generic.py, test_gpu_precision.py);
    K, table "f32":           min(4 E_K + u_out, 1e-5);
    every gradient:           min(4 E_g + u_out, 1e-6),
u_out = 2^-24 for fp32 output and, for fp64, the 1e-10 two fp64 evaluations are held to (E is exactly 0 where K_fwd holds
nothing but the boundary value 1: T = 2 at order 0).  E of a launch whose refined grids hold more than 2^20 cells is taken on
its first rows, that many cells of the same walks (a row's gradient error depends on that row's pairs only).  The margin of 4: the kernel's fp64 increments differ from numpy's in their last
bits, so a different but equally distributed set of them rounds the other way.  E never comes from a device result."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import matern_reference as MR
import radial_reference as RR
from oracle import sigkernel_oracle as O
from parity import rel_entry, rel_max, signed_weights, walks
from plans import generic_plan, generic_route

RBF, LINEAR, IMQ, RQ, MATERN32, MATERN52 = 0, 1, 2, 3, 6, 7
U32 = 2.0 ** -24
K_EXACT = {"f64": 1e-10, "f32": 2e-7}  # I/O type -> K per entry where the increments are fp64 end to end
K_CAP, G_CAP = 1e-5, 1e-6            # what the earlier tests held K and the gradient to: nothing may loosen
MARGIN = 4.0
MIN_K = 0.05                          # below the smallest |K_ref| of any case (asserted: rel_entry(.., 0, min_ref=MIN_K))
FP64_FLOOR = 1e-10                    # what two fp64 evaluations agree to (K_EXACT["f64"]): the tolerance where E is 0, as
                                      # for T = 2 at order 0, whose K_fwd is the boundary value 1 and rounds to itself
E_CELLS = 1 << 20                     # E of a larger launch is taken on its first rows: about this many PDE cells

# edge: what the row is for; route: "precise" (force_generic) / "default"; sym: Y is X (A == B); want: "both" launches or
# "fwd" only (the gradient launch is refused: asserted); ones: also the NULL-weights launch; claim: (fact, value) pairs asserted
Case = namedtuple("Case", "edge A B T d n kind naive route sym want ones claim scale h seed",
                  defaults=(0, False, "precise", False, "both", False, None, 0.3, 1.7, 1))


def _t(edge, T, d, n, fwd, grad, route="precise", kind=RBF, naive=False, ones=False, **claim):
    """a table-mode row: ordered 3 x 2, the increment tables of its forward-only and gradient launches (None: refused)"""
    return Case(edge, 3, 2, T, d, n, kind, naive, route, False, "both" if grad else "fwd", ones,
                tuple(sorted(dict(table_fwd=fwd, table_grad=grad, **claim).items())))


TABLE_CASES = [
    # precise route (force_generic), d = 2, order 0: fp64 table to T = 98 with the gradient, 138 without; then per band
    _t("f64 last with gradient", 98, 2, 0, "f64", "f64", ones=True),
    _t("big first with gradient", 99, 2, 0, "f64", "big", ones=True),
    _t("f64 last forward", 138, 2, 0, "f64", "big"),
    _t("big first forward", 139, 2, 0, "big", "big"),
    _t("big last", 276, 2, 0, "big", "big", last_accepted=True),
    # ... order 1: past the fp64 table the launch keeps fp32 increments (no per-band layout on refined grids)
    _t("f64 last with gradient, order 1", 98, 2, 1, "f64", "f64"),
    _t("f32 in a precise launch, first", 99, 2, 1, "f64", "f32", ones=True),
    _t("f32 in a precise launch", 105, 2, 1, "f64", "f32"),
    _t("f32 in a precise launch, last", 113, 2, 1, "f64", "f32", last_accepted_grad=True),
    _t("f64 last forward, order 1", 138, 2, 1, "f64", None),
    _t("f32 first forward, order 1", 139, 2, 1, "f32", None),
    _t("f32 last forward, order 1", 192, 2, 1, "f32", None, last_accepted=True),
    # ... d = 16
    _t("f64 last, 16 channels", 89, 16, 0, "f64", "f64"),
    _t("big first, 16 channels", 90, 16, 0, "f64", "big"),
    _t("big last, 16 channels", 200, 16, 0, "big", "big", last_accepted=True),
    # default route: fp64 table up to 20 KB, fp32 table up to 160 KB, then per band.  Linear kind while the linear
    # signature kernel stays small (T <= 47), the naive flag beyond
    _t("default f64 last with gradient", 33, 2, 0, "f64", "f64", "default", LINEAR, ones=True),
    _t("default f32 first with gradient", 34, 2, 0, "f64", "f32", "default", LINEAR, ones=True),
    _t("default f64 last forward", 46, 2, 0, "f64", "f32", "default", LINEAR),
    _t("default f32 first forward", 47, 2, 0, "f32", "f32", "default", LINEAR),
    _t("f64 where the default route has f32", 47, 2, 0, "f64", "f64", "precise", LINEAR),
    _t("default f32 first with gradient, naive", 34, 2, 0, "f64", "f32", "default", RBF, True),
    _t("default f32 last with gradient", 113, 2, 0, "f32", "f32", "default", RBF, True),
    _t("default big first with gradient", 114, 2, 0, "f32", "big", "default", RBF, True, ones=True),
    _t("default f32 last forward", 194, 2, 0, "f32", "big", "default", RBF, True),
    _t("default big first forward", 195, 2, 0, "big", "big", "default", RBF, True),
    # the per-band layout with the other instantiations of the kernel (NEWKIND 1 and 2), through the Gram entry point
    _t("big, IMQ", 120, 2, 0, "f64", "big", "default", IMQ),
    _t("big, Matern-5/2", 150, 3, 0, "big", "big", "default", MATERN52),
]

SHORT_CASES = [_t(f"T = 2, {1 << n} cells", 2, d, n, "f64", "f64", P=1 << n, r=1 << n, ones=(n == 3 and d == 2))
               for n in (0, 3, 7) for d in (1, 2)]

BAND_CASES = [
    # order 0: the last band full, of one row, of 63 rows
    *[_t(f"P = {T - 1}", T, 2, 0, "f64", "f64" if T < 99 else "big", P=T - 1, nbands=-(-(T - 1) // 64),
         last_band=(T - 2) % 64 + 1) for T in (64, 65, 66, 128, 129, 130)],
    # through refinement: a coarse row is r lanes of a band, a band, two bands
    _t("P = 64, r = 2", 33, 2, 1, "f64", "f64", P=64, r=2),
    _t("P = 64, r = 4", 17, 2, 2, "f64", "f64", P=64, r=4),
    _t("P = 64, r = 32", 3, 2, 5, "f64", "f64", P=64, r=32),
    _t("r = 64: one coarse row per band", 3, 2, 6, "f64", "f64", P=128, r=64, nbands=2),
    _t("r = 128: a coarse cell across two bands", 3, 2, 7, "f64", "f64", P=256, r=128, nbands=4),
    _t("P = 256, r = 64", 5, 2, 6, "f64", "f64", P=256, r=64, nbands=4),
]

# phase 4: `parts` lanes share a point row (16, 8, 4, 2 up to T = 4, 8, 16, 32), then one row per lane in `passes` passes
PARTS_CASES = [_t(f"parts = {parts}, T = {T}", T, 3, 0, "f64", "f64", parts=parts, passes=passes)
               for (T, parts, passes) in [(4, 16, 1), (5, 8, 1), (8, 8, 1), (9, 4, 1), (16, 4, 1), (17, 2, 1), (32, 2, 1),
                                          (33, 1, 1), (64, 1, 1), (65, 1, 2)]]

# the 16-channel blocks of phase 4 (1, 1, 1, 2, 2, 3); d = 1: no padding column, d = 2, 16, 32: dp = d + 1
CHANNEL_CASES = [_t(f"d = {d}", 9, d, 1, "f64", "f64", cblocks=-(-d // 16), dp=d + 1 if d % 2 == 0 else d)._replace(h=1.7 * max(1, d / 3))
                 for d in (1, 2, 16, 17, 32, 33)]


def _c(edge, A, B, T, d, n, sym=False, route="precise", **claim):
    return Case(edge, A, B, T, d, n, RBF, False, route, sym, "both", False, tuple(sorted(claim.items())))


CHUNK_CASES = [
    *[c for n in (0, 2) for c in (
        _c("JC = 2, last chunk of one", 64, 65, 5, 2, n, JC=2, last_chunk=1, yx=False),
        _c("JC = 8", 256, 70, 5, 2, n, JC=8, last_chunk=6, yx=False),
        _c("JC = 32, last chunk of 6, items past the grid", 1024, 70, 5, 2, n, JC=32, last_chunk=6, rounds=True, yx=False),
        _c("Y is X, ordered below 4096 pairs", 63, 63, 5, 2, n, True, JC=1, yx=False),
        _c("Y is X, unordered from 4096 pairs", 64, 64, 5, 2, n, True, JC=1, yx=True, rounds=True),
        _c("Y is X, JC = 2: chunks left of the diagonal", 190, 190, 5, 2, n, True, JC=2, yx=True, rounds=True))],
    _c("several rounds at one workgroup per CU", 20, 20, 128, 14, 0, JC=1, rounds=True, per_cu=1, table_grad="big")._replace(h=8.0),
    _c("one-channel route, unordered at any size", 5, 5, 5, 1, 0, True, "default", route_name="GenericOneChannel", yx=True),
]

# The pair the earlier 1e-5 could not tell apart: one shape on the fp32 table (default route) and on the fp64 table (precise)
HID_F32, HID_F64 = (next(c for c in TABLE_CASES if c.T == 47 and c.route == r) for r in ("default", "precise"))

ALL_CASES = TABLE_CASES + SHORT_CASES + BAND_CASES + PARTS_CASES + CHANNEL_CASES + CHUNK_CASES


def case_id(c):
    kind = {RBF: "rbf", LINEAR: "lin", IMQ: "imq", RQ: "rq", MATERN32: "m32", MATERN52: "m52"}[c.kind]
    return (f"{c.A}x{c.B}{'-yx' if c.sym else ''}-T{c.T}-d{c.d}-n{c.n}-{kind}{'-naive' if c.naive else ''}-{c.route}")


# ---- the plan of a case and the facts read off it -----------------------------------------------------------------------------
def case_plans(c, cus):
    """(route name, plan of the forward-only launch, plan of the gradient launch) on `cus` compute units"""
    out = []
    for want_grad in (False, True):
        # (forward-only launches of one-channel paths stay on the fp32-sweep kernels: the case's gradient launch is the one meant)
        r = generic_route(c.A, c.B, c.T, c.d, c.n, c.kind, want_grad, c.naive, c.route == "precise", c.sym, cus)
        out.append((r[0], generic_plan(c.A, c.B, c.T, c.d, c.n, want_grad, c.sym and c.A == c.B, r[1], r[2], cus)) if r else (None, None))
    return out[1][0], out[0][1], out[1][1]


def facts(c, cus):
    """what a case's claim is compared with: the gradient launch's plan entries (the forward-only launch's where the gradient
    launch is refused) and what follows from them"""
    route, pf, pg = case_plans(c, cus)
    pl = pg if pg is not None else pf
    T, d = c.T, c.d
    f = dict(pl, route_name=route, table_fwd=pf and pf["table"], table_grad=pg and pg["table"], r=1 << c.n,
             last_band=pl["P"] - 64 * (pl["nbands"] - 1), last_chunk=c.B - pl["JC"] * (pl["nchunks"] - 1),
             rounds=pl["items"] > pl["grid"], per_cu=max(1, min(8, 160 * 1024 // pl["lds"])), cblocks=-(-d // 16),
             dp=d + 1 if d % 2 == 0 else d)
    big = pl["table"] == "big"
    f["parts"] = 1 if big or T > 32 else (16 if T <= 4 else 8 if T <= 8 else 4 if T <= 16 else 2)
    f["passes"] = 1 if f["parts"] > 1 else -(-T // 64)

    def refused(want_grad):
        r = generic_route(c.A, c.B, T + 1, d, c.n, c.kind, want_grad, c.naive, c.route == "precise", c.sym, cus)
        return r is not None and generic_plan(c.A, c.B, T + 1, d, c.n, want_grad, c.sym, r[1], r[2], cus) is None

    f["last_accepted"] = refused(False) and refused(True)
    f["last_accepted_grad"] = refused(True)
    return f


def assert_claim(c, cus):
    """the case reaches the branch it names; -> its facts"""
    f = facts(c, cus)
    assert (c.want == "fwd") == (f["table_grad"] is None), (c, f)
    for k, v in c.claim:
        assert f[k] == v, (c.edge, case_id(c), k, f[k], v)
    return f


# ---- inputs ---------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def inputs(c):
    """(X, Y, w): fp32 paths (the rough 0.3-step walks of tests/test_gpu_generic.py) and signed fp32 weights, the same
    values on both I/O types; Y is X for the symmetric cases"""
    X = walks(c.A, c.T, c.d, c.seed, c.scale)
    Y = X if c.sym else walks(c.B, c.T, c.d, c.seed + 1, c.scale)
    return X, Y, signed_weights(c.A, c.B, c.seed + 2).astype(np.float32)


# ---- the oracle, plain and with the kernel's roundings ------------------------------------------------------------------------
MISTAKES = ("stale_S", "short_chunk_last_dropped", "r128_one_band", "f32_increments", "first_channel_block_only")


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def _phi(kind, s):
    return np.exp(-s) if kind == RBF else (RR.phi(kind, s) if kind in (IMQ, RQ) else MR.phi(kind, s))


def _neg_dphi(kind, s):
    return np.exp(-s) if kind == RBF else (RR.neg_dphi(kind, s) if kind in (IMQ, RQ) else MR.neg_dphi(kind, s))


def solve(X, Y, w=None, kind=RBF, h=1.0, n=0, naive=False, table=None, want_grad=True, mistake=None, JC=None):
    """(K [A, B], gX [A, T, d] or None): d sum(w K) / dX through the first slot (w None: ones).  table None: the plain fp64
    oracle; "f64" / "f32" / "big": with the roundings of that mode of the kernel (module docstring).  mistake: one of
    MISTAKES, a wrong kernel restated (JC: the launch's chunk, for the two mistakes of the column loop)."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    (A, T, d), B = X.shape, Y.shape[0]
    w = np.ones((A, B)) if w is None else np.array(w, np.float64)
    r, Tm = 1 << n, T - 1
    K, gX = np.empty((A, B)), (np.zeros((A, T, d)) if want_grad else None)
    if mistake == "short_chunk_last_dropped":
        assert B % JC, "the last chunk is full"
        w[:, B - 1] = 0.0
    step = max(1, (1 << 22) // (B * (r * Tm + 1) ** 2))
    for i0 in range(0, A, step):
        Xc = X[i0:i0 + step]
        a = len(Xc)
        if kind == LINEAR:
            Yc = np.broadcast_to(Y, (a, B, T, d))
            Xz = Xc
            G = np.einsum("ipk,ijqk->ijpq", Xz, Yc)
        else:  # (translation-invariant: centred on x_i's first point, as the kernel stages them)
            Xz = Xc - Xc[:, :1]
            Yc = Y[None] - Xc[:, None, :1]
            s = ((Xz**2).sum(-1)[:, None, :, None] + (Yc**2).sum(-1)[:, :, None, :] - 2.0 * np.einsum("ipk,ijqk->ijpq", Xz, Yc)) / float(h)
            G = _phi(kind, s)
        D = O.increments(G)
        if table == "f32" or mistake == "f32_increments":
            D = _f32(D)
        g = O.refine(D, n)
        Kfull = O.pde_sweep(g, naive)
        K[i0:i0 + step] = Kfull[..., -1, -1]
        if not want_grad:
            continue
        Krev = O.pde_sweep(g[..., ::-1, ::-1], naive)[..., ::-1, ::-1]
        Kf = Kfull[..., :-1, :-1]
        GG = (Kf if table is None else _f32(Kf)) * Krev[..., 1:, 1:]
        if table == "big":
            assert n == 0
            GG = _f32(GG)
        GG = GG.reshape(a, B, Tm, r, Tm, r)
        if mistake == "r128_one_band":
            assert r == 128
            GG = GG[:, :, :, :64]
        S = GG.sum(axis=(3, 5)) / float(r * r)
        if mistake == "stale_S":  # Sm not re-zeroed per column: every column of a chunk adds to what the chunk left there
            for j0 in range(0, B, JC):
                S[:, j0:j0 + JC] = np.cumsum(S[:, j0:j0 + JC], axis=1)
        R = np.zeros((a, B, T, T))
        R[:, :, 1:, 1:] += S
        R[:, :, :-1, :-1] += S
        R[:, :, 1:, :-1] -= S
        R[:, :, :-1, 1:] -= S
        wR = w[i0:i0 + step, :, None, None] * R
        if kind == LINEAR:
            gc = np.einsum("ijmn,ijnc->imc", wR, Yc)
        else:
            rg = wR * _neg_dphi(kind, s)
            gc = (-2.0 / float(h)) * (Xz * rg.sum(axis=(1, 3))[..., None] - np.einsum("ijmn,ijnc->imc", rg, Yc))
        gX[i0:i0 + step] = gc
    if mistake == "short_chunk_last_dropped":
        K[:, B - 1] = 0.0  # (never stored)
    if mistake == "first_channel_block_only" and want_grad:
        gX[..., 16:] = 0.0
    return K, gX


def e_rows(c):
    """the rows E is taken on: all of them up to E_CELLS cells of the refined grids"""
    return min(c.A, max(1, E_CELLS // (c.B * (((c.T - 1) << c.n) + 1) ** 2)))


@lru_cache(maxsize=None)
def plain(c, weights="signed", rows=None):
    """the plain oracle of a case (its first `rows` rows): (K, gX); weights "signed" (the case's w) or "ones" """
    X, Y, w = inputs(c)
    return solve(X[:rows], Y, w[:rows] if weights == "signed" else None, c.kind, c.h, c.n, c.naive)


@lru_cache(maxsize=None)
def restated(c, table, weights="signed", want_grad=True, mistake=None, JC=None, rows=None):
    X, Y, w = inputs(c)
    return solve(X[:rows], Y, w[:rows] if weights == "signed" else None, c.kind, c.h, c.n, c.naive, table, want_grad, mistake, JC)


@lru_cache(maxsize=None)
def restatement_error(c, table, weights="signed"):
    """(E_K, E_g) of mode `table` on the case's inputs: rel_entry of K and rel_max of the gradient, restated against plain"""
    Kp, gp = plain(c, weights, e_rows(c))
    Kr, gr = restated(c, table, weights, rows=e_rows(c))
    return rel_entry(Kr, Kp, 0, min_ref=MIN_K), rel_max(gr, gp)


def tolerances(c, table, io, weights="signed"):
    """(tol_K, tol_g) of a launch on increment table `table` with I/O type `io` ("f32" / "f64")"""
    E_K, E_g = restatement_error(c, table, weights)
    u = U32 if io == "f32" else FP64_FLOOR
    tol_K = K_EXACT[io] if table in ("f64", "big") else min(MARGIN * E_K + u, K_CAP)
    return tol_K, min(MARGIN * E_g + u, G_CAP)


def assert_generic(c, table, io, K, Kref, g=None, gref=None, weights="signed", where=""):
    """The assertion of the device tests: K per entry (|K_ref| >= MIN_K asserted) and the gradient over its largest entry,
    within `tolerances`.  Prints each figure before it asserts; -> (error / tolerance of K, of the gradient or None)."""
    tol_K, tol_g = tolerances(c, table, io, weights)
    e_K = rel_entry(K, Kref, 0, min_ref=MIN_K)
    e_g = None if g is None else rel_max(g, gref)
    print(f"{case_id(c)} [{c.edge}] {where} table {table} {io}: K {e_K:.2e} / {tol_K:.2e}"
          + ("" if g is None else f", gradient {e_g:.2e} / {tol_g:.2e}"))
    assert e_K < tol_K, (case_id(c), where, "K", e_K, tol_K)
    if g is not None:
        assert e_g < tol_g, (case_id(c), where, "gradient", e_g, tol_g)
    return e_K / tol_K, None if g is None else e_g / tol_g


def reference(c, weights="signed"):
    """What the device results are compared with: the C oracle (RBF and linear kinds), else the numpy oracle"""
    if c.kind in (RBF, LINEAR):
        from oracle import c_oracle as C

        X, Y, w = inputs(c)
        return C.gram_fwd_bwd(X, Y, c.h, c.n, naive=c.naive, kind=c.kind, grad_out=w.astype(np.float64) if weights == "signed" else None)
    return plain(c, weights)


# ---- the exact pass at known flag positions (tests/test_gpu_repair_flags.py) ---------------------------------------------------
# An fp32-sweep kernel flags a pair of paths in <= 3 channels whose condition number in the increments
#     c1 = sum_cells |S D| / max(|K|, 0.1)   (S, D on the coarse grid)
# exceeds 150, or whose grid maximum exceeds 4 max(|K|, 0.1) in two channels; a forward-only launch, which
# has no S, flags sum |K_fwd g| max(grid maximum, 1) / max(|K|, 0.1) > 300.  The batches below hold one rough pair (x*, y*) with
# c1 >= 300 and the forward-only figure >= 600, twice either threshold, at chosen rows and columns of a batch of very smooth
# paths, whose pairs are far below every rule: the flagged pairs among them are known.
FlagShape = namedtuple("FlagShape", "T d n h rough smooth pool")
FLAG_FAST = FlagShape(64, 2, 0, 0.05, 0.2, 0.005, 24)    # register-resident kernel
FLAG_QUAD = FlagShape(100, 2, 0, 0.05, 0.2, 0.005, 16)   # quadrant kernel
FLAG_BAND = FlagShape(33, 2, 3, 0.05, 0.2, 0.005, 24)    # 256 cells: the band kernels, both schedules
C1_TARGET, FWD_TARGET, C1_SMOOTH = 300.0, 600.0, 75.0


def conditioning(X, Y, h, n=0):
    """(K, c1, km, fwd) [A, B] on the oracle: the condition number of the gradient launches' rule, the largest |K| on the
    grid, and the forward-only launches' figure"""
    Kf, g, Gs = O.gram_forward_full(X, Y, RBF, h, n)
    D = O.increments(Gs)
    (A, B), Tm, r = Kf.shape[:2], X.shape[1] - 1, 1 << n
    S = O.gg_matrix(Kf, g).reshape(A, B, Tm, r, Tm, r).sum(axis=(3, 5)) / float(r * r)
    K = Kf[..., -1, -1]
    den = np.maximum(np.abs(K), 0.1)
    km = np.abs(Kf).max(axis=(2, 3))
    return K, np.abs(S * D).sum(axis=(2, 3)) / den, km, np.abs(Kf[..., :-1, :-1] * g).sum(axis=(2, 3)) * np.maximum(km, 1.0) / den


@lru_cache(maxsize=None)
def flag_pair(fs):
    """(x*, y*) [T, d] fp32: the first pair of a seeded pool of rough walks with c1 >= C1_TARGET, the forward-only figure >=
    FWD_TARGET and |K| >= 0.2"""
    rng = np.random.default_rng(7)
    Xr, Yr = (np.cumsum(fs.rough * rng.standard_normal((fs.pool, fs.T, fs.d)), axis=1).astype(np.float32) for _ in range(2))
    K, c1, _, fwd = conditioning(Xr, Yr, fs.h, fs.n)
    i, j = np.argwhere((c1 >= C1_TARGET) & (fwd >= FWD_TARGET) & (np.abs(K) >= 0.2))[0]
    return Xr[i], Yr[j]


def smooth_paths(fs, N, seed):
    return walks(N, fs.T, fs.d, seed, fs.smooth)


def flag_batch(fs, A, B, rows, cols):
    """(X [A], Y [B], targeted [A, B] bool, smooth [A, B] bool): x* at `rows` of X, y* at `cols` of Y, smooth walks elsewhere"""
    xs, ys = flag_pair(fs)
    X, Y = smooth_paths(fs, A, 31), smooth_paths(fs, B, 32)
    X[list(rows)], Y[list(cols)] = xs, ys
    r, c = np.zeros(A, bool), np.zeros(B, bool)
    r[list(rows)], c[list(cols)] = True, True
    return X, Y, r[:, None] & c[None, :], ~r[:, None] & ~c[None, :]


def flag_batch_sym(fs, N, at_x, at_y):
    """(X [N], targeted [N, N], smooth [N, N]): x* at `at_x`, y* at `at_y` of one batch -- the pairs (x*, y*) and their mirror
    images (y*, x*), the same pair, are the targeted ones"""
    xs, ys = flag_pair(fs)
    X = smooth_paths(fs, N, 33)
    X[list(at_x)], X[list(at_y)] = xs, ys
    a, b = np.zeros(N, bool), np.zeros(N, bool)
    a[list(at_x)], b[list(at_y)] = True, True
    t = a[:, None] & b[None, :]
    return X, t | t.T, ~(a | b)[:, None] & ~(a | b)[None, :]


ROWS, COLS = (0, 7, 8, 9), (0, 63, 64, 127, 128, 129)         # ordered 10 x 130: both ends of a full tile of 8 rows and of a
#                                                               last tile of two; both ends of the 64-flag words, a short last word
SYM_X, SYM_Y = (0, 7, 8, 64, 129), (3, 63, 65, 127, 128)      # Y is X, N = 130: targeted pairs on both sides of the diagonal
