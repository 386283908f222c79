"""Inputs, point classes, reference and checker of the per-point tests of the fp32-sweep Gram kernels (gram_fast, gram_quad,
gram_dyad, gram_band): the device tests are tests/test_gpu_every_length.py, the checker is itself checked in
tests/test_sweep_reference_cpu.py.

Why.  The parity files hold a gradient to rel_max, the largest error over the largest entry of the whole [A, T, d] tensor, on
`parity.walks(.., 0.05)`.  The largest entry sits at an end point (moving an end point changes one increment, moving an
interior point two of opposite sign): on the fp64 oracle the strongest interior point is 0.10-0.15 of the strongest end
point in the median and 0.04 at worst, the weakest point 0.1-1 % of it from T = 33 on.  rel_max therefore holds the interior
as a class at 10-25 times the stated 1e-5 and single points at 100-1000 times -- and the interior is where the quadrant seams,
the band hand-overs, the ring wrap and the column-side travelling sums live.  Those walks also start together and drift apart:
the static kernel has decayed by the end of the path and the far corner of the grid barely reaches K.

Inputs.  X = sized_walks(default_rng(1000 + T), 3, T, d, s / sqrt(d)), Y = sized_walks(default_rng(2000 + T), 2, T, d,
s / sqrt(d)), s = SCALE = 0.9, h = 0.9; signed weights (seed 3000 + T; Y is X: N = 3, seed 4000 + T, asymmetric).  fp32-valued, so both I/O
types share one reference.  Refined grids: the same generator on the T coarse points.  Three conditions hold on the fp64
oracle (asserted in the CPU file over the whole case matrix, never on a device result), with the last cell's weight
|K[P,P] - K[P-r,P] - K[P,P-r] + K[P-r,P-r]| / |K[P,P]| (the last COARSE cell, r = 2^n):
    at most 10 % of all (case, pair) combinations below 1e-4;  every case has a pair at or above 1e-4;  0.25 <= |K| <= 16
for every K the device tests compare with, the X x Y pairs and the Y-is-X batch (k(x_i, x_i) included) alike.  At s = 1 the
Y-is-X batch reaches K = 18.9 (T = 52, d = 2) and 0.247 (T = 37, d = 2); s = 0.9 is the largest of 0.85, 0.9, 0.95, 1 with all
three conditions over both populations (0.95: K up to 16.2).  Measured over the case matrix of this file (order 0: 522 cases,
refined grids: 201): see LAST_CELL_FIGURES below, which the CPU file compares with what it measures.

Point classes of a case: ends {0, T - 1}, next {1, T - 2}, interior the rest, handover the points a kernel treats apart or
hands between wavefronts -- gram_quad: {63, 64, 65} within the interior; refined grids: every coarse point t with 0 < t 2^n < P
a multiple of 64, and its two neighbours; gram_fast: none.  The metric of a class is max |g - g_ref| over the class over
max |g_ref| over the class; the hand-over class divides by the interior maximum (by its own where a path has no interior).

Reference and tolerance.  `solve(.., fp32=False)` is the fp64 oracle (pinned to oracle/sigkernel_oracle.py in the CPU file).
`solve(.., fp32=True)` restates the fp32 arithmetic the kernels document (the headers of
gram_fast_kernel.h, gram_quad.hip, gram_dyad.hip and gram_band.hip; the V-form stencil as scripts/dev/precision_vform.py):
    static kernel and 4-corner increments in fp64 on paths centred on the column path's first point, gamma = D / (r^2 sqrt 12)
        rounded once to fp32 (refined grids: one value per coarse cell);
    both sweeps in fp32 difference form, V += gamma (sqrt3 t + gamma (t + K00)), K11 = K01 + V;
    S = K_fwd U in fp32;
    order 0: the 4-corner scatter R in fp32 as a difference of column differences;
    refined grids: the coarse table S_coarse / r^2 in fp32 -- gram_dyad.hip from fp32 runs along a fine row added in fp64,
        gram_band.hip from fp32 sums of S - 1 with the constant put back at the corners -- and R = (S00 + S11) - (S01 + S10)
        in fp32, the corners summed first as both kernels do (three times the error of the difference form at these sizes);
    G = 2^(ns e2) in fp32 from the fp32 differences of the centred coordinates, the argument rounded to fp32;
    the contractions sum R G (x~ - y~) in fp32, row side and (Y is X: each unordered pair once) column side;
    a pair's share (w (-2 / h)) * sum in fp32; the row side summed over partner paths in fp64 (refined grids: in fp32), the
        column side of a (row tile, column) item in fp32 (the three paths of a case are one tile).
Not restated: the two-float add of gram_band.hip at order >= 5 and gram_fast's stored G (the fp64 value rounded once): the
kernel is then more accurate than the restatement; the exact fp64 pass of flagged pairs (K only).  E_c is the class metric of the
restatement against the oracle, the largest over the three launch forms of the case (`class_error`), and
    tol_c = min(4 E_c + u_out, 1e-5 max |g_ref| / max_c |g_ref|),   u_out = 2^-24 (fp32 output) or 1e-10 (fp64),
the rule and the margin of tests/generic_reference.py (the kernel's fp64 increments differ from numpy's in their last bits, so
an equally distributed set of roundings falls the other way); the second term keeps the class assertion at or inside the
contract, which is asserted beside it unchanged: rel_entry(K, K_ref, 1e-6) < 1e-5 and rel_max(g, g_ref) < 1e-5.  E never comes
from a device result.

MISTAKES are wrong kernels restated on top of `solve(.., fp32=True)`, each a keyword; `touches` says where each can happen."""
from functools import lru_cache

import numpy as np

from oracle import sigkernel_oracle as O
from parity import rel_entry, rel_max, signed_weights, sized_walks, walks

f32 = np.float32
H = 0.9
SCALE = 0.9             # overall size of a path, over sqrt(d) per channel (module docstring, Inputs)
U_OUT = {"f32": 2.0 ** -24, "f64": 1e-10}
MARGIN = 4.0
CONTRACT = 1e-5          # the accuracy contract: K per entry, the gradient over its largest entry
SELF = 4e-6              # two fp32 solves of one pair, per entry (tests/test_gpu_fast.py)
LAST_CELL_MIN = 1e-4
K_RANGE = (0.25, 16.0)
SQRT12 = 3.46410161513775459
CLASSES = ("ends", "next", "interior", "handover")

# order 0: every length of both kernels; d = 3 and 7 are the padded forms of the 4- and 8-channel instantiations, 16 takes the
# row accumulator of gram_quad's gradient launches (no EARLY instantiation), d = 3 the FEW instantiation of its forward launches
FAST_T, QUAD_T = range(3, 65), range(65, 129)
FAST_D, FAST_D_EDGE, FAST_T_EDGE = (2, 3, 7, 14), (4, 8, 16), (3, 31, 32, 33, 63, 64)
QUAD_D = (3, 7, 14, 16)
REFINED_D = (2, 7, 14)
WIDE_T = (3, 32, 33, 64, 65, 112, 113, 128)   # also fp64 I/O and SIGSVGD_FLAG_SYM
# what the CPU file measured on the oracle over ORDER0_CASES / REFINED_CASES (pairs below 1e-4, pairs, smallest best pair of a
# case, K range over the X x Y pairs and the Y-is-X batch); it asserts the three conditions and compares its own figures with these
LAST_CELL_FIGURES = {"order0": (216, 3132, 3.50e-4, 0.373, 13.91), "refined": (12, 1206, 2.01e-3, 0.374, 13.43)}


def fast_ds(T):
    return FAST_D + (FAST_D_EDGE if T in FAST_T_EDGE else ())


def refined_tn():
    """every (T, n) whose refined grid the dyad or a band family takes: 3 <= T <= 33, 64 <= (T - 1) 2^n <= 256, the dyad
    family at orders 1 .. 6 up to 128 cells, the band family at orders 2 .. 7 (plans.gram_geometry)"""
    return [(T, n) for n in range(1, 8) for T in range(3, 34)
            if (1 <= n <= 6 and 64 <= (T - 1) << n <= 128) or (2 <= n <= 7 and 64 <= (T - 1) << n <= 256)]


ORDER0_CASES = [(T, d, 0) for T in FAST_T for d in fast_ds(T)] + [(T, d, 0) for T in QUAD_T for d in QUAD_D]
REFINED_CASES = [(T, d, n) for (T, n) in refined_tn() for d in REFINED_D]
ALL_CASES = ORDER0_CASES + REFINED_CASES


def family_of(T, n):
    """"fast" / "quad" / "refined": what decides a case's hand-over class (the device tests assert the launch's own family
    from plans.gram_geometry)"""
    return "refined" if n else ("fast" if T <= 64 else "quad")


# ---- inputs ---------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def inputs(T, d):
    """(X [3, T, d], Y [2, T, d], w [3, 2], w_yx [3, 3]): fp32 paths, fp64 signed weights (fp32-valued)"""
    X = sized_walks(np.random.default_rng(1000 + T), 3, T, d, SCALE / np.sqrt(d))
    Y = sized_walks(np.random.default_rng(2000 + T), 2, T, d, SCALE / np.sqrt(d))
    w = signed_weights(3, 2, 3000 + T).astype(f32).astype(np.float64)
    wyx = signed_weights(3, 3, 4000 + T).astype(f32).astype(np.float64)
    return X, Y, w, wyx


@lru_cache(maxsize=None)
def old_inputs(T, d, n):
    """the inputs of the earlier parity files at the same sizes: walks of step 0.05 (refined grids: 0.3)"""
    s = 0.05 if n == 0 else 0.3
    _, _, w, wyx = inputs(T, d)
    return walks(3, T, d, 1, s), walks(2, T, d, 2, s), w, wyx


# ---- point classes ----------------------------------------------------------------------------------------------------------
def seam_points(T, n):
    """the points with S on two sides of a hand-over: point 64 of gram_quad; refined grids: coarse t with t 2^n on a band edge"""
    if n == 0:
        return [64] if T >= 66 else []
    return [t for t in range(1, T - 1) if (t << n) % 64 == 0]


def classes(T, n):
    """{class: sorted point indices}; empty classes are left out"""
    ends, nxt = {0, T - 1}, {1, T - 2} - {0, T - 1}
    interior = set(range(T)) - ends - nxt
    if n == 0:
        hand = ({63, 64, 65} & interior) if T > 64 else set()
    else:
        hand = {u for t in seam_points(T, n) for u in (t - 1, t, t + 1)}
    out = dict(ends=ends, next=nxt, interior=interior, handover=hand)
    return {k: sorted(v) for k, v in out.items() if v}


def class_metrics(g, gref, T, n):
    """{class: (error / class maximum of the reference, worst point, class maximum)}; handover: over the interior maximum"""
    g, gref = np.asarray(g, np.float64), np.asarray(gref, np.float64)
    cl = classes(T, n)
    out = {}
    for name, pts in cl.items():
        den_pts = cl["interior"] if name == "handover" and "interior" in cl else pts
        den = np.abs(gref[:, den_pts]).max()
        assert den > 0, (name, T, n)
        err = np.abs(g[:, pts] - gref[:, pts]).max(axis=(0, 2))
        out[name] = (float(err.max() / den), int(pts[int(err.argmax())]), float(den))
    return out


# ---- the oracle, plain and with the kernels' roundings ------------------------------------------------------------------------
MISTAKES = ("seam_one_side", "last_group_skipped", "early_cut", "column_sum_missing_first", "column_sum_missing_last",
            "ring_wrap_early", "wji_for_wij")


def skipped_cells(mistake, T, n):
    """[P, P] bool: the cells whose step of the REVERSE sweep a wrong step count leaves out (the step then sees gamma = 0: V
    stays and the neighbour's value is copied), or None.
      last_group_skipped  the last group of anti-diagonals of the sweep's last quadrant: sweep statements of 8 steps
                          (gram_fast: 5 in the last at P = 63) or 16
      early_cut           gram_quad's EARLY instantiations (T <= 112) run a group of 16 steps while (S0 & ~15) <= slast =
                          rows + columns of the quadrant; the wrong kernel asks for (S0 & ~15) + 16 <= slast and starts a
                          quadrant's reverse sweep up to 16 anti-diagonals inside it"""
    P = (T - 1) << n
    p, q = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
    if mistake == "last_group_skipped":
        grp, Pq = (8 if n == 0 and T <= 64 else 16), min(P, 64)
        return p + q < (2 * Pq - 2) % grp + 1
    if mistake == "early_cut":
        if n or not 65 <= T <= 112:
            return None
        rows = np.where(p < 64, 64, P - 64)
        cols = np.where(q < 64, 64, P - 64)
        s = p % 64 + q % 64  # the cell's anti-diagonal in its quadrant: the reverse sweep runs the steps 124 .. 0, the cut is at its start
        return (s & ~15) + 16 > rows + cols
    return None


def touches(mistake, T, d, n, form):
    """whether the mistake can happen in a launch of this case (form: "ordered" / "yx" / "yx-sym")"""
    if mistake == "seam_one_side":
        return bool(seam_points(T, n))
    if mistake == "last_group_skipped":  # (a last group of one step is cell (0, 0) alone, whose U[0][0] = K no gradient reads)
        return int(skipped_cells(mistake, T, n).sum()) > 1
    if mistake == "early_cut":  # (d > 14: the gradient launch takes the row accumulator, which has no EARLY form)
        z = skipped_cells(mistake, T, n)
        return z is not None and bool(z.any()) and d <= 14
    if mistake in ("column_sum_missing_first", "column_sum_missing_last"):
        return form != "ordered"
    if mistake == "ring_wrap_early":
        return n == 0 and T == 33
    if mistake == "wji_for_wij":
        return form == "yx"
    raise KeyError(mistake)


def _sweep32(gam, zero=None):
    """gam [Np, P, P] fp32 (D / sqrt 12 per cell) -> K [Np, P + 1, P + 1] fp32 in difference form; zero: cells swept with 0"""
    if zero is not None:
        gam = np.where(zero, f32(0), gam)
    Np, P = gam.shape[0], gam.shape[-1]
    r3 = f32(np.sqrt(3.0))
    K = np.ones((Np, P + 1, P + 1), f32)
    V = np.zeros((Np, P), f32)
    for s in range(2 * P - 1):
        p = np.arange(max(0, s - P + 1), min(P, s + 1))
        q = s - p
        k10, k01, k00 = K[:, p + 1, q], K[:, p, q + 1], K[:, p, q]
        t = k10 + k01
        gm = gam[:, p, q]
        V[:, p] += gm * (r3 * t + gm * (t + k00))
        K[:, p + 1, q + 1] = k01 + V[:, p]
    assert K.dtype == f32 and V.dtype == f32
    return K


def _scatter(S, drop_rows=(), corners_first=False):
    """R = dL/dG from S = dL/dD, in S's type.  Order 0: a cell row's column differences formed once,
    R[m][n] = (S[m][n] - S[m][n-1]) - (S[m-1][n] - S[m-1][n-1]); corners_first (the coarse tables of gram_dyad.hip and
    gram_band.hip): (S[m-1][n-1] + S[m][n]) - (S[m-1][n] + S[m][n-1]).  drop_rows: the points whose row takes S from the cell
    row above it only."""
    Sp = np.zeros((S.shape[0], S.shape[1] + 2, S.shape[2] + 2), S.dtype)  # cell (a, b) at [a + 1, b + 1], zeros around the grid
    Sp[:, 1:-1, 1:-1] = S
    lo = Sp[:, 1:].copy()  # the cell row below a point
    if len(drop_rows):
        lo[:, list(drop_rows)] = 0
    up = Sp[:, :-1]
    if corners_first:
        return (up[:, :, :-1] + lo[:, :, 1:]) - (up[:, :, 1:] + lo[:, :, :-1])
    return (lo[:, :, 1:] - lo[:, :, :-1]) - (up[:, :, 1:] - up[:, :, :-1])


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c).astype(f32)


def _pairs(Xp, Yp, h, n, fp32, mistake, kernel=None):
    """the pairs (Xp[k], Yp[k]): K [Np], row-side gradient d k / d x [Np, T, d], column-side d k / d y [Np, T, d], last cell.
    fp32: the two sides are the raw fp32 sums of R G (x~ - y~) (`solve` applies weight and -2 / h as the kernels do);
    kernel: "dyad" / "band" on refined grids"""
    Np, T, d = Xp.shape
    r, Tm = 1 << n, T - 1
    c = Yp[:, :1]
    xt, yt = Xp - c, Yp - c
    diff = xt[:, :, None, :] - yt[:, None, :, :]
    G = np.exp(-(diff ** 2).sum(-1) / h)
    D = O.increments(G)
    if not fp32:
        g = O.refine(D, n)
        Kf = O.pde_sweep(g)
        Kr = O.pde_sweep(g[..., ::-1, ::-1])[..., ::-1, ::-1]
        S = (Kf[:, :-1, :-1] * Kr[:, 1:, 1:]).reshape(Np, Tm, r, Tm, r).sum(axis=(2, 4)) / float(r * r)
        RG = _scatter(S) * G
        row = (-2.0 / h) * np.einsum("pmn,pmnc->pmc", RG, diff)
        col = (2.0 / h) * np.einsum("pmn,pmnc->pnc", RG, diff)
        last = np.abs(Kf[:, -1, -1] - Kf[:, -1 - r, -1] - Kf[:, -1, -1 - r] + Kf[:, -1 - r, -1 - r]) / np.abs(Kf[:, -1, -1])
        return Kf[:, -1, -1], row, col, last
    gam = (D / (float(r * r) * SQRT12)).astype(f32)
    gam = np.repeat(np.repeat(gam, r, axis=1), r, axis=2)
    zr = skipped_cells(mistake, T, n)
    Kf = _sweep32(gam)
    U = _sweep32(gam[:, ::-1, ::-1], None if zr is None else zr[::-1, ::-1])[:, ::-1, ::-1]
    Kfw = Kf[:, :-1, :-1].copy()
    if mistake == "ring_wrap_early":  # a ring of P - 1 slots: the last column's K_fwd lands in the first column's slot
        Kfw[:, :, 0] = Kfw[:, :, -1]
    S = Kfw * U[:, 1:, 1:]
    if n and kernel == "band":
        # gram_band.hip: S - 1 summed in fp32 over a coarse cell (one fused multiply-add per cell), the constant put back at the
        # four corners of the point grid, where the scatter does not cancel it
        S = _fma32(Kfw, U[:, 1:, 1:], -1.0).reshape(Np, Tm, r, Tm, r).sum(axis=4, dtype=f32).sum(axis=2, dtype=f32)
        S = (S.astype(np.float64) / float(r * r)).astype(f32)
    elif n:
        # gram_dyad.hip: a fine row's run over a coarse cell in fp32, the runs added in fp64; the table entry S_coarse / r^2 in fp32
        S = S.reshape(Np, Tm, r, Tm, r).sum(axis=4, dtype=f32).astype(np.float64).sum(axis=2)
        S = (S / float(r * r)).astype(f32)
    R = _scatter(S, seam_points(T, n) if mistake == "seam_one_side" else (), corners_first=bool(n))
    if n and kernel == "band":
        for (a, b, sg) in ((0, 0, 1), (-1, -1, 1), (0, -1, -1), (-1, 0, -1)):
            R[:, a, b] += f32(sg)
    df = xt.astype(f32)[:, :, None, :] - yt.astype(f32)[:, None, :, :]
    e = (df * df).sum(-1, dtype=f32)
    G32 = np.exp2((e * f32(-np.log2(np.e) / h)).astype(np.float64)).astype(f32)  # 2^(e2 ns32), the argument rounded to fp32
    prod = (R * G32)[..., None] * df
    row, col = prod.sum(axis=2, dtype=f32), prod.sum(axis=1, dtype=f32)
    assert S.dtype == R.dtype == prod.dtype == row.dtype == f32
    if mistake == "column_sum_missing_first":
        col[:, 0] = 0
    if mistake == "column_sum_missing_last":
        col[:, -1] = 0
    return Kf[:, -1, -1].astype(np.float64), row, col, None


def solve(X, Y, w, h=H, n=0, yx=False, sym=False, fp32=False, mistake=None, kernel=None):
    """(K [A, B], gX [A, T, d], last-cell weights [A, B] or None): d sum(w K) / dX through the first slot; sym: w + w^T
    (SIGSVGD_FLAG_SYM).  fp32=False: the fp64 oracle on ordered pairs.  fp32=True: the kernels' arithmetic restated; with yx
    (Y is X) every unordered pair {i <= j} once, the row side giving x_i's share and the column side x_j's; a pair's share is
    (w (-2 / h)) * sum in fp32, the row side added up over the partners in fp64 (the refined-grid kernels: in fp32), the
    column side in fp32.
    kernel: "dyad" / "band" (refined grids; None: "dyad").  mistake: one of MISTAKES."""
    assert mistake is None or (fp32 and mistake in MISTAKES)
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    (A, T, d), B = X.shape, Y.shape[0]
    W = np.asarray(w, np.float64)
    if sym:
        W = W + W.T
    once = yx and fp32
    ij = [(i, j) for i in range(A) for j in range(i if once else 0, B)]
    I, J = [i for i, _ in ij], [j for _, j in ij]
    Kp, row, col, last = _pairs(X[I], Y[J], float(h), n, fp32, mistake, kernel)
    K, g = np.zeros((A, B)), np.zeros((A, T, d))
    g32 = np.zeros((A, T, d), f32)  # the fp32 row accumulators of gram_dyad.hip / gram_band.hip
    c32 = np.zeros((A, T, d), f32)  # the column-side sums of a (row tile, column) item, fp32 in every kernel (`cslab`)
    L = None if last is None else np.zeros((A, B))
    m2h = f32(-2.0 / h)
    for k, (i, j) in enumerate(ij):
        K[i, j] = Kp[k]
        if L is not None:
            L[i, j] = last[k]
        if not fp32:
            g[i] += W[i, j] * row[k]
            continue
        share = (f32(W[i, j]) * m2h) * row[k]
        if n:
            g32[i] += share
        else:
            g[i] += share
        if once and i < j:
            K[j, i] = Kp[k]
            c32[j] += -(f32(W[i, j] if mistake == "wji_for_wij" else W[j, i]) * m2h) * col[k]
    return K, g + g32 + c32, L


FORMS = ("ordered", "yx", "yx-sym")


def kernel_of(family):
    """the restatement's kernel of a launch family of plans.gram_geometry (None at order 0)"""
    return {"dyad": "dyad", "band serial": "band", "band parallel": "band"}.get(family)


def refined_kernels(T, n):
    """the refined-grid kernels a (T, order) can run on: gram_dyad up to 128 cells, gram_band from order 2 and 65 cells on"""
    P = (T - 1) << n
    return [k for k, ok in (("dyad", 1 <= n <= 6 and 64 <= P <= 128), ("band", 2 <= n <= 7 and 64 < P <= 256)) if ok]


def _form_args(T, d, n, form, old=False):
    X, Y, w, wyx = old_inputs(T, d, n) if old else inputs(T, d)
    if form == "ordered":
        return dict(X=X, Y=Y, w=w, n=n)
    return dict(X=X, Y=X, w=wyx, n=n, yx=True, sym=form == "yx-sym")


@lru_cache(maxsize=None)
def plain(T, d, n, form, old=False):
    """the oracle of a case's launch form: (K, gX, last-cell weights); old: on the earlier files' inputs"""
    return solve(**_form_args(T, d, n, form, old))


@lru_cache(maxsize=None)
def restated(T, d, n, form, mistake=None, old=False, kernel=None):
    kernel = (kernel or refined_kernels(T, n)[0]) if n else None
    return solve(fp32=True, mistake=mistake, kernel=kernel, **_form_args(T, d, n, form, old))[:2]


@lru_cache(maxsize=None)
def restatement_error(T, d, n, form, kernel=None):
    """(E_K per entry, E of the whole gradient, {class: E_c}) of the restatement against the oracle on the case's inputs"""
    Kp, gp, _ = plain(T, d, n, form)
    Kr, gr = restated(T, d, n, form, kernel=kernel)
    return rel_entry(Kr, Kp, 1e-6), rel_max(gr, gp), {k: v[0] for k, v in class_metrics(gr, gp, T, n).items()}


@lru_cache(maxsize=None)
def class_error(T, d, n, kernel=None):
    """{class: E_c} of a case: the largest over its three launch forms.  A class is two or three points of three paths, so one
    form's figure is the maximum of a handful of roundings and varies by a factor of two between the forms of one case (T = 17,
    d = 2, order 4, "next": 7.0e-7 ordered, 1.43e-6 and 1.24e-6 with Y is X); the forms are three draws of the same arithmetic on
    the same paths, and their maximum is the class's rounding scale rather than one draw of it."""
    Es = [restatement_error(T, d, n, form, kernel)[2] for form in FORMS]
    return {k: max(E[k] for E in Es) for k in Es[0]}


def tolerances(T, d, n, form, io, kernel=None):
    """{class: tol_c} of a gradient launch with I/O type `io` ("f32" / "f64")"""
    _, gp, _ = plain(T, d, n, form)
    E = class_error(T, d, n, kernel)
    top = np.abs(gp).max()
    return {k: min(MARGIN * E[k] + U_OUT[io], CONTRACT * top / den)
            for k, (_, _, den) in class_metrics(gp, gp, T, n).items()}


def assert_contract(K, Kref, g=None, gref=None, where=""):
    eK = rel_entry(K, Kref, 1e-6)
    assert eK < CONTRACT, (where, "K", eK)
    if g is not None:
        eg = rel_max(g, gref)
        assert eg < CONTRACT, (where, "gradient", eg)


def assert_classes(T, d, n, form, io, g, gref, where="", family=None):
    """The class assertion of the device tests.  Prints each figure before it asserts (one PERPOINT line per class);
    -> {class: error / tolerance}."""
    tol = tolerances(T, d, n, form, io, kernel_of(family))
    E = class_error(T, d, n, kernel_of(family))
    m = class_metrics(g, gref, T, n)
    for k, (err, worst, _) in m.items():
        print(f"PERPOINT family={family or family_of(T, n)} T={T} d={d} n={n} form={form} io={io} {where} class={k} "
              f"err={err:.3e} tol={tol[k]:.3e} E={E[k]:.3e} worst={worst}")
    for k, (err, worst, _) in m.items():
        assert err < tol[k], (where, T, d, n, form, io, k, "point", worst, err, tol[k])
    return {k: m[k][0] / tol[k] for k in m}
