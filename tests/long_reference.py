"""Inputs, point classes, reference, restatement and checker of the per-point tests of the long route (ring_sweep.h,
gram_long_kernels.h, long_static.h): the device tests are tests/test_gpu_long_points.py, the checker is itself checked in
tests/test_long_reference_cpu.py.  Modelled on tests/sweep_reference.py, which does the same for the fp32-sweep kernels.

Why.  The long route's gradient files hold a gradient to rel_max < 1e-5, the largest error over the largest entry of the tensor,
on rough walks (steps of 0.5 or 2.0 per channel at bandwidth 1) that drift apart: the static kernel is 0 on most of the grid, and
the largest entry sits at an end point.  A wrong S entry on a band-edge row then stays inside the bound in most columns
(profiles/long_points.txt has the figures), and an interior point is held at 10-600 times the stated bound.

Inputs (fp32-valued, so both I/O types share one reference; bandwidth H = 1; A = 3, B = 2; signed weights).
    close    parity.sized_walks of overall size 0.9 (0.9 / sqrt(d) per channel): the unflagged (GG), EXACT_ADJOINT and NAN_TAILS
             launches and the six static kinds.  K is of order 1 and every cell of the grid is live.
    bounded  parity.bounded_points, independent Gaussian points of sd BOUNDED_SIZE / sqrt(d) per channel: LOG_K and
             NORMALIZED.  Bounded, so the static kernel never decays; rough, so K grows: ln K(x, x) > 40 at 131 points (the
             running exponent passes the drift threshold 8 in most blocks of 64 steps), and PAST_FP32_T is the smallest T at
             which ln K(x, x) > 88.8 for every path of the case's seeds (found on the CPU, asserted in the CPU file: it holds
             at T and fails at T - 1).  Cross pairs of independent rough paths have K of order 1 to 1e3, now and then <= 0:
             the seeds are those whose every pair is positive.
The conditions of the CPU file on the fp64 reference, over every case: every K and diagonal K > 0; every pair has >= 99 % of its
cells with |D| > 1e-6 of its largest; every point of every path has a gradient above 1e-4 of the tensor's largest entry; zeroing
the S entry of any cell of rows 63, 64, 127, 128 in every pair moves gX or gY by more than 1e-5 of its largest entry.  A seed
that fails one takes the next (SEED_BUMP says which did).

Point classes, per path (gY: the same with X and Y exchanged).  The seams are read from the code:
    ends {0, T-1};  next {1, T-2};  interior: the rest
    band   coarse points m with m << n a multiple of 64, 0 < m < T - 1, and their two neighbours: the 64-row bands of
           ring_forward / ring_reverse (`kb * kWave`); on the column side the 64-step refill blocks (`s0 += kWave`)
    pass   points 63 k - 1, 63 k, 63 k + 1: static_grad_pass runs 63 points per outer pass (`o0 += kWave - 1`), lane 0 holding
           point o0 - 1 only to hand its S row up
    wrap   on the side that runs along columns (gY, dG's columns, and gX of a Y_IS_X launch, whose column side feeds it):
           coarse columns W - 1, W, W + 1 where plans.ring_plan's W (ring_make_plan: 128 at order 0) is below N - 1
The metric of a class is, per path, max |g - g_ref| over the class over the path's own class maximum of the reference; band, pass
and wrap divide by the path's interior maximum.  Per path: a strong path cannot cover a weak one (with NORMALIZED they differ
by orders of magnitude).

Reference: the existing fp64 helpers -- exact_adjoint_reference.pde (EXACT_ADJOINT), log_k_reference.log_pde (LOG_K,
NORMALIZED), and for GG the oracle's K_fwd K_rev as sweep_reference._pairs(fp32=False) forms it; the 4-corner scatter and the
static kernel's chain are exact_adjoint_reference's and log_k_reference._chain.

Restatement: the same fp64 arithmetic with the two fp32 roundings the kernels document (ring_sweep.h): the stored forward value
(K_fwd[p][q]; c[p][q] under EXACT_ADJOINT) is fp32, and each lane partial (sum over the r columns of a block) r^-2 is fp32; the r
rows of a block are added in fp64 (ring_S), the scatter and the chain run in fp64 (static_grad_pass).  LOG_K: the sweeps are
carried under powers of two, which leave the mantissas alone, and the partial filed is GG / K.  NORMALIZED: the diagonal pass is
restated the same way and the diagonal pair of a Y_IS_X launch is left out of both terms.  With Y_IS_X
each unordered pair is restated once, its column side giving the second path's share.
E_c is the class metric of the restatement against the reference, the largest over the case's launch forms and paths, and
    tol_c = min(4 E_c + u_out, 1e-5 max |g_ref| / den_c),   u_out = 2^-24 (fp32 output) or 1e-10 (fp64),
the rule and margin of tests/sweep_reference.py and tests/generic_reference.py; the second term keeps the class assertion at or
inside the existing contract rel_max < 1e-5, which is asserted beside it unchanged.  E never comes from a device result.

MISTAKES are wrong kernels restated in numpy on top of the restatement; `touches` says where each can happen."""
from functools import lru_cache

import numpy as np

import exact_adjoint_reference as EA
import log_k_reference as LK
from oracle import sigkernel_oracle as O
from parity import bounded_points, rel_max, signed_weights, sized_walks
from plans import ring_plan

f32 = np.float32
H = 1.0
A, B = 3, 2
SCALE = 0.9
BOUNDED_SIZE = 1.1 * np.sqrt(2.0)  # over sqrt(d) per channel: sd 1.1 at d = 2, 0.9 at d = 3
U_OUT = {"f32": 2.0 ** -24, "f64": 1e-10}
MARGIN = 4.0
CONTRACT = 1e-5
LIVE, LIVE_SHARE, WEAKEST_POINT = 1e-6, 0.99, 1e-4
SEAM_ROWS = (63, 64, 127, 128)
PAST_FP32_T = 277  # the smallest T whose bounded paths (d = 2) all have ln K(x, x) > 88.8 (test_long_reference_cpu.py)

# name -> (TX, TY, d, n)
CASES = {
    "T131": (131, 131, 2, 0),      # three bands (64 + 64 + 2), W capped at 128 < 130, pass seams at 63 and 126
    "P65_Q8": (66, 9, 3, 0),       # last band of one row, one 8-deep ring
    "Q130": (9, 131, 3, 0),        # one band, column wrap and column-side pass seams (gY)
    "d17": (70, 20, 17, 0),        # the second group of 16 channels across a band edge
    "n1_T66": (66, 40, 3, 1),      # P = 130 at order 1, block sums of 2 x 2
    "n2_T33": (33, 18, 3, 2),      # P = 128 = two full bands, coarse point 16 on the edge
    "past_fp32": (PAST_FP32_T, PAST_FP32_T, 2, 0),
}
CLOSE_CASES = ("T131", "P65_Q8", "Q130", "d17", "n1_T66", "n2_T33")
BOUNDED_CASES = ("T131", "n1_T66", "past_fp32")
F32_CASES = ("T131", "P65_Q8", "n2_T33")
NAN_LENGTHS = ((63, 64, 127), (65, 131))  # of X's and Y's paths in the NAN_TAILS launch of T131
FLAGS = ("gg", "exact", "log", "norm", "nan")
FAMILY = {"gg": "close", "exact": "close", "nan": "close", "log": "bounded", "norm": "bounded"}
FORMS = ("long", "long2", "yx", "yx_sym", "pair")
TWO_SIDED = ("long2", "yx", "yx_sym")
# (case, family) -> added to the seeds; a seed that fails an input condition takes the next.  What the seeds passed over failed:
#   T131, close         0: a point of gY under EXACT_ADJOINT at 1.4e-5 of the largest entry
#   n1_T66, bounded     0 .. 4: a pair with discrete K <= 0 (independent rough paths: K(x, y) is what is left of terms that
#                       cancel); 5: a point of gX under LOG_K at 7.9e-5 of the largest entry
#   past_fp32, bounded  (each seed at its own smallest T with ln K(x, x) > 88.8)  0: 8 and 7 columns of rows 63 and 64 hidden; 1 .. 8:
#                       a pair with K <= 0; 9: one column of row 64 hidden; 10: under NORMALIZED two columns of row 63 hidden (the
#                       cross pairs' S under their weights w K^); 11: a pair with K <= 0; 12: under NORMALIZED a point of a gradient
#                       below 1e-4 of the largest entry and a hidden column
SEED_BUMP = {("T131", "close"): 1, ("n1_T66", "bounded"): 6, ("past_fp32", "bounded"): 13}


def forms_of(flag):
    return {"gg": FORMS, "exact": FORMS, "log": TWO_SIDED, "norm": TWO_SIDED, "nan": ("long2", "yx")}[flag]


def cases_of(flag):
    return BOUNDED_CASES if FAMILY[flag] == "bounded" else (("T131",) if flag == "nan" else CLOSE_CASES)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def inputs(case, family):
    """(X [3, TX, d], Y [2, TY, d], w [3, 2], w_yx [3, 3]) as fp64 arrays of fp32 values"""
    TX, TY, d, n = CASES[case]
    s = 100 * list(CASES).index(case) + SEED_BUMP.get((case, family), 0)
    if family == "close":
        X = sized_walks(np.random.default_rng(1000 + s), A, TX, d, SCALE / np.sqrt(d))
        Y = sized_walks(np.random.default_rng(2000 + s), B, TY, d, SCALE / np.sqrt(d))
    else:
        sd = BOUNDED_SIZE / np.sqrt(d)
        X, Y = bounded_points(1000 + s, A, TX, d, sd), bounded_points(2000 + s, B, TY, d, sd)
    w = signed_weights(A, B, 3000 + s).astype(f32).astype(np.float64)
    wyx = signed_weights(A, A, 4000 + s).astype(f32).astype(np.float64)
    return X.astype(np.float64), Y.astype(np.float64), w, wyx


def rough_inputs(case, step):
    """rough walks as tests/test_gpu_exact_adjoint.py, test_gpu_log_k.py, test_gpu_normalized.py and test_gpu_nan_tails.py draw
    them, at a case's shape (cumulative steps of `step` per channel)"""
    TX, TY, d, n = CASES[case]
    _, _, w, wyx = inputs(case, "close")
    return LK.walks(17, A, TX, d, step, f32).astype(np.float64), LK.walks(18, B, TY, d, step, f32).astype(np.float64), w, wyx


# ---- point classes ----------------------------------------------------------------------------------------------------------
def ring_W(N, n):
    """the plan's ring width in coarse columns for grids of N coarse points on the column side (ring_make_plan)"""
    return ring_plan(2, N, n, True, 0, 256)["W"]


def band_points(T, n):
    return [m for m in range(1, T - 1) if (m << n) % 64 == 0]


def pass_points(T):
    return [o for o in range(63, T, 63)]


def classes(T, n, wrap=False):
    """{class: sorted point indices} of a path of T points at order n; wrap: the path runs along the grid's columns"""
    ends, nxt = {0, T - 1}, {1, T - 2} - {0, T - 1}
    interior = set(range(T)) - ends - nxt
    inner = set(range(T)) - ends  # (an end point is in `ends` alone: its gradient is an order of magnitude above the rest)
    out = dict(ends=ends, next=nxt, interior=interior,
               band={u for m in band_points(T, n) for u in (m - 1, m, m + 1)} & inner,
               **{"pass": {u for o in pass_points(T) for u in (o - 1, o, o + 1)} & inner})
    W = ring_W(T, n)
    if wrap and W < T - 1:
        out["wrap"] = {W - 1, W, W + 1} & inner
    return {k: sorted(v) for k, v in out.items() if v}


def class_metrics(g, gref, n, wrap=False, lengths=None):
    """{class: [(error / den, worst point, den) per path]}; den: the path's class maximum of the reference (band, pass, wrap:
    its interior maximum); lengths: each path's own (NAN_TAILS), the rows past it are not in any class"""
    g, gref = np.asarray(g, np.float64), np.asarray(gref, np.float64)
    out = {}
    for i in range(len(gref)):
        T = gref.shape[1] if lengths is None else lengths[i]
        cl = classes(T, n, wrap)
        for name, pts in cl.items():
            den_pts = cl["interior"] if name in ("band", "pass", "wrap") and "interior" in cl else pts
            den = np.abs(gref[i, den_pts]).max()
            assert den > 0, (name, i, T, n)
            err = np.abs(g[i, pts] - gref[i, pts]).max(axis=-1)
            out.setdefault(name, []).append((float(err.max() / den), int(pts[int(err.argmax())]), float(den)))
    return out


def cell_metrics(g, gref, n):
    """dG [pairs, M, N] of the PDE launches: the classes are the products of the row classes and the column classes (the corner
    cells are ends x ends); den: the grid's class maximum with band, pass and wrap replaced by interior"""
    g, gref = np.asarray(g, np.float64), np.asarray(gref, np.float64)
    M, N = gref.shape[1:]
    rows, cols = classes(M, n), classes(N, n, True)
    out = {}
    for rn, rp in rows.items():
        for cn, cp in cols.items():
            rd = rows["interior"] if rn in ("band", "pass") and "interior" in rows else rp
            cd = cols["interior"] if cn in ("band", "pass", "wrap") and "interior" in cols else cp
            for k in range(len(gref)):
                den = np.abs(gref[k][np.ix_(rd, cd)]).max()
                assert den > 0
                err = np.abs(g[k] - gref[k])[np.ix_(rp, cp)]
                a, b = np.unravel_index(int(err.argmax()), err.shape)
                out.setdefault(f"{rn}x{cn}", []).append((float(err.max() / den), (rp[a], cp[b]), float(den)))
    return out


# ---- the PDE of a batch of grids: reference and restatement ---------------------------------------------------------------------
MISTAKES = ("band_seam_one_side", "partial_dropped", "stale_forward_cell", "ring_wrap", "pass_seam", "block_row_missing",
            "wji_for_wij", "log_block_exponent", "norm_diagonal_term")
LOG_DRIFT = 8  # kLogDrift of ring_sweep.h


def _lambda(g):
    """the adjoint multipliers lambda [..., P, Q] of exact_adjoint_reference.adjoint (which returns lambda c)"""
    P, Q = g.shape[-2:]
    Ac, Bc, _, _ = EA._coef(g, False)
    lam = np.zeros(g.shape[:-2] + (P + 1, Q + 1))
    alpha, beta = np.zeros_like(lam), np.zeros_like(lam)
    for s in range(P + Q - 2, -1, -1):
        p = np.arange(max(0, s - Q + 1), min(P, s + 1))
        q = s - p
        lam[..., p, q] = 1.0 if s == P + Q - 2 else alpha[..., p, q + 1] + alpha[..., p + 1, q] - beta[..., p + 1, q + 1]
        alpha[..., p, q] = Ac[..., p, q] * lam[..., p, q]
        beta[..., p, q] = Bc[..., p, q] * lam[..., p, q]
    return lam[..., :P, :Q]


def _pow2(s, v):
    return 2.0 ** np.floor(np.log2(np.abs(v).max(axis=-1)))


def _factors(G, n, flag, wrapped):
    """-> (value [...], stored [..., P, Q], other [..., P, Q], log2 |K| [..., P+1, Q+1] or None): the pair's K (ln K with LOG_K)
    and the two factors of dK / dg = stored * other (dK / dg / K with LOG_K): the forward sweep's stored value and what the
    reverse sweep carries.  wrapped: the reverse sweep reads the increment of column b - W at columns b >= W (`ring_wrap`)."""
    g = O.refine(O.increments(np.asarray(G, np.float64)), n)
    gr = g
    if wrapped:
        Wc = ring_W(G.shape[-1], n) << n
        gr = g.copy()
        gr[..., Wc:] = g[..., :g.shape[-1] - Wc]
    if flag in ("gg", "nan"):
        Kf = O.pde_sweep(g)
        Kr = O.pde_sweep(gr[..., ::-1, ::-1])[..., ::-1, ::-1]
        return Kf[..., -1, -1], Kf[..., :-1, :-1], Kr[..., 1:, 1:], None
    if flag == "exact":
        Kf = O.pde_sweep(g)
        _, _, dA, dB = EA._coef(g, False)
        c = (Kf[..., 1:, :-1] + Kf[..., :-1, 1:]) * dA - Kf[..., :-1, :-1] * dB
        return Kf[..., -1, -1], c, _lambda(gr), None
    P, Q = g.shape[-2:]
    Ks, c = LK.scaled_sweep(g, _pow2)  # powers of two: the mantissas are the unscaled solve's, as in the kernels
    Rs, e = LK.scaled_sweep(gr[..., ::-1, ::-1], _pow2)
    Rs = Rs[..., ::-1, ::-1]
    m = Ks[..., P, Q]
    assert (m > 0).all(), "a pair of a LOG_K case has K <= 0"
    lnK = np.log(m) + c[..., P + Q]
    s = np.add.outer(np.arange(P), np.arange(Q))
    other = Rs[..., 1:, 1:] * np.exp(c[..., s] + e[..., (P + Q - 2) - s] - lnK[..., None, None])
    with np.errstate(divide="ignore"):
        l2 = (np.log(np.abs(Ks)) + c[..., np.add.outer(np.arange(P + 1), np.arange(Q + 1))]) / np.log(2.0)
    return lnK, Ks[..., :-1, :-1], other, l2


def _wrong_block_factor(l2):
    """`log_block_exponent` on ONE pair: [P, Q] powers of two the stored forward values are off by when the rows of a reverse
    block below Rsplit are scaled with the upper block's forward exponent.  The forward sweep of band kb keeps one exponent per
    block of 64 steps, changed at a block's start once the lanes' largest exponent has drifted past LOG_DRIFT (ring_forward);
    lane l stores K_fwd[p][q] on step l + q, and the reverse block that starts at stored row Rtop reads rows Rtop - 63 .. Rtop,
    which lie in the forward blocks hb = Rtop >> 6 and hb - 1 (ring_reverse)."""
    P, Q = l2.shape[0] - 1, l2.shape[1] - 1
    out = np.ones((P, Q))
    for kb in range(-(-P // 64)):
        L = min(64, P - 64 * kb)
        lane = np.arange(L)
        nblk = (Q + 63 + 63) // 64
        ef, E = np.zeros(nblk + 1, int), 0
        for blk in range(1, nblk):
            q = 64 * blk - 1 - lane
            ok = (q >= 0) & (q < Q)
            if ok.any():
                e = int(np.floor(l2[64 * kb + lane[ok] + 1, q[ok] + 1].max())) + 1 - E
                if abs(e) > LOG_DRIFT:
                    E += e
            ef[blk] = E
        t = lane[:, None] + np.arange(Q)[None, :]
        R0 = Q - 1 + L - 1
        sp = R0 - t
        hb = np.maximum(R0 - (sp - sp % 64), 0) >> 6
        wrong = t < (hb << 6)
        out[64 * kb:64 * kb + L] = np.where(wrong, 2.0 ** (ef[hb] - ef[np.maximum(hb - 1, 0)]), 1.0)
    return out


def pair_S(G, n, flag, restate=False, mistake=None):
    """static-kernel grids G [..., M, N] -> (K [...] (ln K with LOG_K), S [..., M-1, N-1] = dK/dD (/ K with LOG_K)).
    Without restate: the existing references.  restate: the kernels' two fp32 roundings (module docstring), and `mistake`."""
    G = np.asarray(G, np.float64)
    if not restate:
        assert mistake is None
        if flag == "exact":
            return EA.pde(G, n)[:2]
        if flag in ("log", "norm"):
            return LK.log_pde(G, n)[:2]
    val, stored, other, l2 = _factors(G, n, flag, mistake == "ring_wrap")
    lead, (P, Q), r = stored.shape[:-2], stored.shape[-2:], 1 << n
    if restate:
        stored = stored.astype(f32).astype(np.float64)
    if mistake == "stale_forward_cell":  # (one cell: the middle column of row 64)
        stored = stored.copy()
        stored[..., 64, Q // 2] = stored[..., 63, Q // 2]
    if mistake == "log_block_exponent":
        l2f = l2.reshape((-1,) + l2.shape[-2:])
        stored = stored * np.stack([_wrong_block_factor(x) for x in l2f]).reshape(stored.shape)
    part = (stored * other).reshape(lead + (P, Q // r, r)).sum(-1) / float(r * r)
    if restate:
        part = part.astype(f32).astype(np.float64)
    if mistake == "partial_dropped":  # (one lane partial: the middle block column of row 64)
        part[..., 64, (Q // r) // 2] = 0.0
    rows = part.reshape(lead + (P // r, r, Q // r))
    if mistake == "block_row_missing":
        rows = rows[..., :r - 1, :]
    return val, rows.sum(-2)


def _R(S, n, mistake=None, side="row"):
    """dK / dG [..., M, N] from S, as the pass over the row side's (gX) or the column side's (gY) points forms it"""
    R = EA.scatter(S)
    if mistake not in ("band_seam_one_side", "pass_seam"):
        return R
    if side == "col":
        R, S = np.swapaxes(R, -1, -2).copy(), np.swapaxes(S, -1, -2)
    M = R.shape[-2]
    if mistake == "band_seam_one_side":  # point m takes S from the cell row above it only
        for m in band_points(M, n):
            R[..., m, :-1] -= S[..., m, :]
            R[..., m, 1:] += S[..., m, :]
    if mistake == "pass_seam" and M >= 65:  # point 63 takes the S row of point 62, which the lane below hands up, as 0
        R[..., 63, 1:] -= S[..., 62, :]
        R[..., 63, :-1] += S[..., 62, :]
    return np.swapaxes(R, -1, -2) if side == "col" else R


@lru_cache(maxsize=None)
def _block_exponent_moves(case, flag, yx):
    """whether a pair of the launch (NORMALIZED: of its diagonal pass too) has two forward blocks of different exponents that
    one reverse block reads: where `log_block_exponent` changes anything"""
    X, Y, _, _ = inputs(case, "bounded")
    n = CASES[case][3]
    grids = list(EA.static_gram(X, X if yx else Y, EA.RBF, H).reshape((-1, X.shape[1], (X if yx else Y).shape[1])))
    if flag == "norm":
        grids += [EA.static_gram(Z[i:i + 1], Z[i:i + 1], EA.RBF, H)[0, 0] for Z in ((X,) if yx else (X, Y)) for i in range(len(Z))]
    return any((_wrong_block_factor(_factors(G, n, "log", False)[3]) != 1.0).any() for G in grids)


def touches(mistake, case, flag, form):
    """whether the mistake can happen in a launch of this case, flag and form"""
    TX, TY, d, n = CASES[case]
    P = (TX - 1) << n
    col = form != "long"  # the column-side pass runs
    if form in ("yx", "yx_sym"):
        TY = TX
    if flag == "nan":
        return False
    if mistake == "band_seam_one_side":
        return bool(band_points(TX, n)) or (col and bool(band_points(TY, n)))
    if mistake in ("partial_dropped", "stale_forward_cell"):
        return P > 64
    if mistake == "ring_wrap":
        return ring_W(TY, n) < TY - 1
    if mistake == "pass_seam":
        return TX >= 65 or (col and TY >= 65)
    if mistake == "block_row_missing":
        return n >= 1
    if mistake == "wji_for_wij":
        return form == "yx"
    if mistake == "log_block_exponent":  # (cross pairs of the bounded inputs have K of order 1: their exponent may never move)
        return flag in ("log", "norm") and _block_exponent_moves(case, flag, form in ("yx", "yx_sym"))
    if mistake == "norm_diagonal_term":
        return flag == "norm"
    raise KeyError(mistake)


# ---- a launch: the gradients of a case in a form ---------------------------------------------------------------------------------
def _two_sided(X, Y, W, S, kind, n, once, mistake):
    """(gX, gY) from the pairs' S [A, B, M-1, N-1] and weights W.  once (Y_IS_X restated): pair (i, j), i <= j, is solved once,
    its row side gives x_i's share under w_ij and, i < j, its column side x_j's under w_ji (`wji_for_wij`: under w_ij)"""
    Rr, Rc = _R(S, n, mistake, "row"), _R(S, n, mistake, "col")
    if not once:
        return LK._chain(X, Y, W[:, :, None, None] * Rr, kind, H)[0], LK._chain(X, Y, W[:, :, None, None] * Rc, kind, H)[1]
    up, strict = np.triu(np.ones_like(W)), np.triu(np.ones_like(W), 1)
    Wc = W if mistake == "wji_for_wij" else W.T
    gr = LK._chain(X, Y, (W * up)[:, :, None, None] * Rr, kind, H)[0]
    gc = LK._chain(X, Y, (Wc * strict)[:, :, None, None] * Rc, kind, H)[1]
    return gr + gc, None


def solve(X, Y, w, n, flag="gg", form="long2", kind=EA.RBF, restate=False, mistake=None, lengths=None):
    """-> (K, gX, gY) of a launch: K [A, B] (ln K with LOG_K, K^ with NORMALIZED; [A] for "pair"), the gradients of sum(w K) in
    each slot (gY None where the launch has none: "long" and the Y_IS_X forms).  Forms: "long" gram_long_fwd_bwd, "long2"
    gram_long_fwd_bwd2 with both sides, "yx" / "yx_sym" its Y_IS_X launches (Y is X; w [A, A]), "pair" pair_fwd_bwd (w [A]).
    lengths (NAN_TAILS): ([TX_i], [TY_j]), every pair on its own truncated grid, the rows past a path's end zero."""
    assert mistake is None or (restate and mistake in MISTAKES)
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    yx = form in ("yx", "yx_sym")
    if yx:
        Y = X
    W = np.asarray(w, np.float64)
    if form == "pair":
        W = np.diag(W)
    if form == "yx_sym":
        W = W + W.T
    once = yx and restate
    if flag == "nan":
        lx, ly = lengths
        ly = lx if yx else ly
        K, gX, gY = np.zeros(W.shape), np.zeros_like(X), np.zeros_like(Y)
        for i in range(len(X)):
            for j in range(len(Y)):
                k, a, b = solve(X[i:i + 1, :lx[i]], Y[j:j + 1, :ly[j]], W[i:i + 1, j:j + 1], n, "gg", "long2", kind, restate, mistake)
                K[i, j] = k[0, 0]
                gX[i, :lx[i]] += a[0]
                gY[j, :ly[j]] += b[0]
        return K, gX, (None if yx else gY)
    val, S = pair_S(EA.static_gram(X, Y, kind, H), n, flag, restate, mistake)
    if once:  # the pair (j, i), j > i, is the pair (i, j) read the other way
        for i in range(len(X)):
            for j in range(i):
                S[i, j] = S[j, i].T
    if flag == "norm":
        diag = lambda Z: pair_S(np.stack([EA.static_gram(Z[i:i + 1], Z[i:i + 1], kind, H)[0, 0] for i in range(len(Z))]),
                                n, flag, restate, mistake)
        a, Sa = diag(X)
        b, Sb = (a, Sa) if yx else diag(Y)
        Kh = np.exp(val - 0.5 * a[:, None] - 0.5 * b[None, :])
        if yx:  # the diagonal pair's K^ is the constant 1: the launch leaves it out of both terms
            W = W - np.diag(np.diag(W))
        W = W * Kh
        val = Kh
    gX, gY = _two_sided(X, Y, W, S, kind, n, once, mistake)
    if flag == "norm":
        def diagonal_terms(Z, Sz, wz, skip):
            out = np.zeros_like(Z)
            for i in range(len(Z)):
                if i != skip:
                    gx, gy = _two_sided(Z[i:i + 1], Z[i:i + 1], wz[i].reshape(1, 1), Sz[i:i + 1, None], kind, n, False, mistake)
                    out[i] = gx[0] + gy[0]
            return out
        gX = gX + diagonal_terms(X, Sa, -0.5 * W.sum(1), 0 if mistake == "norm_diagonal_term" else -1)
        if not yx:
            gY = gY + diagonal_terms(Y, Sb, -0.5 * W.sum(0), -1)
    if form == "pair":
        val = np.diagonal(val).copy()
    return val, gX, (None if yx or form == "long" else gY)


def pde_solve(G, w, n, flag="gg", restate=False, mistake=None):
    """-> (K [pairs], dG [pairs, M, N]) of ops.pde_fwd_bwd on grids G [pairs, M, N] with weights w [pairs]"""
    K, S = pair_S(G, n, flag, restate, mistake)
    return K, np.asarray(w)[:, None, None] * _R(S, n, mistake, "row")


def _args(case, flag, form, rough=None):
    X, Y, w, wyx = inputs(case, FAMILY[flag]) if rough is None else rough_inputs(case, rough)
    n = CASES[case][3]
    if form == "pair":
        return dict(X=X[:B], Y=Y, w=w[0], n=n)
    if form in ("yx", "yx_sym"):
        return dict(X=X, Y=X, w=wyx, n=n)
    return dict(X=X, Y=Y, w=w, n=n)


def nan_lengths(form):
    return (NAN_LENGTHS[0], NAN_LENGTHS[0] if form == "yx" else NAN_LENGTHS[1])


@lru_cache(maxsize=None)
def plain(case, flag, form, kind=EA.RBF, rough=None):
    """the reference of a case's launch: (K, gX, gY)"""
    return solve(flag=flag, form=form, kind=kind, lengths=nan_lengths(form) if flag == "nan" else None,
                 **_args(case, flag, form, rough))


@lru_cache(maxsize=None)
def restated(case, flag, form, kind=EA.RBF, mistake=None, rough=None):
    return solve(flag=flag, form=form, kind=kind, restate=True, mistake=mistake,
                 lengths=nan_lengths(form) if flag == "nan" else None, **_args(case, flag, form, rough))


def pde_grids(case):
    """the PDE launches' inputs: the case's static-kernel grids rounded to fp32, [A B, M, N], and signed weights [A B]"""
    X, Y, w, _ = inputs(case, "close")
    G = EA.static_gram(X, Y, EA.RBF, H).astype(f32).astype(np.float64)
    return G.reshape((A * B,) + G.shape[2:]), w.reshape(-1)


@lru_cache(maxsize=None)
def pde_plain(case, flag):
    G, w = pde_grids(case)
    return pde_solve(G, w, CASES[case][3], flag)


@lru_cache(maxsize=None)
def pde_restated(case, flag, mistake=None):
    G, w = pde_grids(case)
    return pde_solve(G, w, CASES[case][3], flag, True, mistake)


# ---- tolerances and the class assertion -----------------------------------------------------------------------------------------
def sides(case, flag, form, got, ref):
    """[(side, g, g_ref, wrap, lengths)] of a launch's gradients"""
    TX, TY, d, n = CASES[case]
    yx = form in ("yx", "yx_sym")
    lx, ly = nan_lengths(form) if flag == "nan" else (None, None)
    out = [("gX", got[1], ref[1], yx, lx)]
    if ref[2] is not None:
        out.append(("gY", got[2], ref[2], True, ly))
    return out


@lru_cache(maxsize=None)
def class_error(case, flag, kind=EA.RBF):
    """{(side, class): E_c}: the restatement against the reference, the largest over the case's launch forms and paths"""
    n, E = CASES[case][3], {}
    for form in (forms_of(flag) if kind == EA.RBF else ("long2",)):  # (the other kinds run the two-sided launch only)
        ref, res = plain(case, flag, form, kind), restated(case, flag, form, kind)
        for side, g, gr, wrap, lengths in sides(case, flag, form, res, ref):
            for k, per_path in class_metrics(g, gr, n, wrap, lengths).items():
                E[(side, k)] = max(E.get((side, k), 0.0), max(e for e, _, _ in per_path))
    return E


@lru_cache(maxsize=None)
def pde_class_error(case, flag):
    m = cell_metrics(pde_restated(case, flag)[1], pde_plain(case, flag)[1], CASES[case][3])
    return {k: max(e for e, _, _ in v) for k, v in m.items()}


def check_classes(metrics, E, top, io, label, printer=print):
    """the class assertion on {class: [(err, worst, den) per path]}: err < min(MARGIN E_c + u_out, CONTRACT top / den).  Prints
    one PERPOINT line per class before it asserts; -> {class: worst err / tol} and the failures [(class, path, point, err, tol)]"""
    worst, failed = {}, []
    for k, per_path in metrics.items():
        ratios = []
        for i, (err, pt, den) in enumerate(per_path):
            tol = min(MARGIN * E[k] + U_OUT[io], CONTRACT * top / den)
            ratios.append((err / tol, err, tol, i, pt))
        ratio, err, tol, i, pt = max(ratios)
        worst[k] = ratio
        if printer:
            printer(f"PERPOINT {label} io={io} class={k} err={err:.3e} tol={tol:.3e} E={E[k]:.3e} worst=path {i} point {pt}")
        failed += [(k, i, pt, err, tol) for (ratio, err, tol, i, pt) in ratios if not ratio < 1.0]
    return worst, failed


def check_launch(case, flag, form, io, got, kind=EA.RBF, where="", printer=print):
    """The assertions of a gradient launch `got` = (K, gX, gY) against the case's reference: the contract rel_max < 1e-5 of each
    gradient, then the class tolerances.  -> ({(side, class): err / tol}, failures); the caller asserts that none failed."""
    ref = plain(case, flag, form, kind)
    E = class_error(case, flag, kind)
    n = CASES[case][3]
    worst, failed = {}, []
    for side, g, gr, wrap, lengths in sides(case, flag, form, got, ref):
        contract = rel_max(g, gr)
        if printer:
            printer(f"CONTRACT case={case} flag={flag} form={form} kind={kind} io={io} {where} {side} rel_max={contract:.3e}")
        if not contract < CONTRACT:
            failed.append((side, "contract", contract))
        w_, f_ = check_classes(class_metrics(g, gr, n, wrap, lengths), {k: v for (s, k), v in E.items() if s == side},
                               np.abs(gr).max(), io, f"case={case} flag={flag} form={form} kind={kind} {where} {side}", printer)
        worst.update({(side, k): v for k, v in w_.items()})
        failed += [(side,) + f for f in f_]
    return worst, failed


def check_pde(case, flag, io, dG, where="", printer=print):
    ref = pde_plain(case, flag)[1]
    failed = []
    contract = rel_max(dG, ref)
    if printer:
        printer(f"CONTRACT case={case} flag={flag} form=pde io={io} {where} dG rel_max={contract:.3e}")
    if not contract < CONTRACT:
        failed.append(("dG", "contract", contract))
    worst, f_ = check_classes(cell_metrics(dG, ref, CASES[case][3]), pde_class_error(case, flag), np.abs(ref).max(), io,
                              f"case={case} flag={flag} form=pde {where} dG", printer)
    return worst, failed + [("dG",) + f for f in f_]
