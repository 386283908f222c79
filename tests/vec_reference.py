"""What the tests of the vector kernels share (`vec_fused_kernel` in csrc/vec_fused.hip, `vec_sqdist_kernel`
and `vec_kgrad_kernel` in csrc/vec_kernels.hip; tests/test_gpu_vec_edges.py on the device, tests/test_vec_reference_cpu.py for the
checker itself): inputs in two forms, the fp64 references, PER-ENTRY bounds that are derived and not measured, the assertion, and
numpy restatements of the kernels' order of operations with the mistakes kernels of this shape can make.  Not a test module.

What is computed:  sq[i,j] = max(0, sum_c (x_ic - y_jc)(xm_ic - ym_jc))   (xm = x M, ym = y M; no metric: xm = x, ym = y)
                   K = f(t), t = hh * sq, hh = 1/(2 h^2);  gaussian f = w = exp(-t);  imq f = (1 + t)^-1/2, w = (1 + t)^-3/2;
                   unit K = sq, w = 1;   dK[i,c] = s * sum_j go[i,j] w[i,j] (xm_ic - ym_jc)

The kernels' constants.
  vec_fused_kernel<NT, METRIC, VEC4>   a workgroup owns FM = 64 rows and walks `per` column tiles of FN = 64; NT = 4, 8, 16, 32
      accumulator tiles serve D <= 64, 128, 256, 512; every operand is centred on row 0 of Y (of YM for xm, ym); S = XM~ Y~^T
      (+ X~ YM~^T with a metric) runs over the channels in stages of 64 (plain) or 32 (metric), each thread staging 8 or 4
      consecutive channels of one row; a_i = sum xm~ x~ comes from the FIRST tile a workgroup walks, b_j = sum ym~ y~ from every
      tile; sq = max(a + b - cross, 0), cross = 2 S (plain) or S (metric); W = go w(sq) passes through LDS; O += W YM~ in stages
      of 64 channels; dK = s (xm~ wsum - O).  With a gradient the column tiles are split over min(ntile, ceil(512 / row tiles))
      workgroups, per = ceil(ntile / splits) tiles each (the last split may own fewer), and the splits' partial dK are joined
      in split order from a workspace, or meet in fp32 atomics without one; without a gradient every tile is its own workgroup.
      Rows are fetched 16 bytes at a time (VEC4) where D % 4 == 0 and X, Y, XM, YM are all 16-byte aligned.
  vec_sqdist_kernel<T, METRIC>   64 x 64 output tiles, channels in stages of 16, direct differences, one sequential chain per entry.
  vec_kgrad_kernel<T>   a workgroup owns 16 rows x 64 channels and walks the partners in stages of 64; K is written by channel
      block 0 only; acc += w (xm - ym) sequentially over the partners.

Inputs (`vec_inputs`), seeded from (seed, A, B, D, form).
  integer  X, Y in -3..3, grad_out in 1..3, the metric 2 on the diagonal and 1 on the first superdiagonal (not symmetric), so
           XM, YM are integers in -9..9; grad_scale one of +-1, +-2.  Centring on Y[0] keeps integers (|x~| <= 6, |xm~| <= 18).
           Every partial sum -- a_i, b_j, S, O, xm~ wsum, the split partials and their join -- is an integer whose magnitude is
           bounded by the sums of absolute values `assert_exact_sums` forms; it asserts them below 2^24 on every set handed out
           (35,162 is the largest on the sets the tests use, 15,659 without the metric).  So with the `unit` kind every fp32
           product and sum is exact in any order, on the atomic route too: sq, K = sq and dK must EQUAL the reference.
  float    X = +-uniform[1, 2], Y = +-uniform[0.25, 0.5], grad_out = uniform[0.5, 1.5]: every channel's (x - y)^2 is at least
           0.25, so a channel or partner lost, doubled or taken from a neighbour moves sq by at least 0.25 (`float_margin`).
           With the metric the channel term (x - y)_c (xm - ym)_c has no such floor; the float form with a metric checks the
           bound, and lost terms under a metric are the integer form's to catch.
  In both forms the last two rows of X, the last two rows of Y and the last two channels of each differ and Y[0, D-1] != 0
  (drawn again if not), so a row, partner or channel taken from its neighbour, or a centre not subtracted, is a different number.
  The bandwidth (`half_inv_h2`): h^2 is the power of four nearest 4 D, so hh = 1/(2 h^2), 1/h^2 and h are exact in fp32 and
  fp64, hh * sq is exact for an integer sq, and t stays within about [0.03, 5] so no K underflows.

Bounds.  u = 2^-24 (2^-53 for fp64 I/O), gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms,
Lemma 3.1): a term that passes through n roundings is off by at most gamma(n) times its magnitude, in any order of summation.
  sq, direct differences (`sq_bound_direct`)   gamma(D + 3) sum_c |dx_c| |dm_c|  (= gamma(D + 3) sq_ref without a metric: all
      terms are non-negative, the bound is relative).  A term passes through the two subtractions, its product and at most
      D - 1 additions whose operands are both non-zero (adding zero padding is exact): D + 2, and one to spare.
  sq, fused expansion (`sq_bound_fused`)   gamma(n + 3) (A_i + B_j + C_ij) in the centred operands, A_i = sum |xm~| |x~|,
      B_j = sum |ym~| |y~|, C_ij = 2 sum |xm~| |y~| (plain) or sum |xm~| |y~| + sum |x~| |ym~| (metric), n = D (plain) or 2 D
      (metric: both cross products run through ONE accumulator, 2 D terms).  A term of the cross sum: two centrings (one per
      operand, each relative to the centred value), one product (none if the matrix core fuses it), at most n - 1 additions,
      the final subtraction: n + 3.  A term of a_i or b_j: two centrings, no product rounding (fused multiply-add), at most D - 1
      additions (the thread's chain and the three shuffle steps together add D terms), then fl(a + b) and the subtraction: D + 3.
      The doubling 2 S is exact, the clamp at zero moves a result towards the non-negative reference.  c = 3.
  K (`kernel_bounds`)   t' = fl(hh sq') with |sq' - sq| <= e_sq: |t' - t| <= hh e_sq (1 + u) + u t =: e_t.
      gaussian  |exp(-t') - exp(-t)| <= K expm1(e_t); plus the function evaluation, F ulps of K.
      imq       den' = fl(1 + t'): |den' - den| <= e_t + u (den + e_t) =: e_d; f is decreasing and convex, so
                |f(den') - f(den)| <= (den - e_d)^-1/2 - den^-1/2; plus F ulps of K.  w' = fl(k' / den'):
                |w' - w| <= (K + e_K) / (den - e_d) (1 + u) - w.
      unit      e_K = e_sq, e_w = 0.
      F (`F_ULPS`) is the one number IEEE arithmetic does not give: the device's exp, sqrt and division (two-launch path), __expf
      and rsqrtf (fused).  It is measured against the fp64 function at the integer form's sq, which the device holds exactly, as
      the largest error beyond the derived part, doubled for arguments not sampled and rounded up to whole ulps (one ulp of K
      is taken as 2 u |K|).  It may not exceed 8.
  dK (`dk_bound`)   |s| (gamma(B + ntile + 6) sum_j |go| |w| (|xm~_i| + |ym~_j|) + (1 + gamma) sum_j |go| e_w (|xm~_i| + |ym~_j|)).
      Fused: a term W_ij ym~_jc passes through fl(w go), the centring of ym~, its product, at most B - 1 additions inside the
      split partials, the subtraction from xm~ wsum, the product with s and at most splits - 1 <= ntile - 1 additions of the join
      (fixed order or atomics): B + ntile + 3; a term of xm~ wsum the same with the centring of xm~.  Two-launch: fl(xm - ym)
      (|xm - ym| <= |xm~| + |ym~|), fl(w go), the product, B - 1 additions, the product with s: B + 3.  c' = ntile + 6 covers both.
  fp64 I/O   at u = 2^-53 the fp64 reference's own rounding counts and is added by the same derivations (`expected`).
  integer form   e_sq = 0; with `unit` every bound is 0.  With gaussian and imq e_t = 0 (hh is a power of two), so K is f at the
      exact sq within e_d's rounding and the F ulps, and dK follows from e_w."""
import numpy as np

from oracle import vector_oracle as VO

U32, U64 = 2.0 ** -24, 2.0 ** -53
FM, FN, FK_PLAIN, FK_METRIC, FC = 64, 64, 64, 32, 64  # vec_fused.hip
VT, VC = 64, 16                                       # vec_sqdist_kernel
GR, GJ, GC = 16, 64, 64                               # vec_kgrad_kernel
FORMS = ("integer", "float")
KINDS = ("unit", "gaussian", "imq")
SEED = 11
# ulps of K allowed to the device's function evaluation, per path: 2 x the largest error seen beyond the derived part on the
# integer form's exact arguments, rounded up (measured on an MI355X over every shape of tests/test_gpu_vec_edges.py; the
# measured figure beside each)
F_ULPS = {
    "fused": 4,        # __expf 1.77 ulps, rsqrtf 0.37 ulps
    "two_launch": 2,   # exp 0.62 ulps, 1 / sqrt 0.45 ulps
    "two_launch64": 2  # fp64 exp 1.00 ulps, 1 / sqrt 0.97 ulps (numpy's own fp64 functions are part of these two figures;
}                      # `expected` adds one ulp for the reference besides)
F_MAX = 8

# ---- shapes (A, B, D) of the device tests; tests/test_gpu_vec_edges.py says which edge each is for ---------------------------
FUSED_D = [1, 3, 4, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 508, 511, 512]
FUSED_D_SHAPES = [(65, 70, D) for D in FUSED_D]
_FA, _FB = [1, 15, 16, 17, 63, 64, 65, 129], [1, 63, 64, 65, 127, 128, 129, 193]
FUSED_AB_SHAPES = [(a, _FB[(i + k) % 8], D) for D in (5, 68) for k in (0, 3) for i, a in enumerate(_FA)] + [(64, 65, 5), (64, 65, 68)]
FUSED_BIG_SHAPES = [(4097, 641, 5), (4097, 641, 68)]  # 65 row tiles -> 8 splits wanted, 11 tiles -> 2 per split, 6 splits, last of 1
FUSED_GUARDED_SHAPES = [(33, 70, 5), (65, 63, 68), (68, 132, 129)]
FUSED_ALIGN_SHAPES = [(65, 70, 64), (65, 70, 68)]
SQDIST_SHAPES = [(a, b, D) for D in (1, 15, 16, 17, 32, 33, 64)
                 for a, b in ((1, 1), (63, 65), (64, 64), (65, 129), (129, 63), (1, 129), (65, 1))]
KGRAD_SHAPES = [(a, b, D) for D in (1, 3, 63, 64, 65, 128, 129)
                for a, b in ((1, 1), (15, 63), (16, 64), (17, 65), (33, 128), (17, 129), (1, 65), (33, 1))]


def gamma(n, u=U32):
    return n * u / (1.0 - n * u)


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def half_inv_h2(D, metric=False):
    """hh = 1 / (2 h^2) with h^2 the power of four nearest 4 D (16 D with the metric, whose sq is about four times as large)"""
    return 0.5 * 4.0 ** -round(np.log(4.0 * D * (4 if metric else 1)) / np.log(4.0))


def fused_geometry(A, B, grad=True):
    """fused_splits of vec_fused.hip restated: row tiles, column tiles, column splits and tiles per split of a launch"""
    ntile, rows = -(-B // FN), -(-A // FM)
    splits = max(1, min(ntile, -(-512 // rows) if grad else ntile))
    per = -(-ntile // splits)
    return {"rows": rows, "ntile": ntile, "splits": -(-ntile // per), "per": per}


def fused_workspace_bytes(A, B, D):
    g = fused_geometry(A, B)
    return g["splits"] * A * D * 4 + 256 if g["splits"] > 1 else 0


# ---- inputs ----------------------------------------------------------------------------------------------------------------
class VecInputs:
    """X [A, D], Y [B, D], go [A, B] as fp32 arrays, XM / YM (None without a metric), the scalar grad_scale, and the form"""

    def __init__(self, X, Y, go, XM, YM, grad_scale, form):
        self.X, self.Y, self.go, self.XM, self.YM, self.grad_scale, self.form = X, Y, go, XM, YM, grad_scale, form
        (self.A, self.D), self.B = X.shape, Y.shape[0]
        self.metric = XM is not None
        self.launch_A = self.A  # the rows of the launch these are rows of (`take_rows`): what sets its split geometry

    def take_rows(self, R):
        """the same inputs restricted to rows R of X (rows are independent; the CPU tests cap the large shapes with it)"""
        sub = VecInputs(self.X[R], self.Y, self.go[R], None if self.XM is None else self.XM[R], self.YM, self.grad_scale, self.form)
        sub.launch_A = self.launch_A
        return sub

    def centred(self):
        """(xm~, x~, ym~, y~) in fp64: every operand minus row 0 of Y (of YM for xm, ym)"""
        X, Y = _f64(self.X), _f64(self.Y)
        XM, YM = (_f64(self.XM), _f64(self.YM)) if self.metric else (X, Y)
        return XM - YM[0], X - Y[0], YM - YM[0], Y - Y[0]

    def grad_operands(self):
        return (self.XM, self.YM) if self.metric else (self.X, self.Y)


def metric_matrix(D):
    return 2.0 * np.eye(D) + np.eye(D, k=1)


def vec_inputs(A, B, D, seed, form, metric=False):
    rng = np.random.default_rng([seed, A, B, D, FORMS.index(form)])
    while True:
        if form == "integer":
            X, Y, go = rng.integers(-3, 4, (A, D)), rng.integers(-3, 4, (B, D)), rng.integers(1, 4, (A, B))
        else:
            assert form == "float"
            X = rng.choice([-1.0, 1.0], (A, D)) * rng.uniform(1.0, 2.0, (A, D))
            Y = rng.choice([-1.0, 1.0], (B, D)) * rng.uniform(0.25, 0.5, (B, D))
            go = rng.uniform(0.5, 1.5, (A, B))
        if ((A == 1 or (X[-1] != X[-2]).any()) and (B == 1 or (Y[-1] != Y[-2]).any()) and Y[0, -1] != 0
                and (D == 1 or ((X[:, -1] != X[:, -2]).any() and (Y[:, -1] != Y[:, -2]).any()))):
            break
    s = float(rng.choice([-2.0, -1.0, 1.0, 2.0]))
    X, Y, go = (np.ascontiguousarray(a, dtype=np.float32) for a in (X, Y, go))
    XM = YM = None
    if metric:
        M = metric_matrix(D)
        XM, YM = (np.ascontiguousarray(_f64(a) @ M, dtype=np.float32) for a in (X, Y))
    inp = VecInputs(X, Y, go, XM, YM, s, form)
    if form == "integer":
        assert_exact_sums(inp)
    return inp


def assert_exact_sums(inp):
    """the 2^24 condition of the integer form: every operand an integer, and the sums of absolute values that bound every
    partial sum of either path (in any order, any grouping) below 2^24.  -> the largest of them"""
    for a in (inp.X, inp.Y, inp.go, inp.XM, inp.YM):
        assert a is None or np.array_equal(a, np.rint(a))
    xm, x, ym, y = (np.abs(a) for a in inp.centred())
    a_i, b_j = (xm * x).sum(1), (ym * y).sum(1)
    cross = xm @ y.T + x @ ym.T
    sq_abs = a_i[:, None] + b_j[None, :] + cross  # bounds a, b, S, their combination, and the direct sum as well
    go = np.abs(_f64(inp.go))
    dk_abs = abs(inp.grad_scale) * (xm * go.sum(1)[:, None] + go @ ym)  # w = 1: O, xm~ wsum, partials, join, and direct sums
    top = max(float(sq_abs.max()), float(dk_abs.max()))
    assert top < 2 ** 24, top
    return top


# ---- fp64 references -------------------------------------------------------------------------------------------------------
def _row_chunks(A, B, D, limit=1 << 18):
    step = max(1, limit // max(1, B * D))
    return [(i, min(A, i + step)) for i in range(0, A, step)]


def sq_reference(X, Y, XM=None, YM=None, absolute=False):
    """sq in fp64, the oracle's own functions on row blocks (the [A, B, D] difference tensor of a block at a time): without a
    metric `VO.pw_dist_sq`; with one the operands XM, YM are the kernels' inputs as given, and the sum is
    `VO.scaled_pw_dist_sq`'s (diff_M * diff).sum(-1) with diff_M = XM - YM.  absolute: sum_c |dx| |dm| (the direct bound's sum)"""
    X, Y, XM, YM = _f64(X), _f64(Y), _f64(XM), _f64(YM)
    (A, D), B = X.shape, Y.shape[0]
    out = np.empty((A, B))
    for lo, hi in _row_chunks(A, B, D):
        if XM is None:
            out[lo:hi] = VO.pw_dist_sq(X[lo:hi], Y)
        else:
            diff, diff_M = X[lo:hi, None, :] - Y[None], XM[lo:hi, None, :] - YM[None]
            out[lo:hi] = np.abs(diff_M * diff).sum(-1) if absolute else np.maximum((diff_M * diff).sum(-1), 0.0)
    return out


def kernel_reference(sq, kind, hh):
    """(K, w) in fp64"""
    sq = _f64(sq)
    if kind == "unit":
        return sq, np.ones_like(sq)
    if kind == "gaussian":
        K = np.exp(-hh * sq)
        return K, K
    assert kind == "imq"
    den = 1.0 + hh * sq
    return den ** -0.5, den ** -1.5


def dk_reference(sq, XM, YM, go, kind, hh, s):
    """the weighted gradient in fp64: `VO.vec_kernel_weighted_grad` for the two kernels it has (h = (2 hh)^-1/2, a power of two), the same sum with w = 1 for `unit`"""
    if kind != "unit":
        h = float(np.sqrt(0.5 / hh))
        assert 0.5 / h ** 2 == hh
        return VO.vec_kernel_weighted_grad(sq, XM, YM, go, kind, h, s)
    w = np.ones_like(_f64(sq)) if go is None else _f64(go)
    return s * (_f64(XM) * w.sum(1, keepdims=True) - w @ _f64(YM))


# ---- bounds ----------------------------------------------------------------------------------------------------------------
def _cached(inp, name, make):
    """`make()` once per input set (the [A, B, D] passes are the expensive part of a test)"""
    if name not in inp.__dict__:
        inp.__dict__[name] = make()
    return inp.__dict__[name]


def sq_of(inp):
    return _cached(inp, "_sq", lambda: sq_reference(inp.X, inp.Y, inp.XM, inp.YM))


def sq_bound_direct(inp, u=U32):
    if not inp.metric:  # all terms non-negative: the sum of absolute values is sq itself
        return gamma(inp.D + 3, u) * sq_of(inp)
    return gamma(inp.D + 3, u) * _cached(inp, "_sq_abs", lambda: sq_reference(inp.X, inp.Y, inp.XM, inp.YM, absolute=True))


def sq_bound_fused(inp):
    xm, x, ym, y = (np.abs(a) for a in inp.centred())
    n = 2 * inp.D if inp.metric else inp.D
    return gamma(n + 3) * ((xm * x).sum(1)[:, None] + (ym * y).sum(1)[None, :] + xm @ y.T + x @ ym.T)


def kernel_bounds(sq, e_sq, kind, hh, u, f_ulps):
    """(e_K, e_w) of the module docstring"""
    assert 0 <= f_ulps <= F_MAX
    sq, e_sq = _f64(sq), _f64(e_sq)
    if kind == "unit":
        return e_sq, np.zeros_like(sq)
    t = hh * sq
    e_t = hh * e_sq * (1 + u) + (0.0 if _power_of_two(hh) else u) * t  # (a power of two multiplies exactly)
    K, w = kernel_reference(sq, kind, hh)
    if kind == "gaussian":
        e_K = K * np.expm1(e_t) + f_ulps * 2 * u * K
        return e_K, e_K
    den = 1.0 + t
    e_d = e_t + u * (den + e_t)
    lo = den - e_d
    assert (lo > 0.5).all()
    e_K = (lo ** -0.5 - K) + f_ulps * 2 * u * K
    return e_K, (K + e_K) / lo * (1 + u) - w


def _power_of_two(v):
    m, _ = np.frexp(v)
    return m == 0.5


def dk_bound(inp, w, e_w, u=U32, weighted=True):
    xm, _, ym, _ = (np.abs(a) for a in inp.centred())
    go = np.abs(_f64(inp.go)) if weighted else np.ones((inp.A, inp.B))
    g = gamma(inp.B + -(-inp.B // FN) + 6, u)
    both = g * go * np.abs(w) + (1 + g) * go * e_w
    return abs(inp.grad_scale) * (xm * both.sum(1)[:, None] + both @ ym)


class Expected:
    """references and per-entry bounds of one launch: sq, K, dK and e_sq, e_K, e_dK"""


def expected(inp, kind, path, hh=None, fp64=False, weighted=True):
    """path: "fused" or "two_launch".  Integer form: e_sq = 0, and with `unit` every bound is 0 (the result must equal the
    reference)."""
    assert path in ("fused", "two_launch") and kind in KINDS and not (fp64 and path == "fused")
    u = U64 if fp64 else U32
    hh = half_inv_h2(inp.D, inp.metric) if hh is None else hh
    e = Expected()
    e.hh, e.u = hh, u
    e.sq = sq_of(inp)
    if inp.form == "integer":
        e.e_sq = np.zeros_like(e.sq)
    else:
        e.e_sq = sq_bound_fused(inp) if path == "fused" else sq_bound_direct(inp, u)
    e.K, w = kernel_reference(e.sq, kind, hh)
    e.e_K, e_w = kernel_bounds(e.sq, e.e_sq, kind, hh, u, F_ULPS[path + ("64" if fp64 else "")])
    XM, YM = inp.grad_operands()
    e.dK = dk_reference(e.sq, XM, YM, inp.go if weighted else None, kind, hh, inp.grad_scale)
    exact = inp.form == "integer" and kind == "unit"
    e.e_dK = np.zeros_like(e.dK) if exact else dk_bound(inp, w, e_w, u, weighted)
    if fp64 and not exact:
        # at u = 2^-53 the fp64 reference's own rounding counts: the oracle takes the same direct differences (the same bound
        # again on a float-form sq; an integer sq is exact), evaluates f to an ulp, and forms dK as XM sum_j W - W @ YM in the
        # operands as given, B + 3 roundings a term
        e.e_sq = 2 * e.e_sq
        if kind != "unit":
            e.e_K, e_w = kernel_bounds(e.sq, e.e_sq, kind, hh, u, F_ULPS["two_launch64"] + 1)
            e.e_dK = dk_bound(inp, w, e_w, u, weighted)
        else:
            e.e_K = e.e_sq
        Wabs = np.abs(w) * (np.abs(_f64(inp.go)) if weighted else 1.0)
        e.e_dK = e.e_dK + gamma(inp.B + 3, u) * abs(inp.grad_scale) * (np.abs(_f64(XM)) * Wabs.sum(1)[:, None] + Wabs @ np.abs(_f64(YM)))
    return e


def float_margin(inp, path):
    """0.25 / max(e_sq): how many bounds the smallest possible channel term of a float-form sq is worth (no metric)"""
    assert inp.form == "float" and not inp.metric
    assert np.abs(inp.X).min() >= 1.0 and np.abs(inp.Y).max() <= 0.5  # |x - y| >= 0.5 in every channel of every pair
    e_sq = sq_bound_fused(inp) if path == "fused" else sq_bound_direct(inp)
    return 0.25 / float(e_sq.max())


def function_error_ulps(got_K, sq, kind, hh, u=U32):
    """the measurement behind F_ULPS: on an exact sq (integer form), the largest error of K beyond the derived part (the
    rounding of 1 + t for imq; nothing for gaussian), in ulps of K"""
    K, _ = kernel_reference(sq, kind, hh)
    e_K, _ = kernel_bounds(sq, np.zeros_like(_f64(sq)), kind, hh, u, 0)
    over = np.maximum(np.abs(_f64(got_K) - K) - e_K, 0.0)
    return float((over / (2 * u * K)).max())


# ---- the assertion ---------------------------------------------------------------------------------------------------------
def assert_vec(got, ref, bound, where, what="K", per=1, stage=FC):
    """Asserts |got - ref| <= bound on EVERY entry; prints the largest error / bound first and names the worst entry with its
    row tile and, for sq / K [A, B], its column tile and split (`per` tiles each), for dK [A, D] its channel stage (of `stage`
    channels).  A zero bound demands equality.  -> the largest error / bound (0 where all are exact)."""
    got, ref, bound = _f64(got), _f64(ref), _f64(bound)
    assert got.shape == ref.shape == bound.shape, (where, got.shape, ref.shape, bound.shape)
    assert np.isfinite(got).all(), (where, what, "not finite")
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, np.where(bound > 0, err / bound, np.inf), 0.0)
    i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    worst = float(ratio[i, j])
    if what == "dK":
        place = f"row tile {i // FM}, channel stage {j // stage}, channel {j % stage} of the stage"
    else:
        place = f"row tile {i // FM}, column tile {j // FN}, column {j % FN} of the tile, split {(j // FN) // per}"
    print(f"{where} {what} {got.shape}: largest error / bound = {worst:.3f} at [{i}, {j}] ({place}); max |error| {err.max():.3e}")
    bad = err > bound
    assert not bad.any(), (where, what, got.shape, f"{int(bad.sum())} entries beyond their bound; worst [{i}, {j}] ({place}): "
                           f"got {got[i, j]!r}, reference {ref[i, j]!r}, bound {bound[i, j]:.3e}")
    return worst


# ---- the kernels' order of operations in fp32 numpy, and their mutations ---------------------------------------------------------
FUSED_MUTATIONS = ("last_channel_dropped", "last_partner_dropped", "stale_last_S_stage", "stale_b_from_previous_tile",
                   "a_reaccumulated_on_second_tile", "centre_not_subtracted_in_tail_stage", "last_split_left_out_of_join",
                   "tail_column_of_K_from_its_neighbour", "xm_uncentred_in_epilogue")
KGRAD_MUTATIONS = ("last_partner_dropped", "tail_channel_from_its_neighbour", "last_row_xm_from_its_neighbour",
                   "grad_out_ignored_in_last_stage")


def fused_applies(mutation, A, B, D, metric=False, grad=True):
    """whether the mistake can happen at the shape: a stale stage needs two stages, a stale b_j or a second a_i two tiles in
    one workgroup, a join two splits, a neighbour has to exist"""
    g = fused_geometry(A, B, grad)
    return {"stale_last_S_stage": D > (FK_METRIC if metric else FK_PLAIN),
            "stale_b_from_previous_tile": g["per"] > 1, "a_reaccumulated_on_second_tile": g["per"] > 1,
            "last_split_left_out_of_join": grad and g["splits"] > 1, "tail_column_of_K_from_its_neighbour": B > 1,
            "xm_uncentred_in_epilogue": grad}.get(mutation, True)


def kgrad_applies(mutation, A, B, D):
    return {"tail_channel_from_its_neighbour": D > 1, "last_row_xm_from_its_neighbour": A > 1}.get(mutation, True)


def _fma32(a, b, c):
    """fl32(a * b + c) on fp32 arrays (the product of two fp32 numbers is exact in fp64; the double rounding differs from a
    fused multiply-add in rare last bits, which no bound depends on)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _fn32(kind, sq, hh):
    """f_kernel_fn / kernel_fn in the arithmetic type of `sq`"""
    T = sq.dtype.type
    if kind == "unit":
        return sq, np.ones_like(sq)
    if kind == "gaussian":
        k = np.exp(-T(hh) * sq)
        return k, k
    den = T(1) + T(hh) * sq
    k = T(1) / np.sqrt(den)
    return k, k / den


def _norm(p, q, FK):
    """sum_c p q of each row as the kernel forms it: eight threads a row, each a sequential fused chain over its FK / 8
    consecutive channels of every stage, then the three shuffle steps"""
    n, Dp = p.shape
    SE = FK // 8
    p, q = p.reshape(n, Dp // FK, 8, SE), q.reshape(n, Dp // FK, 8, SE)
    acc = np.zeros((n, 8), np.float32)
    for st in range(Dp // FK):
        for u in range(SE):
            acc = _fma32(p[:, st, :, u], q[:, st, :, u], acc)
    for width in (1, 2, 4):  # lane ^ width: both lanes of a pair end with the same sum
        acc = acc + acc.reshape(n, 8 // (2 * width), 2, width)[:, :, ::-1, :].reshape(n, 8)
    return acc[:, 0]


def fused_order(inp, kind, hh, grad=True, mutation=None):
    """vec_fused_kernel and vec_join_kernel restated in fp32 numpy -> (K [rows, B], dK [rows, D] or None): centring, 64-wide
    column tiles, S over stages of 64 (plain) or 32 (metric) zero-padded channels (each stage one fp32 matrix product), a_i
    from the first tile of a workgroup, b_j from every tile, sq = max(a + b - cross, 0), W = go w, O in stages of 64 channels,
    dK = s (xm~ wsum - O) per split, the partials joined in split order.  The split geometry is that of `inp.launch_A` rows.
    `mutation`: one of FUSED_MUTATIONS, the same with one mistake."""
    assert mutation is None or (mutation in FUSED_MUTATIONS and fused_applies(mutation, inp.launch_A, inp.B, inp.D, inp.metric, grad))
    f32 = np.float32
    A, B, D, metric = inp.A, inp.B, inp.D, inp.metric
    R = np.arange(A)
    g = fused_geometry(inp.launch_A, B, grad)
    per, splits, ntile = g["per"], g["splits"], g["ntile"]
    FK = FK_METRIC if metric else FK_PLAIN
    nst = -(-D // FK)
    XMm, YMm = inp.grad_operands()
    cy, cym = inp.Y[0], YMm[0]

    def staged(P, c):  # centred, zero beyond D
        out = np.zeros((P.shape[0], nst * FK), f32)
        out[:, :D] = P - c
        return out

    xm_t, y_t = staged(XMm[R], cym), staged(inp.Y, cy)
    x_t, ym_t = (staged(inp.X[R], cy), staged(YMm, cym)) if metric else (xm_t, y_t)
    if mutation == "centre_not_subtracted_in_tail_stage":  # the row side of the last stage is staged as fetched
        k0 = (nst - 1) * FK
        xm_t = xm_t.copy()
        xm_t[:, k0:D] = XMm[R][:, k0:]
        x_t = xm_t
        if metric:
            x_t = staged(inp.X[R], cy)
            x_t[:, k0:D] = inp.X[R][:, k0:]
    tiles4 = [xm_t, y_t] + ([x_t, ym_t] if metric else [])
    if mutation == "last_channel_dropped":
        for t in tiles4:
            t[:, D - 1] = 0
    if mutation == "stale_last_S_stage":  # the LDS buffers still hold the stage before
        for t in tiles4:
            t[:, -FK:] = t[:, -2 * FK:-FK].copy()
    if not metric:
        x_t, ym_t = xm_t, y_t
    ym_o = (YMm - cym).astype(f32)  # the O stages centre their own fetch
    a = _norm(xm_t, x_t, FK)
    go = inp.go[R]
    K = np.zeros((len(R), B), f32)
    part = np.zeros((splits, len(R), D), f32)
    for sp in range(splits):
        wsum, O, b_prev = np.zeros(len(R), f32), np.zeros((len(R), D), f32), None
        for ti, tile in enumerate(range(sp * per, min(ntile, (sp + 1) * per))):
            c0, c1 = tile * FN, min(B, tile * FN + FN)
            b = _norm(ym_t[c0:c1], y_t[c0:c1], FK)
            b_use = b_prev[:c1 - c0] if mutation == "stale_b_from_previous_tile" and ti > 0 else b
            a_use = a * f32(ti + 1) if mutation == "a_reaccumulated_on_second_tile" else a
            b_prev = b
            S = np.zeros((len(R), c1 - c0), f32)
            for st in range(nst):
                k = slice(st * FK, (st + 1) * FK)
                S = S + xm_t[:, k] @ y_t[c0:c1, k].T
                if metric:
                    S = S + x_t[:, k] @ ym_t[c0:c1, k].T
            cross = S if metric else f32(2) * S
            sq = np.maximum((a_use[:, None] + b_use[None, :]) - cross, f32(0))
            k_, w_ = _fn32(kind, sq, hh)
            w_ = w_ * go[:, c0:c1]
            if mutation == "last_partner_dropped" and c1 == B:  # the guard gj < B off by one
                k_, w_ = k_.copy(), w_.copy()
                k_[:, -1], w_[:, -1] = 0, 0
            K[:, c0:c1] = k_
            if grad:
                wsum = wsum + w_.sum(1, dtype=f32)
                for n0 in range(0, D, FC):
                    O[:, n0:n0 + FC] = O[:, n0:n0 + FC] + w_ @ ym_o[c0:c1, n0:n0 + FC]
        xm_e = XMm[R] if mutation == "xm_uncentred_in_epilogue" else (XMm[R] - cym).astype(f32)
        part[sp] = f32(inp.grad_scale) * (xm_e * wsum[:, None] - O)
    if mutation == "tail_column_of_K_from_its_neighbour":
        K[:, B - 1] = K[:, B - 2]
    if not grad:
        return K, None
    dK = np.zeros((len(R), D), f32)
    for sp in range(splits - (mutation == "last_split_left_out_of_join")):
        dK = dK + part[sp]
    return K, dK


def kgrad_order(sq, inp, kind, hh, mutation=None):
    """vec_kgrad_kernel restated in the arithmetic type of `sq` -> (K, dK): partners in stages of 64, weights W = go w(sq),
    acc += W (xm - ym) one partner after the other, dK = s acc.  `mutation`: one of KGRAD_MUTATIONS."""
    assert mutation is None or (mutation in KGRAD_MUTATIONS and kgrad_applies(mutation, inp.A, inp.B, inp.D))
    T = sq.dtype.type
    XM, YM = (a.astype(sq.dtype) for a in inp.grad_operands())
    A, B, D = inp.A, inp.B, inp.D
    if mutation == "last_row_xm_from_its_neighbour":
        XM = XM.copy()
        XM[-1] = XM[-2]
    K, acc = np.zeros((A, B), sq.dtype), np.zeros((A, D), sq.dtype)
    last_stage = ((B - 1) // GJ) * GJ
    for j in range(B):
        k, w = _fn32(kind, sq[:, j], hh)
        K[:, j] = k
        if not (mutation == "grad_out_ignored_in_last_stage" and j >= last_stage):
            w = w * inp.go[:, j].astype(sq.dtype)
        if mutation == "last_partner_dropped" and j == B - 1:
            continue
        acc = acc + w[:, None] * (XM - YM[j][None, :])
    dK = T(inp.grad_scale) * acc
    if mutation == "tail_channel_from_its_neighbour":
        dK[:, D - 1] = dK[:, D - 2]
    return K, dK
