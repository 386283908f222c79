"""What the tests of the velocity kernel share (`svgd_phi_kernel`, csrc/svgd_phi.hip: v = -((K @ score - grad_k)/N) on the fp32
MFMA; tests/test_gpu_phi.py on the device, tests/test_phi_reference_cpu.py for the checker itself): inputs in two forms, the
fp64 reference, a PER-ENTRY bound that is derived and not measured, the assertion, and a numpy restatement of the kernel's
order of operations with the mistakes a kernel of this shape can make.  Not a test module.

The kernel's constants (svgd_phi.hip): a workgroup owns PM = 32 rows by PN = 64 columns of v; k runs in stages of PK = 64,
each split into four quarters of 16 (one per wavefront, MFMA steps of 4); the next stage is fetched while the current one is
multiplied; K and score are fetched 16 bytes at a time where N % 4 == 0 / D % 4 == 0 and the pointer is 16-byte aligned, one
float at a time otherwise.

Inputs (`phi_inputs`):
  integer  K in 1..3, score non-zero in -4..4, grad_k in -8..8.  Every partial sum is an integer of magnitude at most
           12 N + 8 < 2^24 for N <= 1024, so every fp32 product and sum is exact whatever the order, and K @ score - grad_k
           reaches the epilogue exact.  What is left are the two roundings of the epilogue.  Zero references occur by exact
           cancellation.
  float    K uniform in [0.2, 1], score and grad_k = +-uniform[0.5, 1.5] (as `parity.signed_weights`): every term of every
           dot product is at least 0.1 in magnitude, so a term lost, doubled or taken from a neighbour moves the entry by
           at least 0.1/N, far above the bound (`float_margin`).

Bound (`phi_bound`), u = 2^-24 the unit roundoff of fp32 round-to-nearest:
  float    gamma(N + 3) * (|K| @ |score| + |grad_k|) / N, gamma(n) = n u / (1 - n u)  (Higham, Accuracy and Stability of
           Numerical Algorithms, Lemma 3.1).  A term K_ik s_kj passes through at most N roundings: its product (none where the
           product is fused into the sum) and the additions whose operands are both non-zero -- at most N - 1 of them for N
           terms in any order, since adding the zero padding of a partial stage, or a zero accumulator, is exact.  Three more
           come from the subtraction of grad_k, fl(1/N) and the final product.  grad_k passes through those three only.  The
           bound holds for any order of summation, fused or not.
  integer  2 u (1 + u) |ref|: the sum is exact, fl(1/N) = (1/N)(1 + d1) and the product (1 + d2), |d| <= u, so the
           error is at most (2 u + u^2) |ref|.  Where ref == 0 the bound is 0 and the result must be a zero (of either
           sign).  For N a power of two fl(1/N) is exact and so is the product: the bound is 0 everywhere and the result
           must equal the reference, which fp32 then holds exactly.
  mask     a 0/1 mask multiplies exactly and scales the bound; a fractional one adds one rounding of |ref * mask|."""
import numpy as np

U = 2.0 ** -24
PM, PN, PK = 32, 64, 64
FORMS = ("integer", "float")
SEED = 7
# (N, D) of the product tests, on the device and of `kernel_order` here; tests/test_gpu_phi.py says which edge each is for
SHAPES = [(1, 1), (3, 3), (4, 4), (5, 3), (15, 1), (16, 64), (17, 65), (31, 4), (32, 128), (33, 70), (63, 63), (64, 64),
          (65, 63), (65, 65), (68, 68), (68, 132), (100, 132), (127, 3), (128, 128), (128, 132), (129, 63), (132, 4),
          (132, 68), (196, 70), (260, 132)]
BENCH_SHAPE = (1024, 448)  # the benchmark's: integer form only (the float inputs' margin is set for N <= 260)


def gamma(n):
    return n * U / (1.0 - n * U)


def phi_inputs(N, D, seed, form):
    """-> (K [N, N], score, grad_k, mask (zeros and ones), X, each [N, D]) as fp32 numpy arrays, from `seed`"""
    rng = np.random.default_rng([seed, N, D, FORMS.index(form)])
    while True:
        if form == "integer":
            K = rng.integers(1, 4, (N, N))
            s = rng.integers(1, 5, (N, D)) * rng.choice([-1, 1], (N, D))
            gk = rng.integers(-8, 9, (N, D))
        else:
            K = rng.uniform(0.2, 1.0, (N, N))
            s = rng.choice([-1.0, 1.0], (N, D)) * rng.uniform(0.5, 1.5, (N, D))
            gk = rng.choice([-1.0, 1.0], (N, D)) * rng.uniform(0.5, 1.5, (N, D))
        # the last two rows of K and the last two columns of score differ (a small integer draw can repeat one; drawn again
        # then), so a result row or column taken from its neighbour is a different one
        if (N == 1 or (K[-1] != K[-2]).any()) and (D == 1 or (s[:, -1] != s[:, -2]).any()):
            break
    mask = (rng.uniform(size=(N, D)) > 0.3).astype(np.float32)
    X = rng.standard_normal((N, D))
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (K, s, gk, mask, X))


def _f64(a):
    return np.asarray(a, np.float64)


def phi_reference(K, s, gk):
    """-((K @ s - gk)/N) in fp64"""
    K = _f64(K)
    return -((K @ _f64(s) - _f64(gk)) / K.shape[0])


def phi_bound(K, s, gk, form):
    """the per-entry bound of the module docstring, fp64 [N, D]"""
    N = np.shape(K)[0]
    if form == "integer":
        assert 12 * N + 8 < 2 ** 24
        if N & (N - 1) == 0:
            return np.zeros(np.shape(s))
        return 2 * U * (1 + U) * np.abs(phi_reference(K, s, gk))
    assert form == "float"
    return gamma(N + 3) * (np.abs(_f64(K)) @ np.abs(_f64(s)) + np.abs(_f64(gk))) / N


def float_margin(K, s, gk):
    """(0.1/N) / max(bound) of float-form inputs: how many bounds the smallest possible term of a dot product is worth"""
    N = np.shape(K)[0]
    assert np.abs(K).min() >= 0.2 and np.abs(s).min() >= 0.5
    return (0.1 / N) / float(phi_bound(K, s, gk, "float").max())


def assert_phi(v, K, s, gk, form, where, mask=None):
    """Asserts |v - reference| <= bound on EVERY entry; prints the largest error / bound first and names the worst entry with
    its tile, its column within the tile and the number of k stages.  -> the largest error / bound (0 where all are exact)."""
    N, D = np.shape(s)
    ref, bound = phi_reference(K, s, gk), phi_bound(K, s, gk, form)
    if mask is not None:
        m = np.abs(_f64(mask))
        fractional = bool(((m != 0) & (m != 1)).any())
        ref = ref * _f64(mask)
        bound = bound * m * (1 + U) + U * np.abs(ref) if fractional else bound * m
    v = _f64(v).reshape(N, D)
    assert np.isfinite(v).all(), (where, "not finite")
    err = np.abs(v - ref)
    ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    worst = float(ratio[i, j])
    stages = -(-N // PK)
    print(f"{where} ({N}, {D}) {form}: largest error / bound = {worst:.3f} at [{i}, {j}] (tile row {i // PM} col {j // PN}, "
          f"column {j % PN} of the tile, {stages} k stage{'s' * (stages > 1)}, last of {N - (stages - 1) * PK}); "
          f"max |error| {err.max():.3e}, zero references {int((ref == 0).sum())}")
    assert (err <= bound).all(), (where, (N, D), form, f"{int((err > bound).sum())} entries beyond their bound; worst "
                                  f"[{i}, {j}]: got {v[i, j]!r}, reference {ref[i, j]!r}, bound {bound[i, j]:.3e}")
    return worst


# ---- the kernel's order of operations in numpy, and its mutations -------------------------------------------------------------
MUTATIONS = ("last_k_dropped", "quarter_dropped_in_last_stage", "stale_last_stage", "last_column_from_its_neighbour",
             "last_row_from_its_neighbour", "tail_fetch_shifted", "one_over_N_plus_one")


def applies(mutation, N, D):
    """whether the mistake can happen at the shape: a stale stage needs a prefetch (two stages), a neighbour needs to exist"""
    return {"stale_last_stage": N > PK, "last_column_from_its_neighbour": D > 1, "last_row_from_its_neighbour": N > 1}.get(
        mutation, True)


def _fma32(a, b, c):
    """fl32(a * b + c) on fp32 arrays: the product of two fp32 numbers is exact in fp64, the sum is rounded to fp64 and then
    to fp32 (the double rounding differs from a fused multiply-add in rare last bits, which the bound does not depend on)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def kernel_order(K, s, gk, mutation=None):
    """svgd_phi_kernel's arithmetic restated in fp32 numpy: zero-padded 64-deep stages, four k quarters of 16, one sequential
    fp32 chain per quarter (running across the stages), ((q0 + q1) + q2) + q3, then -((sv - gv) * fl(1/N)).  `mutation`: one
    of MUTATIONS, the same with one mistake."""
    assert mutation is None or mutation in MUTATIONS
    K, s, gk = (np.asarray(a, np.float32) for a in (K, s, gk))
    N, D = s.shape
    stages = -(-N // PK)
    Kp = np.zeros((N, stages * PK), np.float32)
    Sp = np.zeros((stages * PK, D), np.float32)
    Kp[:, :N], Sp[:N] = K, s
    if mutation == "last_k_dropped":
        Kp[:, N - 1] = 0
    if mutation == "last_row_from_its_neighbour":
        Kp[N - 1] = Kp[N - 2]
    if mutation == "last_column_from_its_neighbour":
        Sp[:, D - 1] = Sp[:, D - 2]
    if mutation == "tail_fetch_shifted":  # the last group of four k reads one float further on (the next row's start; zero
        flat = np.append(K.reshape(-1), np.float32(0))  # behind the matrix)
        for k in range(4 * ((N - 1) // 4), N):
            Kp[:, k] = flat[np.arange(N) * N + k + 1]
    if mutation == "stale_last_stage":  # the registers still hold the stage before
        Kp[:, -PK:], Sp[-PK:] = Kp[:, -2 * PK:-PK].copy(), Sp[-2 * PK:-PK].copy()
    acc = np.zeros((4, N, D), np.float32)
    for st in range(stages):
        for t in range(PK // 4):
            k = st * PK + np.arange(4) * (PK // 4) + t  # the k of each quarter at this position of its chain
            a, b = Kp[:, k].T[:, :, None], Sp[k][:, None, :]
            new = _fma32(np.broadcast_to(a, acc.shape), np.broadcast_to(b, acc.shape), acc)
            if mutation == "quarter_dropped_in_last_stage" and st == stages - 1:
                new[0] = acc[0]
            acc = new
    sv = ((acc[0] + acc[1]) + acc[2]) + acc[3]
    inv = np.float32(1.0) / np.float32(N + 1 if mutation == "one_over_N_plus_one" else N)
    return -((sv - gk) * inv)
