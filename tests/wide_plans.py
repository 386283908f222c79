"""The launch plan of the register-resident kernel's 32-channel layout (csrc/gram_fast_wide.hip: RBF paths of 17 to 32
channels with SIGSVGD_FLAG_FP32_SWEEPS), restated next to its tests -- `plans.gram_geometry` describes the
unflagged routes, which send d > 16 to the coverage kernel.  tests/test_wide_cabi.py pins it to the library's workspace query."""

ROWS = 4  # rows per tile: 4-wave workgroups, one row per wavefront (`grad_nw` for d > 8)
PER_CU = 1  # workgroups a compute unit holds: one wave per SIMD, 121 KB of LDS


def _r256(b):
    return (b + 255) & ~255


def wide_shape(T, d, n=0):
    """`fast_wide_supported`"""
    return n == 0 and 3 <= T <= 64 and 17 <= d <= 32


def wide_geometry(A, B, sym, cus=256):
    """(rows per tile, items, grid) of a launch: `grad_geometry` (csrc/sweep_host.hip) at 4-row tiles and one workgroup per
    compute unit; the forward-only launches have the same split.  sym: the Y_IS_X orientation (A == B, each unordered pair once)"""
    ntile = -(-A // ROWS)
    items = sum(B - t * ROWS for t in range(ntile)) if sym else ntile * B
    return dict(rows_per_tile=ROWS, items=items, grid=min(items, cus * PER_CU), ntile=ntile)


def wide_bytes(A, B, T, d, want_grad, sym, cus=256):
    """What sigsvgd_gram_workspace_bytes reports for a query that covers this one launch (A != B, or Y_IS_X): no flag area;
    gradient launches the fp64 row segments of (tiles + grid) * 4 paths and, symmetric ones, the fp32 column slab of one path
    per item; 256 bytes of alignment slack."""
    assert wide_shape(T, d)
    if not want_grad:
        return 256
    g = wide_geometry(A, B, sym, cus)
    rseg = _r256((g["ntile"] + g["grid"]) * ROWS * T * d * 8)
    cslab = _r256(g["items"] * T * d * 4) if sym else 0
    return rseg + cslab + 256


# ---- inputs and the C oracle's answers, shared by tests/test_wide_cabi.py and tests/test_gpu_wide.py ----------------------------
import functools  # noqa: E402

H = 1.0


@functools.lru_cache(maxsize=None)
def inputs(A, T, d, seed):
    """`parity.walks(A, T, d, seed, 0.05)`: the smooth regime of the order-0 parity files; callers leave it unchanged"""
    from parity import walks

    return walks(A, T, d, seed, 0.05)


@functools.lru_cache(maxsize=None)
def weights(A, B):
    from parity import signed_weights

    return signed_weights(A, B, 11)


@functools.lru_cache(maxsize=None)
def reference(A, B, T, d, weighted=True, yseed=5):
    """(K, gX, gY) of the C oracle for X = inputs(A, T, d, 0), Y = inputs(B, T, d, yseed) (yseed 0: Y is X) with h = 1: gX the
    first-slot gradient of sum(w K), gY the second-slot one (the first slot of the transposed problem); computed once per shape"""
    from oracle import c_oracle

    X, Y = inputs(A, T, d, 0), inputs(B, T, d, yseed)
    w = weights(A, B) if weighted else None
    K, gX = c_oracle.gram_fwd_bwd(X, Y, h=H, grad_out=w)
    _, gY = c_oracle.gram_fwd_bwd(Y, X, h=H, grad_out=None if w is None else w.T)
    return K, gX, gY
