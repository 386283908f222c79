"""Host-side checks of the two-sided long-path Gram entry points (`sigsvgd_gram_long2_workspace_bytes`,
`sigsvgd_gram_long_fwd_bwd2`, include/sigsvgd_hip.h): exports, argument checks, the launch plan and
its slab bound, and the identity the GPU tests take their second-slot reference from.  No device needed (every call below
returns before any device work)."""
import ctypes

import numpy as np
import pytest

from cabi import assert_exported, BADARG, FAKE, lib, UNSUPPORTED
from plans import device_cus, long2_plan, long_plan, pair_plan
from sigsvgd_amd import _lib, ops

NAMES = ("sigsvgd_gram_long2_workspace_bytes", "sigsvgd_gram_long_fwd_bwd2")
# the launch modes: (want_gradX, want_gradY, flags)
MODES = {"two-slot": (1, 1, 0), "x-only": (1, 0, 0), "y-only": (0, 1, 0), "yx": (1, 0, _lib.FLAG_Y_IS_X),
         "yx-forward": (0, 0, _lib.FLAG_Y_IS_X)}


def long2_ws(A, B, TX, TY, d, n, kind=_lib.STATIC_RBF, want_x=1, want_y=1, flags=0, out=True):
    b = ctypes.c_size_t(12345)
    rc = lib().sigsvgd_gram_long2_workspace_bytes(A, B, TX, TY, d, n, kind, want_x, want_y, flags,
                                                  ctypes.byref(b) if out else None)
    return rc, b.value


def test_long2_symbols_exported():
    assert_exported(NAMES, abi=10)


def _launch(a, gX=FAKE, gY=FAKE, X=FAKE, K=FAKE, dtype=_lib.F32, inv_h=1.0):
    return lib().sigsvgd_gram_long_fwd_bwd2(X, FAKE, a["A"], a["B"], a["TX"], a["TY"], a["d"], dtype, inv_h, a["n"], a["kind"],
                                            a["flags"], None, K, gX, gY, FAKE, 1 << 30, None)


@pytest.mark.parametrize("case", ["A<1", "B<1", "TX<2", "TY<2", "d<1", "kind", "order", "force_generic", "unknown_flag",
                                  "sym_AB", "sym_T", "yx_AB", "yx_T"])
def test_long2_bad_shapes_and_flags(case):
    args = dict(A=3, B=3, TX=300, TY=300, d=2, n=0, kind=_lib.STATIC_RBF, flags=0)
    upd = {"A<1": dict(A=0), "B<1": dict(B=0), "TX<2": dict(TX=1), "TY<2": dict(TY=1), "d<1": dict(d=0), "kind": dict(kind=5),
           "order": dict(n=11), "force_generic": dict(flags=_lib.FLAG_FORCE_GENERIC), "unknown_flag": dict(flags=_lib.FLAG_WS_CLEAN),
           "sym_AB": dict(B=4, flags=_lib.FLAG_SYM), "sym_T": dict(TY=200, flags=_lib.FLAG_SYM),
           "yx_AB": dict(B=4, flags=_lib.FLAG_Y_IS_X), "yx_T": dict(TY=200, flags=_lib.FLAG_Y_IS_X)}[case]
    a = {**args, **upd}
    rc, _ = long2_ws(a["A"], a["B"], a["TX"], a["TY"], a["d"], a["n"], a["kind"], 1, 0, a["flags"])
    assert rc == BADARG, _lib.last_error()
    assert _launch(a, gY=None) == BADARG, _lib.last_error()


def test_long2_gradY_needs_two_slots():
    """Y_IS_X and SYM weight one slot: a gradY output with either is refused, in the query and in the launch."""
    a = dict(A=3, B=3, TX=300, TY=300, d=2, n=0, kind=_lib.STATIC_RBF, flags=0)
    for f in (_lib.FLAG_Y_IS_X, _lib.FLAG_SYM, _lib.FLAG_Y_IS_X | _lib.FLAG_SYM):
        assert long2_ws(3, 3, 300, 300, 2, 0, want_x=1, want_y=1, flags=f)[0] == BADARG
        assert long2_ws(3, 3, 300, 300, 2, 0, want_x=1, want_y=0, flags=f)[0] == 0, _lib.last_error()
        assert _launch({**a, "flags": f}) == BADARG
        assert _launch({**a, "flags": f}, gX=None) == BADARG


def test_long2_launch_argument_checks():
    a = dict(A=3, B=3, TX=300, TY=300, d=2, n=0, kind=_lib.STATIC_RBF, flags=0)
    assert long2_ws(3, 3, 300, 300, 2, 0, out=False)[0] == BADARG
    assert _launch(a, X=None) == BADARG and _launch(a, K=None) == BADARG  # null pointers
    assert _launch(a, dtype=7) == BADARG
    assert _launch(a, inv_h=0.0) == BADARG  # RBF without a bandwidth
    for f in (_lib.FLAG_NAIVE_SOLVER, _lib.FLAG_Y_IS_X, _lib.FLAG_SYM, _lib.FLAG_SYM | _lib.FLAG_Y_IS_X | _lib.FLAG_NAIVE_SOLVER):
        assert long2_ws(3, 3, 300, 300, 2, 0, want_y=0, flags=f)[0] == 0, _lib.last_error()


def test_long2_refusals_are_the_long_routes():
    assert long2_ws(1, 2, 129, 129, 2, 6)[0] == 0  # P = Q = 8192: the edge is taken
    for (TX, TY, n) in [(8194, 10, 0), (10, 8194, 0), (130, 129, 6)]:
        rc, _ = long2_ws(1, 2, TX, TY, 2, n)
        assert rc == UNSUPPORTED and "8192" in _lib.last_error()
    rc, _ = long2_ws(2, 2, 300, 300, 184, 0)
    assert rc == UNSUPPORTED and "LDS" in _lib.last_error()
    assert ops.gram_long2_takes(2, 2, 300, 300, 183) is True
    assert ops.gram_long2_takes(2, 2, 300, 300, 184) is False
    assert ops.gram_long2_takes(2, 2, 8194, 8194, 2, y_is_x=True, want_gradY=False) is False
    with pytest.raises(RuntimeError):  # a bad argument is an error, not a route
        ops.gram_long2_takes(2, 2, 300, 300, 2, static_kind=9)


def test_long2_plan_mirror_matches_workspace_query():
    """`plans.long2_plan` mirrors long2_make_plan over the shape list of test_long_cabi.py's plan test and every launch mode,
    and refuses exactly where the query does.  (Y-is-X modes need a square launch: there B and TY follow A and TX.)"""
    cus = device_cus()
    shapes = [(1, 1, 2, 2), (3, 4, 300, 300), (1, 2, 129, 129), (2, 3, 129, 130), (2, 2, 257, 258), (2, 2, 513, 514),
              (2, 2, 9, 9), (2, 3, 5, 9), (1, 2, 9, 3), (3, 2, 150, 400), (2, 3, 66, 258), (1, 1, 300, 2), (1, 1, 2, 300),
              (64, 64, 40, 40), (40, 60, 40, 40), (500, 700, 20, 20), (64, 64, 1025, 1025), (16, 16, 2048, 2048)]
    seen = set()
    for (A, B, M, N) in shapes:
        for n in (0, 1, 2, 3, 6, 7, 8, 10):
            for d in (1, 2, 17, 183, 184):
                for mode, (wx, wy, flags) in MODES.items():
                    yx = bool(flags & _lib.FLAG_Y_IS_X)
                    Bm, Nm = (A, M) if yx else (B, N)
                    rc, b = long2_ws(A, Bm, M, Nm, d, n, want_x=wx, want_y=wy, flags=flags)
                    pl = long2_plan(A, Bm, M, Nm, d, n, bool(wx), bool(wy), yx, cus)
                    assert (rc == UNSUPPORTED) == (pl is None), (A, Bm, M, Nm, d, n, mode, rc)
                    if pl is None:
                        continue
                    assert rc == 0 and b == pl["bytes"], (A, Bm, M, Nm, d, n, mode, b, pl)
                    if mode == "yx-forward":
                        assert b == 0
                    seen.add((yx, pl["IC"], pl["JC"]))
    assert {(False, 1, 1), (False, 2, 2), (True, 1, 1), (True, 2, 2)} <= seen, seen
    assert any(ic != jc for (_, ic, jc) in seen)


def test_long2_forward_needs_no_workspace():
    for (A, T, d, n) in [(4, 400, 3, 0), (2, 200, 4, 2), (16, 2048, 2, 0)]:
        assert long2_ws(A, A, T, T, d, n, want_x=0, want_y=0) == (0, 0)
        assert long2_ws(A, A, T, T, d, n, want_x=0, want_y=0, flags=_lib.FLAG_Y_IS_X) == (0, 0)
        rc, b = long2_ws(A, A, T, T, d, n)
        assert rc == 0 and b > 0


def test_long2_slab_bound():
    """Slab memory does not grow like A * B * T * d: at A = B = 256, T = 300, d = 4 it is within the bound of the tiling,
    (A ceil(B / JC) TX + B ceil(A / IC) TY) d 8, and below a quarter of A * B * TX * d * 8, in every mode."""
    A = B = 256
    TX = TY = 300
    d = 4
    for mode, (wx, wy, flags) in MODES.items():
        pl = long2_plan(A, B, TX, TY, d, 0, bool(wx), bool(wy), bool(flags & _lib.FLAG_Y_IS_X), device_cus())
        assert pl["IC"] > 1 and pl["JC"] > 1, pl
        bound = (A * -(-B // pl["JC"]) * TX + B * -(-A // pl["IC"]) * TY) * d * 8
        assert pl["slab_bytes"] <= bound, (mode, pl)
        assert pl["slab_bytes"] < A * B * TX * d * 8 // 4, (mode, pl)
        rc, b = long2_ws(A, B, TX, TY, d, 0, want_x=wx, want_y=wy, flags=flags)
        assert rc == 0 and b == pl["bytes"]


def test_existing_long_and_pair_queries_unchanged():
    cus = device_cus()
    for (A, B, M, N, d, n) in [(3, 4, 300, 300, 3, 0), (2, 2, 200, 200, 4, 2), (40, 60, 40, 40, 2, 0), (64, 64, 1025, 1025, 4, 0),
                               (3, 2, 150, 400, 2, 1)]:
        for want_grad in (0, 1):
            b = ctypes.c_size_t(1)
            assert lib().sigsvgd_gram_long_workspace_bytes(A, B, M, N, d, n, 0, want_grad, 0, ctypes.byref(b)) == 0
            assert b.value == long_plan(A, B, M, N, d, n, want_grad, cus)["bytes"]
            assert lib().sigsvgd_pair_workspace_bytes(A, M, N, d, n, 0, want_grad, 0, ctypes.byref(b)) == 0
            assert b.value == pair_plan(A, M, N, d, n, want_grad, cus)["bytes"]


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [0, 2])
@pytest.mark.parametrize("naive", [False, True])
def test_second_slot_identity_on_the_numpy_oracle(kind, n, naive):
    """The reference of the GPU tests.  The second-slot gradient of sum W * K(X, Y) in the project's convention, written out:
    gY[j][q] = sum_i W[i][j] sum_p R_ij[p][q] dk(x_ip, y_jq)/dy_jq, with R_ij the 4-corner scatter of the pair's coarse S
    (what gram_backward contracts with dk/dx), equals the first slot of the swapped call, gram_backward(Y, X, W^T)."""
    from oracle import sigkernel_oracle as O

    rng = np.random.default_rng(3 + kind + n)
    A, B, T, d, h, r = 3, 4, 6, 2, 0.7, 2**n
    X = np.cumsum(0.4 * rng.standard_normal((A, T, d)), axis=1)
    Y = np.cumsum(0.4 * rng.standard_normal((B, T, d)), axis=1)
    W = rng.uniform(0.5, 1.5, (A, B))
    K_full, g, G = O.gram_forward_full(X, Y, kind, h, n, naive)
    S = O.gg_matrix(K_full, g, naive).reshape(A, B, T - 1, r, T - 1, r).sum(axis=(3, 5)) / float(r * r)
    R = np.zeros((A, B, T, T))
    R[:, :, 1:, 1:] += S
    R[:, :, :-1, :-1] += S
    R[:, :, 1:, :-1] -= S
    R[:, :, :-1, 1:] -= S
    if kind == O.LINEAR:  # dk(x_p, y_q)/dy_q = x_p
        Vy = np.broadcast_to(X[:, None, :, None, :], (A, B, T, T, d))
    else:  # 2/h (x_p - y_q) k
        Vy = (2.0 / h) * (X[:, None, :, None, :] - Y[None, :, None, :, :]) * G[..., None]
    gY = np.einsum("ij,ijpq,ijpqc->jqc", W, R, Vy)
    Kt, gY_ref = O.gram_backward(Y, X, W.T, kind, h, n, naive)
    assert np.abs(gY - gY_ref).max() < 1e-13 * np.abs(gY_ref).max()
    assert np.abs(K_full[..., -1, -1] - Kt.T).max() < 1e-13 * np.abs(Kt).max()
