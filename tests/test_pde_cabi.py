"""Host-side checks of the static-grid PDE entry points (`sigsvgd_pde_*`, include/sigsvgd_hip.h) and of the user
static-kernel route of sigsvgd_amd.sigkernel; no device needed (every call below returns before any device work)."""
import ctypes

import pytest
import torch

from cabi import assert_exported, BADARG, FAKE, lib, UNSUPPORTED
from plans import device_cus, pde_plan
from sigsvgd_amd import _lib

def ws_bytes(npairs, M, N, n, want_grad, flags=0):
    b = ctypes.c_size_t(0)
    rc = lib().sigsvgd_pde_workspace_bytes(npairs, M, N, n, want_grad, flags, ctypes.byref(b))
    return rc, b.value


def test_pde_symbols_exported():
    assert_exported(("sigsvgd_pde_workspace_bytes", "sigsvgd_pde_fwd", "sigsvgd_pde_fwd_bwd"), abi=10)


@pytest.mark.parametrize("case", ["null_G", "null_K", "null_dG", "M<2", "N<2", "npairs<1", "dtype", "flag", "order<0",
                                  "order>10"])
def test_pde_bad_arguments(case):
    L = lib()
    args = dict(G=FAKE, npairs=4, M=5, N=6, dtype=_lib.F64, n=1, flags=0, K=FAKE, dG=FAKE)
    upd = {"null_G": dict(G=None), "null_K": dict(K=None), "null_dG": dict(dG=None), "M<2": dict(M=1), "N<2": dict(N=1),
           "npairs<1": dict(npairs=0), "dtype": dict(dtype=7), "flag": dict(flags=_lib.FLAG_SYM), "order<0": dict(n=-1),
           "order>10": dict(n=11)}[case]
    a = {**args, **upd}
    rc = L.sigsvgd_pde_fwd_bwd(a["G"], a["npairs"], a["M"], a["N"], a["dtype"], a["n"], a["flags"], None, a["K"], a["dG"],
                               FAKE, 1 << 30, None)
    assert rc == BADARG, _lib.last_error()
    if case != "null_dG":
        rc = L.sigsvgd_pde_fwd(a["G"], a["npairs"], a["M"], a["N"], a["dtype"], a["n"], a["flags"], a["K"], FAKE, 1 << 30,
                               None)
        assert rc == BADARG, _lib.last_error()


def test_pde_workspace_query():
    rc, b = ws_bytes(100, 10, 10, 4, 1)
    assert rc == 0 and b > 0
    assert ws_bytes(100, 10, 10, 4, 1, _lib.FLAG_NAIVE_SOLVER) == (0, b)
    assert ws_bytes(100, 10, 10, 4, 1, _lib.FLAG_Y_IS_X)[0] == BADARG
    assert ws_bytes(100, 10, 10, 4, 0) == (0, 0)  # the forward sweep keeps nothing
    # does not shrink as the grid grows
    grow = (2, 3, 10, 33, 64, 65, 100, 129, 200, 257)
    for n in (0, 2):
        for shape in ([(M, M) for M in grow], [(M, 20) for M in grow], [(20, N) for N in grow]):
            sizes = []
            for (M, N) in shape:
                rc, b = ws_bytes(4096, M, N, n, 1)
                assert rc == 0, (M, N, n, _lib.last_error())
                sizes.append(b)
            assert sizes == sorted(sizes), (n, shape, sizes)
    # sized by the resident waves: stops growing with npairs
    sizes = [ws_bytes(k, 30, 30, 2, 1)[1] for k in (1, 10, 100, 10_000, 100_000, 1_000_000)]
    assert sizes == sorted(sizes) and sizes[-1] == sizes[-2] == sizes[-3]
    assert sizes[0] < sizes[-1]


def test_pde_supported_range():
    # upstream's GPU path: P + 1 <= 1023 and Q + 1 <= 1023
    for (M, N, n) in [(1023, 1023, 0), (512, 512, 1), (2, 1023, 0), (1023, 2, 0), (64, 64, 4), (2, 2, 9), (33, 129, 3)]:
        for g in (0, 1):
            rc, _ = ws_bytes(1000, M, N, n, g)
            assert rc == 0, (M, N, n, g, _lib.last_error())
    for (M, N, n) in [(20000, 20000, 0), (2, 20000, 0), (2000, 2000, 3), (10, 10, 10)]:
        rc, _ = ws_bytes(1000, M, N, n, 1)
        assert rc == UNSUPPORTED, (M, N, n)
        assert "B" in _lib.last_error()


class _GramOnly:
    """A static kernel with upstream's Gram_matrix and nothing else (an RBF in disguise)."""

    def Gram_matrix(self, X, Y):
        return torch.exp(-torch.cdist(X.flatten(0, 1), Y.flatten(0, 1)).pow(2).reshape(X.shape[0], X.shape[1], Y.shape[0],
                                                                                       Y.shape[1]).permute(0, 2, 1, 3))


def test_user_static_kernel_routing_on_cpu():
    import sigsvgd_amd.sigkernel as sk

    X = torch.randn(2, 4, 3, dtype=torch.float64)
    with pytest.raises(NotImplementedError):
        sk.SigKernel(object(), 1).compute_Gram(X, X)
    assert sk._resolve_static(_GramOnly(), X, X) == (None, None)
    assert sk._resolve_static(sk.RBFKernel(0.5), X, X) == (_lib.STATIC_RBF, 2.0)
    assert sk._resolve_static(sk.LinearKernel(), X, X)[0] == _lib.STATIC_LINEAR
    k = sk.SigKernel(_GramOnly(), 1)
    for call in (lambda: k.compute_Gram(X, X), lambda: k.compute_kernel(X, X), lambda: k.gram_and_grad(X)):
        with pytest.raises(RuntimeError, match="runs only on a HIP device"):
            call()


def test_plan_helper_matches_workspace_query():
    """tests/plans.pde_plan mirrors pde_make_plan: its bytes are the library's (ring wrap, nrow = 1, more pairs than
    resident waves, the 1 GiB scratch cap)."""
    cus = device_cus()
    for npairs in (1, 2, 100, 2500, 100_000):
        for (M, N) in [(2, 2), (10, 10), (70, 129), (70, 130), (40, 257), (40, 258), (20, 513), (20, 514), (9, 9), (3, 9),
                       (66, 40), (300, 2), (2, 300), (129, 129), (1023, 1023)]:
            for n in (0, 1, 2, 6, 7, 8, 10):
                for want_grad in (0, 1):
                    rc, b = ws_bytes(npairs, M, N, n, want_grad)
                    pl = pde_plan(npairs, M, N, n, want_grad, cus)
                    assert (rc == UNSUPPORTED) == (pl is None), (npairs, M, N, n, want_grad, rc)
                    if pl is not None:
                        assert rc == 0 and b == pl["bytes"], (npairs, M, N, n, want_grad, b, pl)


@pytest.mark.parametrize("n", [7, 8, 9, 10])
def test_high_orders(n):
    """Orders 7 to 10: taken up to P = Q = 8192 (nrow = 1), refused past it."""
    edge = 8192 // (1 << n) + 1
    for (M, N) in [(edge, edge), (edge, 3), (3, edge), (2, 2)]:
        for want_grad in (0, 1):
            assert ws_bytes(2, M, N, n, want_grad)[0] == 0, _lib.last_error()
    for (M, N) in [(edge + 1, edge), (edge, edge + 1), (2, edge + 1)]:
        rc, _ = ws_bytes(2, M, N, n, 1)
        assert rc == UNSUPPORTED and "8192" in _lib.last_error()
