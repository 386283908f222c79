"""Host-side checks of the distance select (`sigsvgd_sqdist_select*`, include/sigsvgd_hip.h), of `utils.math.bw_from_median`
and of the routing of data-dependent bandwidths in `sigkernel.inv_bandwidth_from_fn`; no device needed (every library call
below returns before any device work, and the routing tests run on an oracle-backed double of the op)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from cabi import assert_exported, BADARG, FAKE, lib, WORKSPACE
from helpers import golden
from oracle import sigkernel_oracle as O
from sigsvgd_amd import _lib, ops
from sigsvgd_amd.utils.math import bw_from_median, bw_median

NAMES = ("sigsvgd_sqdist_select_workspace_bytes", "sigsvgd_sqdist_select")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def select_ws(A, B, TX, TY, d, flags=0, out=True):
    b = ctypes.c_size_t(12345)
    rc = lib().sigsvgd_sqdist_select_workspace_bytes(A, B, TX, TY, d, flags, ctypes.byref(b) if out else None)
    return rc, b.value


def select(A=3, B=4, TX=5, TY=6, d=2, dtype=_lib.F32, flags=0, rank=0, X=FAKE, Y=FAKE, out=FAKE, ws=FAKE, ws_bytes=1 << 30):
    return lib().sigsvgd_sqdist_select(X, Y, A, B, TX, TY, d, dtype, flags, rank, out, ws, ws_bytes, None)


def test_select_symbols_exported():
    assert_exported(NAMES, abi=10)
    header = open(os.path.join(ROOT, "include", "sigsvgd_hip.h")).read()
    declared = re.findall(r"\b(sigsvgd_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    for name in NAMES:
        assert declared.count(name) == 1
    assert int(re.search(r"#define SIGSVGD_ABI_VERSION (\d+)", header).group(1)) == 10


@pytest.mark.parametrize("case", ["A<1", "B<1", "TX<1", "TY<1", "d<1", "sym", "naive", "generic", "unknown_bit",
                                  "yx_A!=B", "yx_TX!=TY", "n>=2^63"])
def test_select_bad_shapes_and_flags(case):
    big = 2**31 - 1
    upd = {"A<1": dict(A=0), "B<1": dict(B=-1), "TX<1": dict(TX=0), "TY<1": dict(TY=0), "d<1": dict(d=0),
           "sym": dict(flags=_lib.FLAG_SYM), "naive": dict(flags=_lib.FLAG_NAIVE_SOLVER),
           "generic": dict(flags=_lib.FLAG_FORCE_GENERIC | _lib.FLAG_Y_IS_X, A=4, TX=6), "unknown_bit": dict(flags=1 << 20),
           "yx_A!=B": dict(flags=_lib.FLAG_Y_IS_X, TX=6), "yx_TX!=TY": dict(flags=_lib.FLAG_Y_IS_X, A=4),
           "n>=2^63": dict(A=big, B=big, TX=big, TY=big)}[case]
    a = {**dict(A=3, B=4, TX=5, TY=6, d=2, flags=0), **upd}
    rc, _ = select_ws(a["A"], a["B"], a["TX"], a["TY"], a["d"], a["flags"])
    assert rc == BADARG, _lib.last_error()
    assert select(**a) == BADARG, _lib.last_error()


def test_select_launch_argument_checks():
    assert select_ws(3, 4, 5, 6, 2, out=False)[0] == BADARG
    assert select(X=None) == BADARG
    assert select(Y=None) == BADARG
    assert select(out=None) == BADARG
    assert select(dtype=7) == BADARG
    n = 3 * 4 * 5 * 6
    assert select(rank=n) == BADARG and "rank" in _lib.last_error()
    assert select(rank=2**64 - 1) == BADARG
    # the largest count taken: n = 2^62 (< 2^63); a rank at n is refused, and a workspace too small is E_WORKSPACE -- all
    # of it before any device work (the pointers are fake)
    two31 = dict(A=2**15, B=2**15, TX=2**16, TY=2**16)
    assert select_ws(2**15, 2**15, 2**16, 2**16, 2)[0] == 0, _lib.last_error()
    assert select(**two31, rank=2**62) == BADARG
    rc, need = select_ws(3, 4, 5, 6, 2)
    assert rc == 0 and need > 0
    assert select(ws_bytes=need - 1) == WORKSPACE and str(need) in _lib.last_error()
    assert select(ws=None, ws_bytes=0) == WORKSPACE
    assert select(**two31, rank=2**62 - 1, ws_bytes=need - 1) == WORKSPACE
    # Y_IS_X with one shape in both slots is taken
    assert select_ws(4, 4, 5, 5, 2, _lib.FLAG_Y_IS_X)[0] == 0, _lib.last_error()


def test_select_workspace_does_not_grow_with_the_problem():
    sizes = set()
    for (A, B, TX, TY, d) in [(1, 1, 1, 1, 1), (5, 7, 9, 4, 3), (1024, 1024, 64, 64, 7), (1024, 1024, 64, 128, 2),
                              (16, 16, 2000, 2000, 2), (2**15, 2**15, 2**16, 2**16, 300)]:
        for flags in (0, _lib.FLAG_Y_IS_X) if (A == B and TX == TY) else (0,):
            rc, b = select_ws(A, B, TX, TY, d, flags)
            assert rc == 0 and b > 0, _lib.last_error()
            sizes.add(b)
    assert max(sizes) <= 16 << 20 and max(sizes) == min(sizes)  # one constant size


def test_bw_from_median_reproduces_the_fixture():
    G = golden()
    sq = torch.as_tensor(G["bw_in"])
    med = torch.median(sq)
    assert float(bw_from_median(med, sq.shape[0])) == pytest.approx(float(G["bw_out"]), rel=1e-14)
    assert float(bw_from_median(med, sq.shape[0], bw_scale=2.0)) == pytest.approx(float(G["bw_out_scale2"]), rel=1e-14)
    # bw_median is its own tail on the median: the same bits, and unchanged on the fixture
    assert float(bw_median(sq)) == float(bw_from_median(med, sq.shape[0]))
    assert float(bw_median(sq, 2.0, 1e-3)) == float(bw_from_median(med, sq.shape[0], 2.0, 1e-3))
    assert float(bw_median(sq)) == pytest.approx(float(G["bw_out"]), rel=1e-14)
    assert float(bw_median(sq, bw_scale=2.0)) == pytest.approx(float(G["bw_out_scale2"]), rel=1e-14)
    assert float(bw_from_median(torch.tensor(0.0, dtype=torch.float64), 5, tol=1e-3)) == 1e-3  # the clamp


def test_median_route_predicate():
    import sigsvgd_amd.sigkernel as sk

    assert sk._median_route(bw_median, True, 2**32) is True      # the headline shape: 34 GB of distances, no limit
    assert sk._median_route(bw_median, True, 2**40) is True
    assert sk._median_route(bw_median, True, max(sk.MEDIAN_DEVICE_MIN_ELEMS, 4)) is True
    assert sk._median_route(bw_median, False, 2**32) is False    # CPU tensors keep the torch path
    assert sk._median_route(functools.partial(bw_median, bw_scale=2.0), True, 2**32) is True
    assert sk._median_route(functools.partial(bw_median, bw_scale=2.0, tol=1e-6), True, 2**32) is True
    assert sk._median_keywords(functools.partial(bw_median, bw_scale=2.0)) == {"bw_scale": 2.0}
    assert sk._median_route(functools.partial(bw_median, 1.0), True, 2**32) is False  # positional: not recognised
    assert sk._median_route(lambda sq: sq.median().sqrt(), True, 2**32) is False      # any other function of the data
    assert sk._median_route(lambda sq: bw_median(sq), True, 2**32) is False
    assert sk._median_route(torch.median, True, 2**32) is False


def _torch_walks(A, T, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.3 * torch.randn(A, T, d, generator=g, dtype=torch.float64)).cumsum(1)


def test_constant_bandwidth_never_reaches_the_predicate(monkeypatch):
    import sigsvgd_amd.sigkernel as sk

    def refuse(*a, **k):
        raise AssertionError("a constant bandwidth reached the route decision")

    monkeypatch.setattr(sk, "_median_route", refuse)
    monkeypatch.setattr(ops, "path_sqdist_select", refuse)
    X = _torch_walks(3, 4, 2, 0)
    assert sk.inv_bandwidth_from_fn(lambda _: 0.25, X, X) == 4.0


def test_median_bandwidth_takes_the_select_past_the_size_limit(monkeypatch):
    """`inv_bandwidth_from_fn(bw_median, ...)` on what it sees as device tensors of 2^29 + 1 distance elements (4 GiB + 8 B
    of fp64, past the limit of the torch path) asks `ops.path_sqdist_select` for the median and returns the oracle's
    1 / bw_median; other data-dependent functions and CPU tensors keep the torch path and its refusal."""
    import sigsvgd_amd.sigkernel as sk

    X, Y = _torch_walks(5, 6, 3, 1), _torch_walks(4, 7, 3, 2)
    sq = O.pairwise_sqdist(X.numpy(), Y.numpy())
    calls = []

    def select_double(P, Q=None, rank=None):
        calls.append((tuple(P.shape), None if Q is None else tuple(Q.shape), rank))
        flat = np.sort(O.pairwise_sqdist(P.numpy(), (P if Q is None else Q).numpy()).ravel())
        return torch.tensor(flat[(flat.size - 1) // 2 if rank is None else rank], dtype=torch.float64)

    monkeypatch.setattr(ops, "path_sqdist_select", select_double)
    big = (sk._MAX_DIST_BYTES >> 3) + 1
    assert big * 8 > sk._MAX_DIST_BYTES
    monkeypatch.setattr(sk, "_dist_elems", lambda P, Q: big)
    monkeypatch.setattr(sk, "_on_device", lambda P, Q: True)

    inv_h = sk.inv_bandwidth_from_fn(bw_median, X, Y)
    assert calls == [((5, 6, 3), (4, 7, 3), None)]
    assert inv_h == pytest.approx(1.0 / O.bw_median(sq), rel=1e-14)
    inv_h2 = sk.inv_bandwidth_from_fn(functools.partial(bw_median, bw_scale=2.0), X, Y)
    assert inv_h2 == pytest.approx(1.0 / O.bw_median(sq, 2.0), rel=1e-14) and len(calls) == 2
    # one buffer in both slots: the select is told so
    sk.inv_bandwidth_from_fn(bw_median, X, X)
    assert calls[-1] == ((5, 6, 3), None, None)
    # the default kernel object goes the same way
    from sigsvgd_amd.kernels import BatchGaussianKernel

    assert BatchGaussianKernel().inv_bandwidth(X, Y) == pytest.approx(1.0 / O.bw_median(sq), rel=1e-14)
    n_calls = len(calls)

    # any other data-dependent function: today's path and today's message
    with pytest.raises(RuntimeError, match="data-dependent bandwidth needs the full distance tensor"):
        sk.inv_bandwidth_from_fn(lambda s: s.median(), X, Y)
    # CPU tensors: the torch path whatever the function
    monkeypatch.setattr(sk, "_on_device", lambda P, Q: False)
    with pytest.raises(RuntimeError, match="data-dependent bandwidth needs the full distance tensor"):
        sk.inv_bandwidth_from_fn(bw_median, X, Y)
    monkeypatch.undo()
    monkeypatch.setattr(ops, "path_sqdist_select", select_double)
    assert sk.inv_bandwidth_from_fn(bw_median, X, Y) == pytest.approx(1.0 / O.bw_median(sq), rel=1e-12)  # CPU, small: torch
    assert len(calls) == n_calls
