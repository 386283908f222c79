"""Host-side checks of `sigsvgd_pair_schedule` (include/sigsvgd_hip.h): which kernel a paired
launch runs -- one wavefront per pair (csrc/gram_long.hip) or a workgroup per pair with the bands dealt to its wavefronts
(csrc/pair_bands.hip) --, under SIGSVGD_PAIR_MODE and under the default rule, and that the workspace does not depend on it.
No device needed: every call returns before any device work."""
import ctypes

import pytest

from cabi import assert_exported, BADARG, lib, UNSUPPORTED
from plans import device_cus, pair_plan
from sigsvgd_amd import _lib, ops

LDS_MAX = 160 * 1024
# (A, TX, TY, d, order): two bands up to 64, orders 0 .. 8, TX != TY, more bands than waves, a wide channel count
SHAPES = [(2, 1024, 1024, 4, 0), (2, 260, 260, 3, 2), (3, 130, 130, 2, 0), (2, 322, 322, 3, 0), (2, 400, 6, 2, 0),
          (2, 70, 600, 2, 0), (2, 9, 9, 2, 8), (3, 150, 140, 3, 1), (2, 300, 300, 17, 0), (1, 4096, 4096, 4, 0),
          (6, 100, 100, 3, 3), (64, 200, 200, 3, 2), (1024, 64, 64, 7, 0), (2, 40, 40, 3, 0), (2, 300, 300, 183, 0),
          (2, 8193, 8193, 2, 0), (5000, 130, 130, 2, 0)]


def schedule(A, TX, TY, d, n, kind=_lib.STATIC_RBF, want_grad=1, flags=0, null=None):
    w, g, b = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_size_t(12345)
    outs = [None if null == k else ctypes.byref(v) for k, v in (("waves", w), ("grid", g), ("lds", b))]
    rc = lib().sigsvgd_pair_schedule(A, TX, TY, d, n, kind, want_grad, flags, *outs)
    return rc, w.value, g.value, b.value


def pair_ws(A, TX, TY, d, n, want_grad=1, flags=0):
    b = ctypes.c_size_t(12345)
    rc = lib().sigsvgd_pair_workspace_bytes(A, TX, TY, d, n, _lib.STATIC_RBF, want_grad, flags, ctypes.byref(b))
    return rc, b.value


def nbands(TX, n):
    return -(-((TX - 1) << n) // 64)


def test_pair_schedule_exported():
    assert_exported(("sigsvgd_pair_schedule",), abi=10)
    assert "sigsvgd_pair_schedule" in _lib.ARGTYPES and len(_lib.ARGTYPES["sigsvgd_pair_schedule"]) == 11


@pytest.mark.parametrize("mode", ["serial", "bands", None])
def test_pair_schedule_refusals_are_the_workspace_query_s(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("SIGSVGD_PAIR_MODE", raising=False)
    else:
        monkeypatch.setenv("SIGSVGD_PAIR_MODE", mode)
    for null in ("waves", "grid", "lds"):
        assert schedule(3, 300, 200, 2, 0, null=null)[0] == BADARG
    cases = [dict(flags=_lib.FLAG_SYM), dict(n=11), dict(TX=8194), dict(TY=8194), dict(A=0), dict(d=0), dict(kind=5),
             dict(flags=_lib.FLAG_Y_IS_X), dict(d=184, TY=300)]
    for upd in cases:
        a = {**dict(A=3, TX=300, TY=200, d=2, n=0, kind=_lib.STATIC_RBF, flags=0), **upd}
        b = ctypes.c_size_t(0)
        want = lib().sigsvgd_pair_workspace_bytes(a["A"], a["TX"], a["TY"], a["d"], a["n"], a["kind"], 1, a["flags"],
                                                  ctypes.byref(b))
        got = schedule(a["A"], a["TX"], a["TY"], a["d"], a["n"], a["kind"], 1, a["flags"])[0]
        assert got == want and got in (BADARG, UNSUPPORTED), (upd, got, want)
    assert schedule(3, 300, 200, 2, 0, flags=_lib.FLAG_SYM)[0] == BADARG
    assert schedule(3, 300, 200, 2, 11)[0] == BADARG
    assert schedule(3, 8194, 10, 2, 0)[0] == UNSUPPORTED


def test_pair_schedule_serial_is_todays_plan(monkeypatch):
    monkeypatch.setenv("SIGSVGD_PAIR_MODE", "serial")
    cus = device_cus()
    for (A, TX, TY, d, n) in SHAPES:
        for want_grad in (0, 1):
            pl = pair_plan(A, TX, TY, d, n, want_grad, cus)
            rc, waves, grid, lds = schedule(A, TX, TY, d, n, want_grad=want_grad)
            assert rc == 0, _lib.last_error()
            assert (waves, grid, lds) == (1, pl["grid"], pl["lds"]), (A, TX, TY, d, n, want_grad)


def test_pair_schedule_bands(monkeypatch):
    monkeypatch.setenv("SIGSVGD_PAIR_MODE", "bands")
    cus = device_cus()
    for (A, TX, TY, d, n) in SHAPES:
        for want_grad in (0, 1):
            rc, waves, grid, lds = schedule(A, TX, TY, d, n, want_grad=want_grad)
            assert rc == 0, _lib.last_error()
            pl = pair_plan(A, TX, TY, d, n, want_grad, cus)
            if waves == 1:  # stays on the serial kernel: its plan
                assert (grid, lds) == (pl["grid"], pl["lds"])
                continue
            assert 2 <= waves <= 16 and waves <= nbands(TX, n), (A, TX, TY, d, n, waves)
            assert lds <= LDS_MAX
            assert 1 <= grid <= min(A, pl["grid"])  # never more pairs in flight than the workspace has slots for
    W = lambda *a: schedule(*a)[1]
    assert W(2, 1024, 1024, 4, 0) >= 4 and W(2, 1024, 1024, 8, 0) >= 4
    assert W(2, 260, 260, 3, 2) >= 8 and W(2, 1024, 1024, 4, 2) >= 8 and W(2, 1024, 1024, 4, 3) >= 8
    assert W(2, 40, 40, 3, 0) == 1      # one band
    assert W(2, 65, 300, 3, 0) == 1     # 64 rows: still one band
    assert W(2, 66, 300, 3, 0) == 2
    assert W(2, 300, 300, 183, 0) == 1  # 65 points of 183 channels per wave: LDS admits no second wave
    assert W(2, 300, 300, 17, 0) > 1
    assert ops.pair_schedule(2, 1024, 1024, 4)[0] == W(2, 1024, 1024, 4, 0)
    assert ops.pair_schedule(2, 260, 260, 3, 2, want_grad=False) == schedule(2, 260, 260, 3, 2, want_grad=0)[1:]


def test_pair_workspace_does_not_depend_on_the_mode(monkeypatch):
    cus = device_cus()
    for mode in ("serial", "bands", None):
        if mode is None:
            monkeypatch.delenv("SIGSVGD_PAIR_MODE", raising=False)
        else:
            monkeypatch.setenv("SIGSVGD_PAIR_MODE", mode)
        for (A, TX, TY, d, n) in SHAPES:
            for want_grad in (0, 1):
                rc, b = pair_ws(A, TX, TY, d, n, want_grad)
                assert rc == 0 and b == pair_plan(A, TX, TY, d, n, want_grad, cus)["bytes"], (mode, A, TX, TY, d, n)
                if not want_grad:
                    assert b == 0


def test_pair_schedule_default_rule(monkeypatch):
    """bands where 3 x its rounds x its dependent steps stay below the serial schedule's rounds x steps"""
    monkeypatch.delenv("SIGSVGD_PAIR_MODE", raising=False)
    D = lambda *a, **k: schedule(*a, **k)[1]
    assert D(1024, 64, 64, 7, 0) == 1         # many short pairs, one band: the serial kernel
    assert D(2, 1024, 1024, 4, 0) > 1         # a handful of long pairs: bands
    assert D(1, 4096, 4096, 4, 0) > 1
    for (A, T, d, n) in [(6, 1024, 4, 0), (32, 1024, 4, 0), (128, 1024, 4, 0), (512, 1024, 4, 0), (6, 100, 3, 3),
                         (16, 100, 3, 3), (64, 200, 3, 2)]:  # the measured shapes where bands is ahead
        assert D(A, T, T, d, n) > 1 and D(A, T, T, d, n, want_grad=0) > 1, (A, T, d, n)
    # few bands per pair: the pipeline's fill outweighs what it shares out, at any number of pairs
    assert D(2, 40, 40, 3, 0) == 1 and D(2, 100, 100, 3, 0) == 1 and D(3, 130, 130, 2, 0) == 1
    assert D(2, 322, 322, 3, 0) == 1 and D(300, 322, 322, 3, 0) == 1
    # many short pairs of two bands or more stay serial
    assert D(2000, 100, 100, 3, 0) == 1 and D(1024, 100, 100, 3, 0) == 1 and D(4000, 128, 128, 3, 0) == 1
    assert D(100000, 130, 130, 2, 0) == 1
    # the threshold in the number of bands at these lengths: six bands (T = 322: 3 x 49 phases x 16 = 2352 steps against
    # 6 x 384 = 2304) stay serial, seven (T = 386: 3 x 58 x 16 = 2784 against 7 x 448 = 3136) go to the workgroup
    assert D(2, 322, 322, 3, 0) == 1 and D(2, 386, 386, 3, 0) > 1 and D(2, 450, 450, 3, 0) > 1


def test_pair_mode_is_matched_whole(monkeypatch):
    """only `serial` and `bands` pin the schedule; anything else leaves the default rule in charge"""
    for value, want_long, want_short in [("serial", 1, 1), ("bands", 8, 3), ("both", 8, 1), ("s", 8, 1), ("b", 8, 1),
                                         ("serial-ish", 8, 1), ("", 8, 1)]:
        monkeypatch.setenv("SIGSVGD_PAIR_MODE", value)
        assert schedule(2, 1024, 1024, 4, 0)[1] == want_long, value
        assert schedule(3, 130, 130, 2, 0)[1] == want_short, value
