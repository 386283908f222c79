"""The shared test support (tests/parity.py) itself: the two metrics on values worked out by hand, and the two seeded path
generators pinned to their bytes.  The tolerances of the whole GPU suite were validated on these seeded inputs, so a change
to a generator that moves one value has to show up here and not as a hundred parity figures that shift a little."""
import numpy as np
import pytest
import torch

from parity import bounded_points, rel_entry, rel_max, sized_walks, walks


def test_rel_entry_floors():
    K, K_ref = [1.0, 2e-7], [1.0, 1e-7]
    assert rel_entry(K, K_ref, 1e-6) == pytest.approx(0.1, rel=1e-12)  # 1e-7 over the floor
    assert rel_entry(K, K_ref, 0.0) == pytest.approx(1.0, rel=1e-12)  # 1e-7 over |K_ref| = 1e-7
    assert rel_entry([1.0, 0.06], [1.0, 0.05], 0.1) == pytest.approx(0.1, rel=1e-12)  # 0.01 over the floor, not over 0.05
    assert rel_entry([1.0, 0.06], [1.0, 0.05], 1e-6) == pytest.approx(0.2, rel=1e-12)
    assert rel_entry(torch.tensor([2.0, 4.0]), np.array([2.0, 5.0]), 1e-6) == pytest.approx(0.2, rel=1e-12)


def test_rel_entry_min_ref():
    assert rel_entry([1.0, 0.5], [1.0, 0.5], 0.0, min_ref=0.5) == 0.0
    with pytest.raises(AssertionError):
        rel_entry([1.0, 0.4], [1.0, 0.4], 0.0, min_ref=0.5)


def test_rel_max():
    assert rel_max([1.0, 3.0], [1.0, 2.0]) == 0.5
    assert rel_max(torch.tensor([1.0, 3.0], requires_grad=True), np.array([1.0, 2.0])) == 0.5
    assert rel_max(np.float32([1.0, 3.0]), torch.tensor([1.0, 2.0], dtype=torch.float64)) == 0.5
    assert rel_max([0.0, -2.0], [0.0, -4.0]) == 0.5  # entries may pass through zero: only the largest counts


def test_rel_max_refuses_an_all_zero_reference():
    with pytest.raises(AssertionError, match="all zero"):
        rel_max([0.0, 0.0], [0.0, 0.0])
    with pytest.raises(AssertionError, match="all zero"):
        rel_max([1.0, 2.0], np.zeros(2))
    with pytest.raises(AssertionError):
        rel_max([1.0, 2.0], [np.nan, 1.0])
    assert rel_max([0.0, 0.0], [0.0, 0.0], zero_ok=True) == 0.0
    assert rel_max([1e-3, 0.0], [0.0, 0.0], zero_ok=True) > 1e100


# printed by the per-file copies these generators replace (`_paths(2, 3, 2, 1)` of tests/test_gpu_fast.py, default step 0.05,
# and `paths(default_rng(7), 2, 4, 2)` of tests/test_gpu_long.py) on the commit before they moved
WALKS_2_3_2_SEED1 = ("218d8d3c7444283dfc720a3d083dc5bcdaeea13d4574e6baa1efdbbca606ee3c"
                     "e2360dbc5740333d9ddcebbbec9b913d")
SIZED_WALKS_2_4_2_RNG7 = ("193d213a2df5183e8fba0bbe3d8397be9542babee5af4abf03ddaabec41df9bd"
                          "7e027cbe71d79ebe32f59abafef406bec30b533dd3d618bf6223173d855c7fbe")


def test_walks_are_the_values_the_tolerances_were_validated_on():
    X = walks(2, 3, 2, 1, 0.05)
    assert X.dtype == np.float32 and X.shape == (2, 3, 2)
    assert X.tobytes().hex() == WALKS_2_3_2_SEED1
    assert X[0, 0, 0] == np.float32(0.017279209569096565) and X[1, 2, 1] == np.float32(0.07109817862510681)
    # the shift is added in fp64 before the one rounding to fp32
    rng = np.random.default_rng(1)
    steps = np.cumsum(0.05 * rng.standard_normal((2, 3, 2)), axis=1)
    assert walks(2, 3, 2, 1, 0.05, offset=100.0).tobytes() == (steps + 100.0).astype(np.float32).tobytes()


def test_sized_walks_are_the_values_the_tolerances_were_validated_on():
    Y = sized_walks(np.random.default_rng(7), 2, 4, 2)
    assert Y.dtype == np.float32 and Y.shape == (2, 4, 2)
    assert Y.tobytes().hex() == SIZED_WALKS_2_4_2_RNG7
    assert Y[0, 0, 0] == np.float32(0.0006150766857899725) and Y[1, 3, 1] == np.float32(-0.24937637150287628)
    # `scale` multiplies the steps before the sum: a power of two commutes with every rounding
    assert sized_walks(np.random.default_rng(7), 2, 4, 2, 2.0).tobytes() == (2 * Y).tobytes()


# printed by `bounded_points(7, 2, 4, 2, 0.5)` on the commit that added it (tests/long_reference.py chose its seeds on these values)
BOUNDED_POINTS_SEED7_2_4_2 = ("193d213a2df5183ecc5b0cbed4fde3be9cca68be8cdcfdbe2359f63c2c8c2b3f"
                              "7e027cbe71d79ebe94cc7a3ee5b9363e6de3573d2733eebe85a16fbc64ffb13e")


def test_bounded_points_are_the_values_the_tolerances_were_validated_on():
    Z = bounded_points(7, 2, 4, 2, 0.5)
    assert Z.dtype == np.float32 and Z.shape == (2, 4, 2)
    assert Z.tobytes().hex() == BOUNDED_POINTS_SEED7_2_4_2
    assert Z[1, 3, 1] == np.float32(0.5 * np.random.default_rng(7).standard_normal((2, 4, 2))[1, 3, 1])
    # independent points, not a walk: `sd` multiplies each point, and a power of two commutes with the rounding
    assert bounded_points(7, 2, 4, 2, 1.0).tobytes() == (2 * Z).tobytes()


# ---- tests/guarded_workspace.py on CPU tensors: a detector that cannot fail proves nothing ---------------------------------
CPU = torch.device("cpu")


@pytest.mark.parametrize("fill,byte", [("zeros", 0), ("ones", 0xFF), ("random", None)])
@pytest.mark.parametrize("offset", [0, 1])
def test_guarded_workspace_layout(fill, byte, offset):
    from guarded_workspace import GuardedWorkspace, MIN_GUARD

    nbytes = 5000
    ws = GuardedWorkspace(fill, offset)
    t, n = ws(CPU, nbytes)
    r = ws.requests[0]
    assert n == nbytes and t.numel() == nbytes and t.dtype == torch.uint8 and ws.count == 1 and ws.sizes == [nbytes]
    assert t.data_ptr() % 256 == offset  # offset 1: the library's aligned base lies 255 B in
    assert t.data_ptr() == r["buf"].data_ptr() + r["start"]  # a view of the one allocation, between its guards
    assert r["start"] >= MIN_GUARD and r["back"] >= MIN_GUARD and r["start"] + nbytes + r["back"] == r["buf"].numel()
    if byte is None:  # seeded bytes: the same for the same request, of many values, most of them finite as fp32
        t2, _ = GuardedWorkspace(fill, offset)(CPU, nbytes)
        assert torch.equal(t, t2) and t.unique().numel() > 200
        assert bool(torch.isfinite(t[:4 * (nbytes // 4)].clone().view(torch.float32)).float().mean() > 0.9)
    else:
        assert bool((t == byte).all())
    for g in r["guards"]:  # not a constant: a kernel's own zeros or 0xFF cannot pass for an intact guard
        assert g.unique().numel() > 200
    assert not torch.equal(r["guards"][0][:4096], r["guards"][1][:4096])
    assert ws.interior_untouched()
    t[nbytes - 1] ^= 1
    assert not ws.interior_untouched()
    ws.check()  # the interior is the launch's to write
    assert ws.requests == [] and ws.sizes == [nbytes]


def test_guarded_workspace_back_guard_covers_the_cached_slack():
    from guarded_workspace import GuardedWorkspace, MIN_GUARD

    assert GuardedWorkspace.back_guard_bytes(1) == MIN_GUARD
    big = 64 << 20
    assert GuardedWorkspace.back_guard_bytes(big) == big // 4 + 4096 >= int(big * 1.25) + 4096 - big
    ws = GuardedWorkspace()
    ws(CPU, 8 << 20)
    assert ws.requests[0]["back"] >= (8 << 20) // 4 + 4096
    ws.check()


def test_guarded_workspace_short_and_empty_requests():
    from guarded_workspace import GuardedWorkspace

    ws = GuardedWorkspace("ones", 1, short=1)
    t, n = ws(CPU, 777)
    assert n == 776 and t.numel() == 777 and ws.interior().data_ptr() == t.data_ptr()  # reported short, allocated in full
    assert ws(CPU, 0) == (None, 0) and ws.count == 2 and len(ws.requests) == 1
    ws.check()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("where", ["back first", "back last", "before interior", "front first"])
def test_guarded_workspace_notices_one_changed_guard_byte(where, offset):
    from guarded_workspace import GuardedWorkspace

    ws = GuardedWorkspace("random", offset)
    ws(CPU, 300)            # an intact launch before the damaged one: the message must name the second request
    t, n = ws(CPU, 1000)
    r = ws.requests[1]
    buf, start, end = r["buf"], r["start"], r["start"] + n
    at, guard, rel = {"back first": (end, "back", 0), "back last": (buf.numel() - 1, "back", r["back"] - 1),
                      "before interior": (start - 1, "front", -1), "front first": (0, "front", -start)}[where]
    buf[at] ^= 0x40
    with pytest.raises(AssertionError) as e:
        ws.check()
    msg = str(e.value)
    assert "request 2 of the test (nbytes=1000" in msg and "request 1 " not in msg
    assert f"{guard} guard changed in 1 bytes, lowest at {rel:+d}, highest at {rel:+d}" in msg
    assert ("interior's end" if guard == "back" else "interior's start") in msg
    assert ws.requests == []


def test_guarded_workspace_reports_the_span_of_an_overrun():
    from guarded_workspace import GuardedWorkspace

    ws = GuardedWorkspace("zeros", 1)
    t, n = ws(CPU, 4096)
    r = ws.requests[0]
    end = r["start"] + n
    want = r["guards"][1][16:64]
    r["buf"][end + 16:end + 64] = want ^ 0xFF  # 48 bytes behind the interior, every one of them changed
    with pytest.raises(AssertionError, match=r"back guard changed in 48 bytes, lowest at \+16, highest at \+63 "):
        ws.check()


def test_guarded_workspace_installs_over_ops(monkeypatch):
    from guarded_workspace import GuardedWorkspace
    from sigsvgd_amd import ops

    ws = GuardedWorkspace("ones", 1).install(monkeypatch)
    t, n = ops._workspace(CPU, 512)
    assert n == 512 and t.data_ptr() % 256 == 1 and bool((t == 0xFF).all())
    assert ops._workspace(CPU, 0) == (None, 0)
    ws.check()
