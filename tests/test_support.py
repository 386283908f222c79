"""The shared test support (tests/parity.py) itself: the two metrics on values worked out by hand, and the two seeded path
generators pinned to their bytes.  The tolerances of the whole GPU suite were validated on these seeded inputs, so a change
to a generator that moves one value has to show up here and not as a hundred parity figures that shift a little."""
import numpy as np
import pytest
import torch

from parity import rel_entry, rel_max, sized_walks, walks


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
