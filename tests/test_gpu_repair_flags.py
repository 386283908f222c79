"""The exact fp64 pass over the pairs an fp32-sweep kernel flagged (`generic_repair_launch`, csrc/gram_generic.hip), at known flag
positions.

On fp64 I/O a repaired entry (about 1e-13 from the oracle) and an fp32-sweep entry (rarely below 1e-8) are far apart, so the
set of repaired pairs can be read off K.  The batches (tests/generic_reference.py: `flag_batch`, `flag_batch_sym`) hold one
rough pair (x*, y*) at twice the rules' thresholds -- c1 >= 300 against 150, the forward-only figure >= 600 against 300 --
at chosen rows and columns of a batch of very smooth paths that no rule comes near
(tests/test_generic_reference_cpu.py asserts both on the oracle).  Every launch is held to:
    every targeted entry within 1e-10 of the oracle (the exact pass reached it: flag words, their ends, the tile map);
    every entry within 1e-5 (the contract);
    at least 90 % of the smooth x smooth entries further than 1e-9 from it (nothing else went through the exact pass: an
    fp32 result lands within 1e-9 by chance for about one pair in a hundred; the observed share is printed)."""
import numpy as np
import pytest
import torch

import generic_reference as G
from oracle import c_oracle as C
from parity import np64
from plans import device_cus, gram_geometry, set_band_mode

pytestmark = pytest.mark.gpu

_REF = {}


def oracle(name, X, Y, fs):
    if name not in _REF:
        _REF[name] = C.gram_fwd_bwd(X, Y, fs.h, fs.n, want_grad=False)[0]
    return _REF[name]


def assert_repaired(K, Kref, targeted, smooth, where, owned=None):
    """the three assertions of the module docstring on the entries `owned` (all of them when None)"""
    K, owned = np64(K), np.ones(Kref.shape, bool) if owned is None else owned
    assert np.abs(Kref[targeted | smooth]).min() > 0.1
    err = np.abs(K - Kref) / np.maximum(np.abs(Kref), 1e-6)
    t, s = targeted & owned, smooth & owned
    share = float((err[s] > 1e-9).mean())
    print(f"{where}: {t.sum()} targeted entries within {err[t].max():.2e}; all within {err[owned].max():.2e}; "
          f"{share:.4f} of {s.sum()} smooth entries further than 1e-9 (closest {err[s].min():.2e})")
    assert t.any() and err[t].max() < 1e-10
    assert err[owned].max() < 1e-5
    assert share >= 0.9
    return share


def family(A, B, fs, want_grad, sym, mode=None):
    g = gram_geometry(A, B, fs.T, fs.d, fs.n, want_grad, sym, device_cus(), mode)
    assert g is not None, "not a launch of the fp32-sweep kernels"
    return g["family"]


@pytest.mark.parametrize("name,fs,fam", [("fast", G.FLAG_FAST, "fast"), ("quad", G.FLAG_QUAD, "quad")])
def test_ordered_flag_words_and_tiles(gpu, name, fs, fam):
    """ordered 10 x 130: x* at both ends of a full row tile and of a last tile of two rows, y* at both ends of the 64-flag
    words and in the short last word; the gradient launch (rule: c1 > 150) and the forward-only launch (figure > 300) on the
    register-resident kernel (T = 64) and the quadrant kernel (T = 100)"""
    from sigsvgd_amd import ops

    X, Y, targeted, smooth = G.flag_batch(fs, 10, 130, G.ROWS, G.COLS)
    Kref = oracle(name, X, Y, fs)
    Xg, Yg = (torch.as_tensor(t, device=gpu).double() for t in (X, Y))
    assert family(10, 130, fs, True, False) == fam == family(10, 130, fs, False, False)
    K, _ = ops.gram_fwd_bwd(Xg, Yg, 1.0 / fs.h, fs.n)
    assert_repaired(K, Kref, targeted, smooth, f"{name} gradient launch")
    assert_repaired(ops.gram_fwd(Xg, Yg, 1.0 / fs.h, fs.n), Kref, targeted, smooth, f"{name} forward-only launch")


@pytest.mark.parametrize("mode", ["serial", "parallel"])
def test_refined_grid_kernels(gpu, monkeypatch, mode):
    """order 3, 256 cells: the band kernels on both schedules; the exact pass reads the coarse increment table (Drow >> n)"""
    from sigsvgd_amd import ops

    fs = G.FLAG_BAND
    set_band_mode(monkeypatch, mode)
    X, Y, targeted, smooth = G.flag_batch(fs, 10, 130, G.ROWS, G.COLS)
    Kref = oracle("band", X, Y, fs)
    Xg, Yg = (torch.as_tensor(t, device=gpu).double() for t in (X, Y))
    assert family(10, 130, fs, True, False, mode) == f"band {mode}"
    K, _ = ops.gram_fwd_bwd(Xg, Yg, 1.0 / fs.h, fs.n)
    assert_repaired(K, Kref, targeted, smooth, f"band {mode} gradient launch")
    assert_repaired(ops.gram_fwd(Xg, Yg, 1.0 / fs.h, fs.n), Kref, targeted, smooth, f"band {mode} forward-only launch")


def test_symmetric_and_partial_solves(gpu):
    """Y is X, N = 130, x* and y* interleaved: targeted pairs on both sides of the diagonal, of which only j >= i is solved
    and flagged -- the mirror image carries the same bits.  The same batch through the partial solve, cyclic over two ranks
    and folded over three: each share repairs the targeted pairs of the tiles it owns and is zero elsewhere, and the shares add up to
    the full launch's K bit for bit."""
    from sigsvgd_amd import ops

    fs, N = G.FLAG_FAST, 130
    X, targeted, smooth = G.flag_batch_sym(fs, N, G.SYM_X, G.SYM_Y)
    assert np.triu(targeted, 1).any() and np.tril(targeted, -1).any()
    Kref = oracle("sym", X, X, fs)
    Xg = torch.as_tensor(X, device=gpu).double()
    assert family(N, N, fs, True, True) == "fast"
    K, _ = ops.gram_fwd_bwd(Xg, Xg, 1.0 / fs.h, fs.n, y_is_x=True)
    assert torch.equal(K, K.T)
    assert_repaired(K, Kref, targeted, smooth, "Y is X gradient launch")
    Kf = ops.gram_fwd(Xg, Xg, 1.0 / fs.h, fs.n, y_is_x=True)
    assert torch.equal(Kf, Kf.T)
    assert_repaired(Kf, Kref, targeted, smooth, "Y is X forward-only launch")
    rows = ops.sym_tile_rows(fs.T, fs.d)
    ntile = -(-N // rows)
    assert ntile == 17 and sorted(ops.owned_tiles(ntile, 0, 2, True)) == sorted(ops.owned_tiles(ntile, 0, 2, False))
    for (fold, ranks) in [(False, 2), (True, 3)]:  # (17 tiles: folded over two ranks is the cyclic split; over three it is not)
        total = torch.zeros_like(K)
        for rank in range(ranks):
            Kp, _ = ops.gram_sym_partial(Xg, 1.0 / fs.h, rank, ranks, fold=fold)
            tile_of = np.arange(N) // rows
            own_row = np.isin(tile_of, ops.owned_tiles(ntile, rank, ranks, fold))
            i, j = np.minimum(*np.indices((N, N))), np.maximum(*np.indices((N, N)))
            owned = own_row[i]  # (i <= j: the pair belongs to the tile of its smaller index; both of its entries are stored)
            assert np.array_equal(np64(Kp) != 0, owned), (fold, rank)
            assert_repaired(Kp, Kref, targeted, smooth, f"partial solve, {'folded' if fold else 'cyclic'}, rank {rank}", owned)
            total += Kp
        assert torch.equal(total, K), fold
