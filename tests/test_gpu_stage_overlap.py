"""The column staging of gram_fast_kernel in the multi-item regime (csrc/gram_fast_kernel.h, "staging").

A workgroup of the register-resident kernel walks a range of (row tile, column) items.  The next column trajectory is
loaded at the top of the current pair and stays in flight, as raw bits, through the pair; after the pair's closing
barrier the waves add up their parked column-side sums, convert and store the column (fp64 and fp32 side, row norms,
reference point) into the one LDS buffer, and meet at a second barrier.  What can go wrong there does not show with one item
per workgroup: a stale or half-written column buffer, the wrong column after a tile change or on the first column of a
range, a race between the block sum of the column-side gradient and the next pair's stores into the same LDS, a wave
without a pair that misses a barrier.  (The file was written with a variant that stores the next column's fp64 side into a
second buffer during the pair and moves the second barrier into the next pair; it passed here and lost time, DESIGN.md
5.1.  The cases are the ones that variant needs, so a next attempt finds them in place.)  Every case below therefore
asserts, from `plans.gram_geometry` with the device's CU count, the regime of
tests/test_gpu_partition.py (items >= 2 grid + 1, a range that starts inside a tile, one that crosses a tile boundary, a
tile met by two workgroups), that ranges of three items exist and -- Y-is-X launches, whose size is free -- that one of them
crosses a tile boundary, at sizes ragged against the tile height, with signed weights where the launch takes them.

Per case:
  * K and the gradient against the fp64 oracle, metric and bound of tests/test_gpu_partition.py;
  * five launches on the same inputs return byte-equal K and gradient (a race in the overlapped window shows here);
  * K[i][j] of about 32 probe pairs -- first and last item of workgroup ranges spread over the launch, as
    tests/test_gram_geometry.py spreads them -- is byte-equal to the same pair solved alone, as the only off-diagonal pair
    of a two-trajectory launch of the same kind (Y-is-X launches: K[0][1] on X[[i, j]]; the ordered launch: K[0][0] of
    X[[i]] against Y[[j]], which runs the same ordered kernel).  A pair's solve does not depend on where, when or into which
    buffer its column was staged, so a wrong or stale column cannot pass this.  (The parent of the commit that added this
    file satisfies the byte equality on the same inputs.)
"""
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from parity import rel_entry, rel_max, signed_weights, walks
from plans import device_cus, gram_geometry, gram_item_ranges, gram_multi_item_regime, probes

pytestmark = pytest.mark.gpu

TOL = 1e-5  # tests/test_gpu_partition.py: K per entry, the gradient relative to its largest entry

# variant: what of the kernel the shape reaches; launch: "sym" (Y is X, gradient), "ordered" (A x B, gradient),
# "fwdsym" (Y is X, forward only); size: N or (A, B); rows: rows per tile the geometry must report
Case = namedtuple("Case", "variant launch T d size rows")
CASES = [
    Case("fast<8,8> LP, fixed windows (headline twin)", "sym", 64, 7, 97, 8),
    Case("fast<8,8>: the row norms in ynd", "sym", 64, 8, 97, 8),
    Case("fast<8,8> LP, table windows", "sym", 40, 7, 97, 8),
    Case("fast<8,4,32>: 32-slot ring, two rows per wave, three workgroups per CU", "sym", 32, 7, 181, 8),
    Case("fast<4,8> LP with the flag array", "sym", 64, 3, 97, 8),
    Case("fast<16,4>: 4-row tiles", "sym", 64, 12, 71, 4),
    Case("fast<8,8> LP ordered: no block sum", "ordered", 64, 7, (43, 97), 8),
    Case("fwd<8,4> Y is X: no yf, no G image", "fwdsym", 64, 7, 117, 4),
]


def _id(c):
    return f"{c.launch}-T{c.T}-d{c.d}"


def _claim(c):
    """assert the regime on this device; -> (A, B, sym, grad, geometry)"""
    sym, grad = c.launch != "ordered", c.launch != "fwdsym"
    A, B = (c.size, c.size) if sym else c.size
    g = gram_geometry(A, B, c.T, c.d, 0, grad, sym, device_cus())
    assert g is not None and g["family"] == "fast" and g["rows_per_tile"] == c.rows, g
    r = gram_multi_item_regime(A, B, g, sym)
    bounds, starts = gram_item_ranges(A, B, g, sym)
    lo, hi, inner = bounds[:-1], bounds[1:], starts[1:-1]
    long_cross = bool((((lo[:, None] < inner[None, :]) & (inner[None, :] < hi[:, None])).any(axis=1) & (hi - lo >= 3)).any())
    print(f"{c.variant}: {A} x {B}, {g['rows_per_tile']} rows per tile, {g['items']} items on {g['grid']} workgroups, "
          f"regime {r}, a range of >= 3 items crosses a tile boundary: {long_cross}")
    assert all(r.values()) and int((hi - lo).max()) >= 3, (g, r)
    if sym:  # (the ordered launch runs at the 43 x 97 of the partition file: its ranges of three items lie inside tiles)
        assert long_cross, g
    assert A % c.rows and B % c.rows, "ragged against the tile height"
    return A, B, sym, grad, g


_cache = {}


def _launched(c, gpu):
    """inputs, the oracle's result (once per case) and one launch of the case"""
    if c not in _cache:
        A, B, sym, grad, g = _claim(c)
        h = 1.1 if sym else 0.9
        X = walks(A, c.T, c.d, 21 if sym else 11, 0.05)
        Y = X if sym else walks(B, c.T, c.d, 12, 0.05)
        go = signed_weights(A, B, 23 if sym else 13) if grad else None
        Kref, gref = C.gram_fwd_bwd(X, Y, h, 0, grad_out=go, want_grad=grad)
        Xg = torch.as_tensor(X, device=gpu)
        Yg = Xg if sym else torch.as_tensor(Y, device=gpu)
        gog = None if go is None else torch.as_tensor(go, device=gpu, dtype=torch.float32)

        def launch(Xa=Xg, Ya=Yg, w=gog):
            from sigsvgd_amd import ops

            if not grad:
                return ops.gram_fwd(Xa, Ya, 1.0 / h, 0, y_is_x=sym), None
            return ops.gram_fwd_bwd(Xa, Ya, 1.0 / h, 0, grad_out=w, y_is_x=sym)

        K, gx = launch()
        torch.cuda.synchronize()
        _cache[c] = dict(A=A, B=B, sym=sym, grad=grad, geom=g, Xg=Xg, Yg=Yg, Kref=Kref, gref=gref, launch=launch, K=K, gx=gx)
    return _cache[c]


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_against_the_oracle(gpu, c):
    s = _launched(c, gpu)
    eK = rel_entry(s["K"].cpu().numpy(), s["Kref"], 1e-6)
    eg = rel_max(s["gx"].cpu().numpy(), s["gref"]) if s["grad"] else 0.0
    print(f"K {eK:.2e} gradient {eg:.2e}")
    assert eK < TOL and eg < TOL
    if s["sym"]:
        assert torch.equal(s["K"], s["K"].T)


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_five_launches_are_byte_equal(gpu, c):
    s = _launched(c, gpu)
    for k in range(4):
        K, gx = s["launch"]()
        torch.cuda.synchronize()
        sameK = torch.equal(K, s["K"])
        sameg = gx is None or torch.equal(gx, s["gx"])
        print(f"launch {k + 2}: K equal {sameK}, gradient equal {sameg}")
        assert sameK and sameg


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_probe_pairs_equal_the_pair_solved_alone(gpu, c):
    s = _launched(c, gpu)
    pairs = probes(s["A"], s["B"], s["geom"], s["sym"], 5)
    assert len(pairs) == 32
    K = s["K"].cpu().numpy()
    bad = []
    for (i, j) in pairs:
        if s["sym"]:
            Z = s["Xg"][[i, j]].contiguous()
            w = None if not s["grad"] else torch.ones(2, 2, device=gpu)
            alone = s["launch"](Z, Z, w)[0][0, 1]
        else:
            w = torch.ones(1, 1, device=gpu)
            alone = s["launch"](s["Xg"][[i]].contiguous(), s["Yg"][[j]].contiguous(), w)[0][0, 0]
        a = np.float32(alone.item())
        if a.tobytes() != K[i, j].tobytes():
            bad.append((i, j, float(a), float(K[i, j])))
    print(f"{len(pairs)} probes, {len(bad)} differ from the pair solved alone: {bad[:4]}")
    assert not bad
