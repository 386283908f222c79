"""One rank's share of the sharded C4 step on ONE GPU (no collectives): partial solve + velocity for every rank of
G = 1, 2, 4, 8 with folded and cyclic tile ownership; worst rank / mean tells the balance.

    python scripts/shard_cost.py N T d                 the fused partial solve (ops.gram_sym_partial)
    python scripts/shard_cost.py N T d ORDER long      the long route's partial solve (ops.gram_long_sym_partial, DESIGN.md
                                                       section 5.13): every rank's share for G = 1, 2, 4, 8 (folded), its
                                                       plan (R, JC, items, grid, eff) and, alternating with the shares in the
                                                       same process, the single-GPU launches for the shape (Y-is-X and ordered):
                                                       median of 10 after warm-up, with min - max"""
import sys
import time

import torch

sys.path.insert(0, ".")
from sigsvgd_amd import ops  # noqa: E402
from sigsvgd_amd.utils.synthetic import synthetic_inputs  # noqa: E402

dev = torch.device("cuda:0")
N, T, d = (int(a) for a in sys.argv[1:4]) if len(sys.argv) > 3 else (1024, 64, 7)
ORDER = int(sys.argv[4]) if len(sys.argv) > 4 else 0
LONG = len(sys.argv) > 5 and sys.argv[5] == "long"
X, s = synthetic_inputs(N, T, d)
X, s = X.to(dev), s.to(dev)
out = (torch.empty(N, N, device=dev), torch.empty(N, T, d, device=dev, dtype=torch.float64))


def t(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.time() - t0) / n * 1e3


def long_mode(reps=10, warm=2):
    """every rank's share of the long partial solve against the single-GPU launches, alternated call by call"""
    import statistics

    def share_plan(R, JC, off, G):
        """items, grid and eff of rank `off` of G (folded) under the library's (R, JC): the kernel's item order (the chunks
        strictly inside a tile, the first chunks, the last chunks), item k on wave k mod grid"""
        owned = ops.owned_tiles(-(-N // R), off, G, True)
        nc = [-(-(N - t * R) // JC) for t in owned]
        order = [(k, c) for k in range(len(owned)) for c in range(1, nc[k] - 1)] + [(k, 0) for k in range(len(owned))]
        order += [(k, nc[k] - 1) for k in range(len(owned)) if nc[k] >= 2]
        sizes = []
        for k, c in order:
            i0 = owned[k] * R
            j0, j1 = i0 + c * JC, min(N, i0 + (c + 1) * JC)
            sizes.append(sum(max(0, j1 - max(j0, i)) for i in range(i0, min(N, i0 + R))))
        grid = max(1, min(resident, len(sizes)))
        load = [0] * grid
        for k, p in enumerate(sizes):
            load[k % grid] += p
        return dict(items=len(sizes), grid=grid, eff=-(-sum(sizes) // resident) / max(load) if sizes else 1.0)

    # resident waves of the long route at this shape: 160 KB of LDS over one wave's ring, boundary row and points, at most 8
    nrow = max(64 >> ORDER, 1)
    Wcap = 1
    while Wcap * 2 * nrow <= 8192:
        Wcap <<= 1
    W = 1
    while W < T - 1:
        W <<= 1
    lds = (nrow * min(W, Wcap) + (T - 1 << ORDER) + 2 + 64 + (nrow + 1) * d) * 8
    resident = torch.cuda.get_device_properties(0).multi_processor_count * min(160 * 1024 // lds, 8)

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    calls = {("yx",): lambda: ops.gram_long_fwd_bwd2(X, X, 1.0, ORDER, y_is_x=True),
             ("ordered",): lambda: ops.gram_long_fwd_bwd(X, X, 1.0, ORDER)}
    rowwise = N % 8 == 0 and ops.gram_takes(N // 8, N, T, d, ORDER)  # a rank's row-wise solve at G = 8, where it runs
    if rowwise:
        calls[("rowwise8",)] = lambda: ops.gram_fwd_bwd(X[:N // 8], X, 1.0, ORDER)
    for G in (1, 2, 4, 8):
        for r in range(G):
            calls[(G, r)] = lambda G=G, r=r: ops.gram_long_sym_partial(X, 1.0, r, G, ORDER, out=out, fold=True)
    ms = {k: [] for k in calls}
    for rep in range(warm + reps):
        for k, fn in calls.items():  # one call of each in turn: shares and parents see the same clocks
            v = once(fn)
            if rep >= warm:
                ms[k].append(v)
    fmt = lambda v: f"{statistics.median(v):.2f} ({min(v):.2f} - {max(v):.2f})"
    print(f"N={N} T={T} d={d} order={ORDER}: Y-is-X launch {fmt(ms[('yx',)])} ms | ordered launch {fmt(ms[('ordered',)])} ms",
          flush=True)
    if rowwise:
        print(f"row-wise solve of one rank of 8 (own rows x all columns, fused kernels): {fmt(ms[('rowwise8',)])} ms", flush=True)
    parent = min(statistics.median(ms[("yx",)]), statistics.median(ms[("ordered",)]))
    for G in (1, 2, 4, 8):
        R, JC = ops.gram_long_partial_tiles(N, T, d, ORDER, 0, G)
        pls = [share_plan(R, JC, r, G) for r in range(G)]
        med = [statistics.median(ms[(G, r)]) for r in range(G)]
        mean = sum(med) / G
        print(f"G={G}: R={R} JC={JC} items {min(p['items'] for p in pls)}-{max(p['items'] for p in pls)} "
              f"grid {pls[0]['grid']} eff {min(p['eff'] for p in pls):.3f} | share min {min(med):.2f} mean {mean:.2f} max "
              f"{max(med):.2f} ms (worst/mean {max(med) / mean:.3f}; slowest single run "
              f"{max(max(ms[(G, r)]) for r in range(G)):.2f}) | G x slowest {G * max(med):.2f} ms = "
              f"{G * max(med) / parent:.3f} x the faster single-GPU launch", flush=True)


if LONG:
    long_mode()
    sys.exit(0)

for G in (1, 2, 4, 8):
    for fold in (True, False):
        part = [t(lambda r=r: ops.gram_sym_partial(X, 1.0, r, G, out=out, fold=fold), 10) for r in range(G)]
        Kp, gp = ops.gram_sym_partial(X, 1.0, 0, G, out=out, fold=fold)
        phi = t(lambda: ops.svgd_phi(Kp, s, gp.to(s.dtype)))

        def step():
            Kp, gp = ops.gram_sym_partial(X, 1.0, G - 1, G, out=out, fold=fold)
            return ops.svgd_phi(Kp, s, gp.to(s.dtype))

        mean = sum(part) / G
        print(f"G={G} {'folded' if fold else 'cyclic'}: partial solve per rank min {min(part):.3f} mean {mean:.3f} max "
              f"{max(part):.3f} ms (worst/mean {max(part) / mean:.3f}) | velocity {phi:.3f} ms | partial + velocity "
              f"(last rank, incl. K_partial zeroing) {t(step):.3f} ms", flush=True)
