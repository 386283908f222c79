"""A/B of the coverage kernel's RBF launch between two builds of libsigsvgd_hip.so, interleaved on one device as scripts/ab.py
does, with a bit comparison of what the RBF, linear, IMQ and rational-quadratic kernels return on every entry point that takes a
static kernel (the kinds both builds have; IMQ and RQ without the first-order stencil on the long route, which has none for them).

    python scripts/static_kinds_ab.py parent.so branch.so [rounds=6]

Every run is a process of its own under SIGSVGD_LIB_PATH.  It times ops.gram_fwd_bwd(X, X, 1.0, 0, y_is_x=True,
force_generic=True) at N = 256, T = 64, d = 7 (median of 10 launches with device events after warm-up) and saves the RBF and
other kinds' outputs of the fused, long, two-sided, paired, partial and bandwidth launches.  Prints the series, range and median per library,
and whether every saved tensor of the last library equals the first's bit for bit."""
import os
import statistics
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def child(out_path):
    import torch

    from oracle import sigkernel_oracle as O
    from sigsvgd_amd import ops
    from long_time import timed

    dev = torch.device("cuda:0")
    X = O.synthetic_inputs(256, 64, 7)[0].to(dev)
    ms = timed(lambda: ops.gram_fwd_bwd(X, X, 1.0, 0, y_is_x=True, force_generic=True), 10, warmup=3)[0]
    out = {}
    K, g = ops.gram_fwd_bwd(X, X, 1.0, 0, y_is_x=True, force_generic=True)
    out["generic_forced"] = (K, g)
    S = O.synthetic_inputs(24, 64, 7)[0].to(dev)
    out["smoke_shape"] = ops.gram_fwd_bwd(S, S, 1.0, 0, y_is_x=True)
    W = torch.as_tensor(O.synthetic_inputs(6, 6, 1, seed_x=3)[0][..., 0], dtype=torch.float64, device=dev)
    for kind in (0, 1, 2, 3):
        for (T, d, n) in [(20, 3, 2), (70, 17, 0), (128, 14, 0)]:
            A, B = O.synthetic_inputs(6, T, d)[0].double().to(dev), O.synthetic_inputs(6, T, d, seed_x=5)[0].double().to(dev)
            out[f"generic k{kind} {T} {d} {n}"] = ops.gram_fwd_bwd(A, B, 1.0, n, kind, W, force_generic=True)
            out[f"generic fwd k{kind} {T} {d} {n}"] = (ops.gram_fwd(A, B, 1.0, n, kind, force_generic=True),)
            out[f"generic naive k{kind} {T} {d} {n}"] = ops.gram_fwd_bwd(A, B, 1.0, n, kind, W, naive=True, force_generic=True)
        big = O.synthetic_inputs(64, 6, 2)[0].double().to(dev)
        out[f"generic yx k{kind}"] = ops.gram_fwd_bwd(big, big, 1.0, 0, kind, y_is_x=True, force_generic=True)
        for (TX, TY, d, n) in [(70, 66, 3, 0), (9, 12, 17, 2), (300, 300, 2, 0)]:
            A, B = O.synthetic_inputs(6, TX, d)[0].double().to(dev), O.synthetic_inputs(6, TY, d, seed_x=5)[0].double().to(dev)
            for naive in ((False, True) if kind < 2 else (False,)):
                out[f"long k{kind} {TX} {d} {n} {naive}"] = ops.gram_long_fwd_bwd(A, B, 1.0, n, kind, W, naive)
                out[f"long2 k{kind} {TX} {d} {n} {naive}"] = ops.gram_long_fwd_bwd2(A, B, 1.0, n, kind, W, naive)
                out[f"pair k{kind} {TX} {d} {n} {naive}"] = ops.pair_fwd_bwd(A, B, 1.0, n, kind, W[0].contiguous(), naive)
            out[f"long fwd k{kind} {TX} {d} {n}"] = (ops.gram_long_fwd(A, B, 1.0, n, kind), ops.pair_fwd(A, B, 1.0, n, kind))
            if TX == TY:
                out[f"long2 yx k{kind} {TX}"] = ops.gram_long_fwd_bwd2(A, A, 1.0, n, kind, W, y_is_x=True)[:2]
                out[f"partial k{kind} {TX}"] = ops.gram_long_sym_partial(A, 1.0, 1, 2, n, kind, W, fold=True)
            if kind != 1:  # (the linear kernel has no bandwidth)
                out[f"long h k{kind} {TX} {d} {n}"] = ops.gram_long_fwd_bwd_h(A, B, 1.0, n, kind, W)
                out[f"pair h k{kind} {TX} {d} {n}"] = ops.pair_fwd_bwd_h(A, B, 1.0, n, kind, W[0].contiguous())
    torch.cuda.synchronize()
    torch.save({k: tuple(t.cpu() for t in v) for k, v in out.items()}, out_path)
    print(f"MS {ms:.4f}")


def main():
    libs = [a for a in sys.argv[1:] if a.endswith(".so")]
    rest = [a for a in sys.argv[1:] if not a.endswith(".so")]
    rounds = int(rest[0]) if rest else 6
    import torch

    ms = {lib: [] for lib in libs}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(rounds):
            for k, lib in enumerate(libs):
                env = dict(os.environ, SIGSVGD_LIB_PATH=os.path.abspath(lib))
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.join(tmp, f"{k}.pt")], env=env,
                                   capture_output=True, text=True, timeout=300)
                if p.returncode != 0:
                    sys.exit(f"{lib}: exit status {p.returncode}\n{p.stderr[-2000:]}")
                ms[lib].append(float(p.stdout.strip().splitlines()[-1].split()[1]))
                print(f"run {r + 1} {lib} generic_forced_ms {ms[lib][-1]:.4f}", flush=True)
        for lib in libs:
            v = ms[lib]
            print(f"{lib}: {min(v):.4f} .. {max(v):.4f} (range {max(v) - min(v):.4f}), median {statistics.median(v):.4f}")
        first, last = torch.load(os.path.join(tmp, "0.pt")), torch.load(os.path.join(tmp, f"{len(libs) - 1}.pt"))
        bad = [k for k in first if not all(torch.equal(a, b) for a, b in zip(first[k], last[k]))]
        print(f"bit comparison of {len(first)} RBF / linear / IMQ / RQ launches, {libs[0]} against {libs[-1]}: "
              + ("all equal" if not bad and first.keys() == last.keys() else f"DIFFERENT: {bad}"))
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
