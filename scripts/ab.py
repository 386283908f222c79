"""A/B two builds of libsigsvgd_hip.so on the SAME GPU box, interleaved (cdna guide rule 24).
usage: python scripts/ab.py libA.so libB.so [libC.so ...] [rounds] [c4|c5|stream|short|bench]
`bench`: every run is `python bench.py --gpus 1 --headline-only --no-cpu-baseline --steps 200 --warmup 5` in a process of its own; prints
its ms_per_step and roofline.median_launch_ms per run, then range and median per library.  A run that fails ends the series."""
import json, os, statistics, subprocess, sys
libs = [a for a in sys.argv[1:] if a.endswith(".so")]
rest = [a for a in sys.argv[1:] if not a.endswith(".so")]
rounds = int(rest[0]) if rest else 3
shape = rest[1] if len(rest) > 1 else "c4"
if shape == "bench":
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--headline-only", "--no-cpu-baseline", "--steps", "200", "--warmup", "5"]
    ms = {lib: [] for lib in libs}
    for r in range(rounds):
        for lib in libs:
            env = dict(os.environ, SIGSVGD_LIB_PATH=os.path.abspath(lib))
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit(f"{lib}: bench.py exit status {p.returncode}\n{p.stderr[-2000:]}")
            res = json.loads(p.stdout.strip().splitlines()[-1])
            ms[lib].append(res["ms_per_step"])
            print(f"run {r + 1} {os.path.basename(lib)} ms_per_step {res['ms_per_step']:.4f} "
                  f"median_launch_ms {res['roofline']['median_launch_ms']:.4f}", flush=True)
    for lib in libs:
        v = ms[lib]
        print(f"{os.path.basename(lib)}: ms_per_step {min(v):.4f} .. {max(v):.4f} (range {max(v) - min(v):.4f}), "
              f"median {statistics.median(v):.4f}")
    sys.exit(0)
for r in range(rounds):
    for lib in libs:
        env = dict(os.environ, SIGSVGD_LIB_PATH=os.path.abspath(lib))
        out = subprocess.run([sys.executable, "scripts/dev/bench_shapes.py", shape], env=env, capture_output=True, text=True).stdout
        print(os.path.basename(lib), " || ".join(out.strip().splitlines()) if out.strip() else "??", flush=True)
