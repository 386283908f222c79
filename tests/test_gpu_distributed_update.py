"""The sharded step with its update rules on the device: `ShardedSigSVGD(update=..., mask=...)` under nccl (= RCCL) with one
rank, in a child process (a process group of its own, torn down with the process), N = 16, T = 8, d = 3, Adam + mask and
Adagrad, three steps each.

After every step `last_v_rows` is within the project's phi tolerance of `oracle.svgd_velocity` (1e-5 of its largest entry,
DESIGN.md section 2), and the new particles and state equal the fp64 formulas (torch.optim.Adam itself; the reference's two
Adagrad lines) applied to that same `last_v_rows` and to the particles and state the step started from, within the fp32
roundings of one update: the counts are stated and derived in tests/update_reference.py (Adam: exp_avg 4, exp_avg_sq 8, X 14
roundings of 2^-24, X relative to |x| + step_size |m / (sqrt(q)/sqrt(bc2) + eps)|; Adagrad: sum 3, X 7).  An independent
run's velocity is no reference for the update: Adam's division turns last-bit differences of entries near zero into
differences of the order of lr."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N, T, D, STEPS, LR = 16, 8, 3, 3, 1e-2
MASKED = (3, 10)


def child():
    for p in (ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import torch
    import torch.distributed as dist

    import update_reference as R
    from oracle import sigkernel_oracle as O
    from sigsvgd_amd.distributed import ShardedSigSVGD

    gpu = torch.device("cuda:0")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = "29577"
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=gpu)
    try:
        X, score = O.synthetic_inputs(N, T, D)
        mask = torch.ones(N, T, 1)
        mask[list(MASKED)] = 0.0
        mask[:, 0] = 0.0
        np64 = lambda t: t.detach().double().cpu().numpy()
        tensors = lambda sd: {k: np64(t) for k, t in sd.items() if isinstance(t, torch.Tensor)}
        zero = np.zeros((N, T * D))
        for mode, m in (("adam", mask), ("adagrad", None)):
            sh = ShardedSigSVGD(1.0, LR, update=mode, mask=None if m is None else m.to(gpu))
            Xs, sg = X.to(gpu), score.to(gpu)
            for k in range(STEPS):
                before = tensors(sh.state_dict()) or ({"adagrad": zero} if mode == "adagrad" else
                                                      {"exp_avg": zero, "exp_avg_sq": zero})
                Xn = sh.step(Xs, sg)
                assert sh.last_route == "partial" and Xn.data_ptr() != Xs.data_ptr()
                x, v = np64(Xs), np64(sh.last_v_rows)
                K, gk = O.gram_backward(x, x, None, O.RBF, 1.0, 0)
                v_ref = O.svgd_velocity(K, score.numpy(), gk)
                rel = np.abs(v - v_ref).max() / np.abs(v_ref).max()
                print(f"{mode} step {k}: velocity error {rel:.3e} of its largest entry")
                assert rel < 1e-5
                sd = sh.state_dict()
                assert sd["step"] == k + 1 and sd["update"] == mode
                R.check_update(mode, np64(Xn), tensors(sd), v, x, LR, None if m is None else m.numpy(), before, k,
                               where=f"step {k}")
                if m is not None:
                    assert torch.equal(Xn[list(MASKED)], Xs[list(MASKED)]) and torch.equal(Xn[:, 0], Xs[:, 0])
                    assert not torch.equal(Xn[0, 1:], Xs[0, 1:])
                Xs = Xn
    finally:
        dist.destroy_process_group()
    print("child ok")


@pytest.mark.gpu
def test_sharded_update_rules_on_rccl_single_rank(gpu):
    p = subprocess.run([sys.executable, "-s", os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(p.stdout)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


if __name__ == "__main__":
    child()
