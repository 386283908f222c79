"""The sharded step's update rules under gloo (world sizes 2 and 4): manual + mask, Adagrad, Adagrad + mask, Adam and
Adam + mask on the rank's own rows behind the reduce-scatter (the partial route), and Adam + mask and Adagrad on the row-wise
route (`rowwise=True`: the other caller of the same update), three consecutive steps each, with oracle-backed doubles for the
per-rank compute (as tests/test_distributed_cpu.py) and a torch restatement of `ops.svgd_update` as `update_fn`.

The reference is one process in fp64 (tests/update_reference.py says why it is built this way): every step's reduced
velocity against `oracle.svgd_velocity` on the gathered particles of that step, within the project's phi tolerance (1e-5 of
its largest entry), and every step's new particles and state against torch.optim.Adam / the reference's
two Adagrad lines applied to that velocity, within the rounding of one fp32 update.  Every row of a masked particle stays
exactly where it was, and a run resumed from `state_dict()` continues exactly as the uninterrupted one."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N, T, D, STEPS, LR = 8, 5, 2, 3, 0.05
# name -> (update, masked, row-wise route)
CONFIGS = {"manual+mask": ("manual", True, False), "adagrad": ("adagrad", False, False),
           "adagrad+mask": ("adagrad", True, False), "adam": ("adam", False, False), "adam+mask": ("adam", True, False),
           "adam+mask rowwise": ("adam", True, True), "adagrad rowwise": ("adagrad", False, True)}
MASKED = (1, N - 1)  # particles that must not move; every path also keeps its first point (TrajectorySVGD's gradient_mask)


def global_mask():
    m = torch.ones(N, T, 1)
    m[list(MASKED)] = 0.0
    m[:, 0] = 0.0
    return m


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import helpers
        import update_reference as R
        from oracle import sigkernel_oracle as O
        from sigsvgd_amd.distributed import ShardedSigSVGD, shard_rows

        X, score = O.synthetic_inputs(N, T, D)
        r0, r1 = shard_rows(N, rank, world)

        def make(mode, masked, **kw):
            return ShardedSigSVGD(1.0, LR, partial_fn=helpers.gram_sym_partial,
                                  phi_fn=lambda K, s, gk: helpers.svgd_phi(K, s, gk),
                                  rows_fn=lambda Xs_, Xf, ih: helpers.gram_fwd_bwd(Xs_, Xf, ih), update=mode,
                                  mask=global_mask()[r0:r1] if masked else None, update_fn=R.torch_update, **kw)

        tensors = lambda sd: {k: t.numpy().copy() for k, t in sd.items() if isinstance(t, torch.Tensor)}
        out = {}
        for name, (mode, masked, rowwise) in CONFIGS.items():
            sh, Xs, steps, sd2 = make(mode, masked, rowwise=rowwise), X[r0:r1].clone(), [], None
            for k in range(STEPS):
                before = tensors(sh.state_dict())
                Xn = sh.step(Xs, score[r0:r1])
                steps.append(dict(x=Xs.numpy().copy(), v=sh.last_v_rows.numpy().copy(), x_new=Xn.numpy().copy(),
                                  state=before, state_new=tensors(sh.state_dict())))
                Xs = Xn
                if k == 1:
                    sd2, X2 = sh.state_dict(), Xs.clone()
            # resume: the state after two steps into a new object, then the third step
            assert sd2["step"] == 2 and sd2["update"] == mode and sd2["world_size"] == world and sd2["rank"] == rank
            sh2 = make(mode, masked, rowwise=rowwise)
            sh2.load_state_dict(sd2)
            X3 = sh2.step(X2, score[r0:r1])
            resumed = dict(x=X3.numpy().copy(), state=tensors(sh2.state_dict()), step=sh2.state_dict()["step"])
            refused = []
            for bad in (dict(sd2, world_size=world + 1), dict(sd2, update="adam" if mode != "adam" else "adagrad")):
                try:
                    make(mode, masked).load_state_dict(bad)
                    refused.append(False)
                except ValueError:
                    refused.append(True)
            out[name] = dict(steps=steps, resumed=resumed, refused=refused, route=sh.last_route)
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


_RUNS = {}


def run(world):
    """all configurations on `world` ranks, once per session: {config: [per rank: dict]}"""
    if world in _RUNS:
        return _RUNS[world]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + (os.getpid() % 1000) + world
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = []
    for _ in range(world):  # (a rank that raised never puts: fail as soon as one has exited non-zero)
        for _ in range(300):
            try:
                outs.append(q.get(timeout=1))
                break
            except Exception:
                assert all(p.exitcode in (None, 0) for p in procs), [p.exitcode for p in procs]
        else:
            raise AssertionError("timeout waiting for the ranks")
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    outs.sort(key=lambda t: t[0])
    _RUNS[world] = {name: [o[1][name] for o in outs] for name in CONFIGS}
    return _RUNS[world]


_VELOCITY = {}


def oracle_velocity(Xfull):
    """`oracle.svgd_velocity` on the gathered particles (fp64), computed once per distinct particle set"""
    from oracle import sigkernel_oracle as O

    key = Xfull.tobytes()
    if key not in _VELOCITY:
        _, score = O.synthetic_inputs(N, T, D)
        K, gk = O.gram_backward(Xfull, Xfull, None, O.RBF, 1.0, 0)
        _VELOCITY[key] = O.svgd_velocity(K, score.numpy(), gk)
    return _VELOCITY[key]


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_sharded_update_matches_the_reference(world, config):
    import update_reference as R

    mode, masked, rowwise = CONFIGS[config]
    ranks = run(world)[config]
    per = N // world
    mask = global_mask().numpy().astype(np.float64) if masked else None
    for k in range(STEPS):
        Xfull = np.concatenate([r["steps"][k]["x"] for r in ranks], axis=0)
        v_ref = oracle_velocity(Xfull)
        v_got = np.concatenate([r["steps"][k]["v"] for r in ranks], axis=0).astype(np.float64)
        rel = np.abs(v_got - v_ref).max() / np.abs(v_ref).max()
        print(f"world {world} {config} step {k}: velocity error {rel:.3e} of its largest entry")
        assert rel < 1e-5  # last_v_rows is the reduced velocity BEFORE the mask
        for r, out in enumerate(ranks):
            s = out["steps"][k]
            m = None if mask is None else mask[r * per:(r + 1) * per]
            R.check_update(mode, s["x_new"], s["state_new"], s["v"], s["x"], LR, m, s["state"] or _zero_state(mode, s["v"]),
                           k, where=f"world {world} rank {r} step {k}")
            if masked:  # exactly: x - lr * 0, and 0 / (0 + eps) under Adam, 0 / sqrt(1e-12) under Adagrad
                own = [i - r * per for i in MASKED if r * per <= i < (r + 1) * per]
                assert np.array_equal(s["x_new"][own], s["x"][own])
                assert np.array_equal(s["x_new"][:, 0], s["x"][:, 0])
    if masked:  # over the whole run
        X0 = np.concatenate([r["steps"][0]["x"] for r in ranks], axis=0)
        X3 = np.concatenate([r["steps"][-1]["x_new"] for r in ranks], axis=0)
        assert np.array_equal(X3[list(MASKED)], X0[list(MASKED)]) and not np.array_equal(X3[0, 1:], X0[0, 1:])
    assert all(r["route"] == ("rowwise" if rowwise else "partial") for r in ranks)  # both ends of the update call


def _zero_state(mode, v):
    z = np.zeros((v.shape[0], v[0].size))
    return {"adagrad": z} if mode == "adagrad" else {"exp_avg": z, "exp_avg_sq": z} if mode == "adam" else {}


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_resumed_run_continues_exactly(world, config):
    for out in run(world)[config]:
        last = out["steps"][-1]
        assert np.array_equal(out["resumed"]["x"], last["x_new"])
        assert out["resumed"]["step"] == STEPS
        assert out["resumed"]["state"].keys() == last["state_new"].keys()
        for k, t in last["state_new"].items():
            assert np.array_equal(out["resumed"]["state"][k], t)
        assert out["refused"] == [True, True]  # another world size, another mode: ValueError


def test_update_argument_is_checked():
    from sigsvgd_amd.distributed import ShardedSigSVGD

    with pytest.raises(ValueError):
        ShardedSigSVGD(1.0, 0.05, update="sgd")
