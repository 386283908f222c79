"""`svgd_phi_kernel` (csrc/svgd_phi.hip) per entry against the fp64 reference, at its tile, stage and alignment edges.

The kernel is v = -((K @ score - grad_k)/N) on the fp32 MFMA with the mask, Adagrad, Adam and X - lr*v epilogues, behind
`ops.svgd_phi`, `ops.svgd_adam` and each rank's velocity of the sharded step.  tests/phi_reference.py has the inputs, the
reference and the derived per-entry bound (`assert_phi`), tests/test_phi_reference_cpu.py shows on the CPU that the bound
rejects a kernel that loses, repeats or misplaces one term; tests/update_reference.py has the update rules' reference and
rounding bounds (`check_update`).  Four groups:

(a) The product, every entry within its bound, in the integer form (exact sums: a zero reference must give a zero, a power
    of two N the reference itself) and the float form.  Shapes (N, D) and the edge each is there for -- a workgroup owns 32
    rows by 64 columns, k runs in stages of 64 in four wavefront quarters of 16 and MFMA steps of 4, and the next stage is
    fetched under k0 + 64 < N; 16-byte fetches of K need N % 4 == 0, of score D % 4 == 0:
      (1, 1)      one entry, one k: everything else of the tile, the stage and the fetch is padding
      (3, 3)      scalar fetch, k short of one MFMA step
      (4, 4)      one full 16-byte fetch of each operand, one MFMA step, three quarters of the stage empty
      (5, 3)      first k behind a 16-byte group, scalar; the smallest shape of tests/test_gpu_update.py
      (15, 1)     one short of a quarter; a single column
      (16, 64)    exactly one quarter; a full column tile; 16-byte fetch of both
      (17, 65)    first k of the second quarter; first column of a second column tile, scalar
      (31, 4)     one short of a row tile; scalar K with a 16-byte score
      (32, 128)   exactly one row tile, two full column tiles, half a stage
      (33, 70)    first row of a second row tile; partial second column tile with D % 4 = 2
      (63, 63)    one short of tile and stage in every direction
      (64, 64)    exactly one stage: the prefetch test k0 + 64 < N is false at its boundary
      (65, 63)    a second stage of one k (scalar), prefetched once
      (65, 65)    the same with a second column tile of one column
      (68, 68)    N % 4 == 0 with a partial stage of 4: the 16-byte fetch's tail guard gc + 3 < N; D % 4 == 0 with a
                  partial column tile of 4
      (68, 132)   the same stage tail with a third column tile of 4 columns
      (100, 132)  16-byte fetches, partial stage of 36 (two quarters full, one of 4), partial row and column tiles
      (127, 3)    one short of two stages; three columns
      (128, 128)  two full stages, full tiles: the last prefetch is the last stage
      (128, 132)  the same with a 4-column third tile (aligned pointers, for (b))
      (129, 63)   a third stage of one k behind two full ones; fifth row tile of one row
      (132, 4)    a third stage of one 16-byte group; one 16-byte group of columns
      (132, 68)   both at once
      (196, 70)   four stages, the last of 4; scalar score
      (260, 132)  five stages, nine row tiles, three column tiles, the last of each partial
      (1024, 448) the benchmark's, integer form only (N a power of two: exact)
(b) The fetch form: K, score, both, then grad_k / mask / X on pointers 4, 8 and 12 bytes off the 16-byte grid.  Only the
    loads differ, so the result has the aligned launch's bits.
(c) Nothing outside [N, D]: every output between seeded guards that must keep their bits, every input between NaN areas
    that no result may meet (the zero padding does not absorb a NaN), through `ops._launch` on pointers into buffers the
    test owns.
(d) The fused epilogues, and `ops.svgd_update` on the same velocities, per entry against `check_update` -- driven by the
    velocity the kernel itself produced (pinned in (a) and again here), for the reason the docstring of update_reference.py
    gives -- over three steps, with and without a mask, out of place and in place."""
import numpy as np
import pytest
import torch

import phi_reference as P
import update_reference as R
from oracle import sigkernel_oracle as O
from parity import rel_max
from phi_reference import BENCH_SHAPE, SEED, SHAPES

pytestmark = pytest.mark.gpu

LR, STEPS = 0.05, 3
MODES = ("manual", "adagrad", "adam")
_CACHE = {}


def inputs(N, D, form, gpu, seed=SEED):
    """(numpy arrays of `phi_inputs`, the same on the device), made once per shape, form and seed"""
    key = (N, D, form, seed)
    if key not in _CACHE:
        arrays = P.phi_inputs(N, D, seed, form)
        _CACHE[key] = (arrays, tuple(torch.as_tensor(a, device=gpu) for a in arrays))
    return _CACHE[key]


def host(t):
    return t.detach().cpu().numpy()


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", P.FORMS)
@pytest.mark.parametrize("N,D", SHAPES)
def test_product_per_entry(gpu, N, D, form):
    from sigsvgd_amd import ops

    (K, s, gk, _, _), (Kg, sg, gkg, _, _) = inputs(N, D, form, gpu)
    v = ops.svgd_phi(Kg, sg, gkg)
    assert v.shape == (N, D) and v.dtype == torch.float32
    P.assert_phi(host(v), K, s, gk, form, "svgd_phi")


def test_product_per_entry_at_the_benchmark_shape(gpu):
    from sigsvgd_amd import ops

    N, D = BENCH_SHAPE
    (K, s, gk, _, _), (Kg, sg, gkg, _, _) = inputs(N, D, "integer", gpu)
    assert P.assert_phi(host(ops.svgd_phi(Kg, sg, gkg)), K, s, gk, "integer", "svgd_phi") == 0.0


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
def shifted(t, off):
    """a contiguous copy of `t` whose data_ptr() is `off` bytes past a multiple of 16, inside a larger flat buffer"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    first = ((off - buf.data_ptr()) % 16) // 4
    out = buf[first:first + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == off and out.is_contiguous()
    return out


@pytest.fixture
def launches(monkeypatch):
    """the argument tuples `ops` hands to the library, in order"""
    from sigsvgd_amd import ops

    seen, launch = [], ops._launch

    def spy(dev, name, args, *a, **k):
        seen.append((name, tuple(args)))
        return launch(dev, name, args, *a, **k)

    monkeypatch.setattr(ops, "_launch", spy)
    return seen


@pytest.mark.parametrize("off", [4, 8, 12])
@pytest.mark.parametrize("which", ["K", "score", "both", "rest"])
@pytest.mark.parametrize("N,D", [(68, 68), (128, 132)])
def test_fetch_form(gpu, launches, N, D, which, off):
    from sigsvgd_amd import ops

    assert N % 4 == 0 and D % 4 == 0
    for form in P.FORMS:
        (K, s, gk, mask, _), (Kg, sg, gkg, mg, Xg) = inputs(N, D, form, gpu)
        assert all(t.data_ptr() % 16 == 0 for t in (Kg, sg, gkg, mg, Xg))
        del launches[:]
        if which == "rest":  # the epilogue's operands: scalar loads whatever the pointer
            v0, X0 = ops.svgd_phi(Kg, sg, gkg, mask=mg, X=Xg, lr=LR)
            gk1, m1, X1 = shifted(gkg, off), shifted(mg, off), shifted(Xg, off)
            v1, Xn1 = ops.svgd_phi(Kg, sg, gk1, mask=m1, X=X1, lr=LR)
            args = launches[1][1]
            assert (args[2], args[3], args[7]) == (gk1.data_ptr(), m1.data_ptr(), X1.data_ptr())
            assert torch.equal(Xn1, X0) and not torch.equal(X0, Xg)
            P.assert_phi(host(v1), K, s, gk, form, f"grad_k, mask, X at {off} mod 16", mask=mask)
        else:
            v0 = ops.svgd_phi(Kg, sg, gkg)
            K1 = shifted(Kg, off) if which in ("K", "both") else Kg
            s1 = shifted(sg, off) if which in ("score", "both") else sg
            v1 = ops.svgd_phi(K1, s1, gkg)
            args = launches[1][1]
            assert (args[0], args[1]) == (K1.data_ptr(), s1.data_ptr())  # passed on as they came, no copy
            P.assert_phi(host(v1), K, s, gk, form, f"{which} at {off} mod 16")
        assert [name for name, _ in launches] == ["svgd_step", "svgd_step"]
        assert torch.equal(v1, v0)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
def guard_floats(N, D):
    return 32 * max(N, D, 64) + 64  # one tile of rows at the launch's longest row (K's or an [N, D] operand's), and a little


class Fenced:
    """[guard | interior | guard] in one allocation, each guard of `g` floats; the interior is what a launch is given.
    Guards: seeded bits kept in a copy (`intact`), or NaN."""

    def __init__(self, interior, g, seed=None):
        n = interior.numel()
        if seed is None:
            self.buf = torch.full((2 * g + n,), float("nan"), dtype=torch.float32, device=interior.device)
        else:
            gen = torch.Generator().manual_seed(seed)
            bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (2 * g + n,), dtype=torch.int32, generator=gen)
            self.buf = bits.to(interior.device).view(torch.float32)
        self.g, self.n = g, n
        self.t = self.buf[g:g + n].view(interior.shape)
        self.t.copy_(interior)
        self.copy = self.buf.view(torch.int32).clone()
        assert self.t.data_ptr() % 16 == interior.data_ptr() % 16 == 0  # the fetch form of the ordinary launch

    def intact(self):
        now, g, n = self.buf.view(torch.int32), self.g, self.n
        return torch.equal(now[:g], self.copy[:g]) and torch.equal(now[g + n:], self.copy[g + n:])


def direct_launch(ops, gpu, mode, N, D, K, s, gk, mask, v, X_in, X_out, state, step):
    """the fused launch of `mode` through `ops._launch` on the tensors given (interiors of `Fenced` buffers)"""
    head = (K.data_ptr(), s.data_ptr(), gk.data_ptr(), mask.data_ptr(), N, D, v.data_ptr(), X_in.data_ptr(), X_out.data_ptr())
    if mode == "adam":
        ops._launch(gpu, "svgd_adam_step", (*head, LR, 0.9, 0.999, 1e-8, state[0].data_ptr(), state[1].data_ptr(),
                                            step.data_ptr()))
    else:
        ops._launch(gpu, "svgd_step", (*head, LR, state[0].data_ptr() if mode == "adagrad" else None))


def ordinary_launch(ops, gpu, mode, I, state0):
    """-> (v, X_new, state tensors) of the ordinary `ops` call on the inputs `I`, the state starting from `state0`; Adam's
    counter at 2"""
    Kg, sg, gkg, mg, Xg = I
    if mode == "adam":
        st = ops.AdamState(Xg)
        st.exp_avg.copy_(state0[0]), st.exp_avg_sq.copy_(state0[1]), st.step.fill_(2)
        st.t_host = 2
        v, Xn = ops.svgd_adam(Kg, sg, gkg, Xg, LR, st, mask=mg)
        assert int(st.step) == 3
        return v, Xn, (st.exp_avg, st.exp_avg_sq)
    ag = state0[0].clone() if mode == "adagrad" else None
    v, Xn = ops.svgd_phi(Kg, sg, gkg, mask=mg, X=Xg, lr=LR, adagrad_state=ag)
    return v, Xn, (ag,) if mode == "adagrad" else ()


def starting_state(mode, N, D, gpu):
    """a state in mid-run: seeded, positive second moments"""
    gen = torch.Generator().manual_seed(1000 * N + D)
    a, b = torch.randn(N, D, generator=gen).to(gpu), (torch.rand(N, D, generator=gen) + 0.1).to(gpu)
    return {"manual": (), "adagrad": (b,), "adam": (0.1 * a, 0.01 * b)}[mode]


@pytest.mark.parametrize("side", ["writes", "reads"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,D", [(33, 70), (65, 63), (68, 132)])
def test_nothing_outside_the_operands(gpu, N, D, mode, side):
    """writes: v_out, X_out and the state between seeded guards, unchanged afterwards bit for bit.  reads: K, score, grad_k,
    mask and X_in between NaN areas; no output meets one.  Either way the interiors equal the ordinary launch's."""
    from sigsvgd_amd import ops

    _, I = inputs(N, D, "float", gpu)
    state0 = starting_state(mode, N, D, gpu)
    v0, X0, st0 = ordinary_launch(ops, gpu, mode, I, state0)
    step = torch.full((), 2, dtype=torch.int32, device=gpu)
    g = guard_floats(N, D)
    if side == "writes":
        outs = [Fenced(torch.zeros(N, D, device=gpu), g, seed=11), Fenced(torch.zeros(N, D, device=gpu), g, seed=12)]
        state = [Fenced(t, g, seed=13 + i) for i, t in enumerate(state0)]
        ins = list(I)
    else:
        outs = [torch.zeros(N, D, device=gpu), torch.zeros(N, D, device=gpu)]
        state = [t.clone() for t in state0]
        fences = [Fenced(t, g) for t in I]
        assert all(bool(torch.isnan(f.buf[:g]).all()) and bool(torch.isnan(f.buf[-g:]).all()) for f in fences)
        ins = [f.t for f in fences]
    t = lambda f: f.t if isinstance(f, Fenced) else f
    direct_launch(ops, gpu, mode, N, D, *ins[:4], t(outs[0]), ins[4], t(outs[1]), [t(f) for f in state], step)
    torch.cuda.synchronize(gpu)
    if side == "writes":
        names = ["v_out", "X_out"] + {"manual": [], "adagrad": ["adagrad"], "adam": ["exp_avg", "exp_avg_sq"]}[mode]
        for name, f in zip(names, outs + state):
            assert f.intact(), f"{name}: a guard changed"
    got = [t(outs[0]), t(outs[1])] + [t(f) for f in state]
    for name, a, b in zip(["v", "X", "state", "state 2"], got, [v0, X0, *st0]):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b), name
    assert int(step) == (3 if mode == "adam" else 2)
    assert not torch.equal(got[1], I[4])


# ---- (d) ---------------------------------------------------------------------------------------------------------------------
def state_arrays(mode, state):
    if mode == "adagrad":
        return {"adagrad": host(state).astype(np.float64)}
    if mode == "adam":
        return {"exp_avg": host(state.exp_avg).astype(np.float64), "exp_avg_sq": host(state.exp_avg_sq).astype(np.float64)}
    return {}


def new_state(ops, mode, X):
    return torch.zeros_like(X) if mode == "adagrad" else ops.AdamState(X) if mode == "adam" else None


def same_state(mode, a, b):
    if mode == "adagrad":
        return torch.equal(a, b)
    if mode == "adam":
        return torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq) and int(a.step) == int(b.step)
    return True


EPILOGUE_SHAPES = [(5, 3), (33, 70), (68, 132), (129, 63)]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,D", EPILOGUE_SHAPES)
def test_fused_epilogues_per_entry(gpu, N, D, mode, masked):
    from sigsvgd_amd import ops

    (_, _, _, mask, X0), (Kg, _, _, mg, Xg0) = inputs(N, D, "float", gpu)
    K = host(Kg)
    m, mgpu = (mask, mg) if masked else (None, None)
    Xo, Xi = Xg0.clone(), Xg0.clone()  # out of place, in place
    so, si = new_state(ops, mode, Xg0), new_state(ops, mode, Xg0)
    for k in range(STEPS):
        (_, s, gk, _, _), (_, sg, gkg, _, _) = inputs(N, D, "float", gpu, seed=SEED + k)
        v_raw = ops.svgd_phi(Kg, sg, gkg)
        P.assert_phi(host(v_raw), K, s, gk, "float", f"step {k}")
        Xprev, x_before, before = Xo, host(Xo).astype(np.float64), state_arrays(mode, so)
        if mode == "adam":
            vo, Xo = ops.svgd_adam(Kg, sg, gkg, Xo, LR, so, mask=mgpu)
            vi, Xr = ops.svgd_adam(Kg, sg, gkg, Xi, LR, si, mask=mgpu, inplace=True)
            assert int(so.step) == k + 1
        else:
            vo, Xo = ops.svgd_phi(Kg, sg, gkg, mask=mgpu, X=Xo, lr=LR, adagrad_state=so)
            vi, Xr = ops.svgd_phi(Kg, sg, gkg, mask=mgpu, X=Xi, lr=LR, adagrad_state=si, inplace=True)
        R.check_update(mode, host(Xo), state_arrays(mode, so), host(v_raw), x_before, LR, m, before, k,
                       where=f"fused ({N}, {D}) step {k}", got_v=host(vo))
        assert Xr is Xi and torch.equal(Xi, Xo) and torch.equal(vi, vo) and same_state(mode, si, so)
        if masked:
            still = mg == 0
            assert bool(still.any()) and not bool(still.all()) and torch.equal(Xo[still], Xprev[still])
    assert bool(torch.isfinite(Xo).all()) and not torch.equal(Xo, Xg0)
    if masked:
        assert torch.equal(Xo[mg == 0], Xg0[mg == 0])


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,D", EPILOGUE_SHAPES)
def test_update_kernel_per_entry(gpu, N, D, mode, masked):
    """`svgd_update_kernel` on the same velocities: the per-entry evidence tests/test_gpu_distributed_update.py has at
    (16, 24) inside its RCCL child, here at the partial-tile shapes (D = 132: its 16-byte path; the others: one element per
    access)"""
    from sigsvgd_amd import ops

    (_, _, _, mask, _), (Kg, _, _, mg, Xg0) = inputs(N, D, "float", gpu)
    m, mgpu = (mask, mg) if masked else (None, None)
    Xu, su = Xg0.clone(), new_state(ops, mode, Xg0)
    for k in range(STEPS):
        _, (_, sg, gkg, _, _) = inputs(N, D, "float", gpu, seed=SEED + k)
        v_raw = ops.svgd_phi(Kg, sg, gkg)
        x_before, before = host(Xu).astype(np.float64), state_arrays(mode, su)
        kw = dict(adam=su) if mode == "adam" else dict(adagrad_state=su)
        vu, Xu = ops.svgd_update(v_raw, Xu, LR, mask=mgpu, **kw)
        R.check_update(mode, host(Xu), state_arrays(mode, su), host(v_raw), x_before, LR, m, before, k,
                       where=f"update ({N}, {D}) step {k}", got_v=host(vu))
    if masked:
        assert torch.equal(Xu[mg == 0], Xg0[mg == 0])


# ---- the round-1 smoke comparison of the velocity kernel, moved here unchanged from tests/test_gpu_generic.py -----------------
TOL = 1e-5  # north_star: within 1e-5 relative fp32


def test_phi(gpu):
    from sigsvgd_amd import ops

    rng = np.random.default_rng(0)
    for N, D in [(16, 40), (100, 20), (128, 224), (257, 65)]:
        K = rng.standard_normal((N, N)).astype(np.float32)
        s = rng.standard_normal((N, D)).astype(np.float32)
        gk = rng.standard_normal((N, D)).astype(np.float32)
        m = (rng.random((N, D)) > 0.3).astype(np.float32)
        X = rng.standard_normal((N, D)).astype(np.float32)
        vref = O.svgd_velocity(K, s, gk, m)
        v, Xn = ops.svgd_phi(*(torch.as_tensor(t, device=gpu) for t in (K, s, gk, m)), X=torch.as_tensor(X, device=gpu), lr=0.1)
        assert rel_max(v.cpu().numpy(), vref) < TOL
        assert rel_max(Xn.cpu().numpy(), X - 0.1 * vref) < TOL
        v2 = ops.svgd_phi(*(torch.as_tensor(t, device=gpu) for t in (K, s, gk)))
        assert rel_max(v2.cpu().numpy(), O.svgd_velocity(K, s, gk)) < TOL
