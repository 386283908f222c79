"""The vector kernels per entry against the fp64 reference, at their tile, stage, split and alignment edges: `vec_fused_kernel`
(csrc/vec_fused.hip) behind `ops.vec_kernel_fused`, `vec_sqdist_kernel` and `vec_kgrad_kernel` (csrc/vec_kernels.hip) behind
`ops.vec_sqdist` and `ops.vec_kernel`, and the routing of the drop-in classes between them.

tests/vec_reference.py has the inputs (integer form: exact sums, the `unit` kind must EQUAL the reference; float form: every
channel term far above the bound), the references, the derived per-entry bounds and `assert_vec`;
tests/test_vec_reference_cpu.py shows on the CPU that the bounds reject a kernel that loses, repeats or misplaces one term.

(a) Fused kernel, every entry of K and dK within its bound, with and without a metric, in the three output selections
    (K and dK; K only -- every column tile its own workgroup; dK only) and on both reduction routes (workspace: the same
    bits twice; atomics: the same bound, so equality in the integer / unit form).  Shapes (A, B, D) and their edges:
      (65, 70, D)      D = 1, 3, 4 one partial stage, scalar and 16-byte fetch;  31, 32, 33 either side of a metric stage;
                       63, 64, 65 either side of a plain stage and of NT = 4 -> 8;  127, 128, 129 NT = 8 -> 16;
                       255, 256, 257 NT = 16 -> 32;  508, 511, 512 the last 16-byte group, the last channel, the limit
      A in 1, 15, 16, 17, 63, 64, 65, 129 paired with B in 1, 63, 64, 65, 127, 128, 129, 193 (two pairings) at D = 5 and 68:
                       one row, a wavefront's 16 rows and its neighbours, a row tile and its neighbours, three row tiles;
                       one partner, a column tile and its neighbours, two and their neighbours, four tiles
      (64, 65, D)      two splits of one tile, the second a single column: b_j and W mostly padding
      (4097, 641, D)   65 row tiles: 8 splits wanted, 11 column tiles: 2 a workgroup, 6 splits, the last owning ONE tile --
                       stage buffers, wt and bn reused across tiles, a_i from the first tile only, the join of six partials
(b) The fetch form: X, Y, XM, YM each 4, 8 and 12 bytes off the 16-byte grid at D = 64 and 68 (only the pointer clears VEC4):
    the bits of the aligned launch.
(c) Nothing outside the operands, through the C entry point: K and dK between seeded guards, the workspace guarded and
    NaN-filled, the inputs between NaN areas.
(d) Two-launch path: `vec_sqdist` at its 64 x 64 tile and 16-channel stage edges, `vec_kernel` at its 16-row, 64-partner and
    64-channel block edges (K complete with 1, 2 and 3 channel blocks), fp32 and, on a third of the shapes, fp64.
(e) Routing of the drop-in classes: D = 513 and fp64 go to the two launches, D = 512 fp32 with h given to the fused one."""
import ctypes

import numpy as np
import pytest
import torch

import vec_reference as V
from guarded_workspace import GuardedWorkspace
from vec_reference import SEED

pytestmark = pytest.mark.gpu

_CACHE, _EXPECTED = {}, {}
MEASURED_F = {}  # path, kind -> the largest function error seen, in ulps (printed by every test that adds to it)


class Dev:
    pass


def inputs(A, B, D, form, metric, gpu, dtype=torch.float32):
    key = (A, B, D, form, metric, dtype)
    if key not in _CACHE:
        inp, d = V.vec_inputs(A, B, D, SEED, form, metric), Dev()
        for name in ("X", "Y", "go", "XM", "YM"):
            a = getattr(inp, name)
            setattr(d, name, None if a is None else torch.as_tensor(a, device=gpu).to(dtype))
        d.GXM, d.GYM = (d.XM, d.YM) if metric else (d.X, d.Y)
        _CACHE[key] = (inp, d)
    return _CACHE[key]


def expected(inp, kind, path, fp64=False, weighted=True):
    key = (id(inp), kind, path, fp64, weighted, inp.grad_scale)
    if key not in _EXPECTED:
        _EXPECTED[key] = V.expected(inp, kind, path, fp64=fp64, weighted=weighted)
    return _EXPECTED[key]


def host(t):
    return t.detach().cpu().numpy()


def kind_code(kind):
    from sigsvgd_amd import _lib

    return {"unit": _lib.VEC_UNIT, "gaussian": _lib.VEC_GAUSSIAN, "imq": _lib.VEC_IMQ}[kind]


def kinds_of(form):
    return ("unit", "gaussian", "imq") if form == "integer" else ("gaussian", "imq")


def note_f(path, kind, K, e, u=V.U32):
    """the function error of K on an exact sq, recorded and printed (the measurement behind `vec_reference.F_ULPS`)"""
    f = V.function_error_ulps(host(K), e.sq, kind, e.hh, u)
    MEASURED_F[(path, kind)] = max(MEASURED_F.get((path, kind), 0.0), f)
    print(f"function error {path} {kind}: {f:.2f} ulps here, {MEASURED_F[(path, kind)]:.2f} so far")


def fused(ops, inp, d, kind, hh, **kw):
    return ops.vec_kernel_fused(d.X, d.Y, kind_code(kind), 2 * hh, inp.grad_scale, XM=d.XM, YM=d.YM, grad_out=d.go, **kw)


def check_fused(inp, kind, K, dK, where, grad=True):
    e = expected(inp, kind, "fused")
    worst = 0.0
    if K is not None:
        worst = V.assert_vec(host(K), e.K, e.e_K, where, "K", V.fused_geometry(inp.A, inp.B, grad)["per"])
    if dK is not None:
        worst = max(worst, V.assert_vec(host(dK), e.dK, e.e_dK, where, "dK"))
    return worst


def fused_workspace_splits(A, B, D):
    """the column splits of a gradient launch, from the library's own workspace query"""
    from sigsvgd_amd import ops

    n = ctypes.c_size_t(0)
    ops._query("vec_fused_workspace_bytes", (A, B, D), (n,))
    assert n.value == V.fused_workspace_bytes(A, B, D)
    return (n.value - 256) // (A * D * 4) if n.value else 1


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [False, True], ids=["plain", "metric"])
@pytest.mark.parametrize("A,B,D", V.FUSED_D_SHAPES + V.FUSED_AB_SHAPES)
def test_fused_per_entry(gpu, A, B, D, metric):
    from sigsvgd_amd import ops

    assert fused_workspace_splits(A, B, D) == V.fused_geometry(A, B)["splits"]
    for form in V.FORMS:
        inp, d = inputs(A, B, D, form, metric, gpu)
        hh = V.half_inv_h2(D, metric)
        for kind in kinds_of(form):
            where = f"fused ({A}, {B}, {D}) {'metric' if metric else 'plain'} {form} {kind}"
            K, dK = fused(ops, inp, d, kind, hh)
            assert K.shape == (A, B) and dK.shape == (A, D) and K.dtype == dK.dtype == torch.float32
            if form == "integer" and kind != "unit":
                note_f("fused", kind, K, expected(inp, kind, "fused"))
            worst = check_fused(inp, kind, K, dK, where)
            assert worst == 0.0 or not (form == "integer" and kind == "unit")
            K2, dK2 = fused(ops, inp, d, kind, hh)
            assert torch.equal(K2, K) and torch.equal(dK2, dK), "workspace route: not the same bits twice"
            Ko, none = fused(ops, inp, d, kind, hh, want_grad=False)  # every column tile its own workgroup
            assert none is None
            check_fused(inp, kind, Ko, None, where + ", K only", grad=False)
            none, dKo = fused(ops, inp, d, kind, hh, want_K=False)
            assert none is None and torch.equal(dKo, dK), "dK only: not the bits of the joint launch"
            Ka, dKa = fused(ops, inp, d, kind, hh, reproducible=False)
            assert torch.equal(Ka, K)
            check_fused(inp, kind, None, dKa, where + ", atomics")


@pytest.mark.parametrize("metric", [False, True], ids=["plain", "metric"])
@pytest.mark.parametrize("A,B,D", V.FUSED_BIG_SHAPES)
def test_fused_several_tiles_per_workgroup_and_a_short_last_split(gpu, A, B, D, metric):
    from sigsvgd_amd import ops

    g = V.fused_geometry(A, B)
    assert fused_workspace_splits(A, B, D) == g["splits"] == 6 and g["per"] == 2 and g["ntile"] == 11  # the last split owns one tile
    for form, kind in (("integer", "unit"), ("float", "gaussian")):
        inp, d = inputs(A, B, D, form, metric, gpu)
        hh = V.half_inv_h2(D, metric)
        where = f"fused ({A}, {B}, {D}) {'metric' if metric else 'plain'} {form} {kind}"
        K, dK = fused(ops, inp, d, kind, hh)
        worst = check_fused(inp, kind, K, dK, where)
        assert worst == 0.0 or form == "float"
        K2, dK2 = fused(ops, inp, d, kind, hh)
        assert torch.equal(K2, K) and torch.equal(dK2, dK)
        Ka, dKa = fused(ops, inp, d, kind, hh, reproducible=False)
        assert torch.equal(Ka, K)
        check_fused(inp, kind, None, dKa, where + ", atomics")


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


@pytest.mark.parametrize("metric", [False, True], ids=["plain", "metric"])
@pytest.mark.parametrize("A,B,D", V.FUSED_ALIGN_SHAPES)
def test_fused_fetch_form(gpu, launches, A, B, D, metric):
    from sigsvgd_amd import ops

    assert D % 4 == 0
    for form, kind in (("integer", "unit"), ("float", "gaussian")):
        inp, d = inputs(A, B, D, form, metric, gpu)
        hh = V.half_inv_h2(D, metric)
        names = ("X", "Y", "XM", "YM") if metric else ("X", "Y")
        assert all(getattr(d, n).data_ptr() % 16 == 0 for n in names)
        K0, dK0 = fused(ops, inp, d, kind, hh)
        check_fused(inp, kind, K0, dK0, f"aligned ({A}, {B}, {D}) {form}")
        for which in names:
            for off in (4, 8, 12):
                d1 = Dev()
                d1.__dict__.update(d.__dict__)
                setattr(d1, which, shifted(getattr(d, which), off))
                del launches[:]
                K1, dK1 = fused(ops, inp, d1, kind, hh)
                name, args = launches[0]
                assert name == "vec_kernel_fused" and args[names.index(which)] == getattr(d1, which).data_ptr()  # no copy
                assert torch.equal(K1, K0) and torch.equal(dK1, dK0), (which, off, form)
        # all of them off the grid at once
        d1 = Dev()
        d1.__dict__.update(d.__dict__)
        for which in names:
            setattr(d1, which, shifted(getattr(d, which), 4))
        K1, dK1 = fused(ops, inp, d1, kind, hh)
        assert torch.equal(K1, K0) and torch.equal(dK1, dK0)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
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

    def intact(self):
        now, g, n = self.buf.view(torch.int32), self.g, self.n
        return torch.equal(now[:g], self.copy[:g]) and torch.equal(now[g + n:], self.copy[g + n:])


@pytest.mark.parametrize("metric", [False, True], ids=["plain", "metric"])
@pytest.mark.parametrize("A,B,D", V.FUSED_GUARDED_SHAPES)
def test_fused_nothing_outside_the_operands(gpu, monkeypatch, A, B, D, metric):
    """`sigsvgd_vec_kernel_fused` on pointers into buffers the test owns: K and dK between seeded guards that keep their
    bits, the workspace exactly sized between guards and NaN-filled, X, Y, XM, YM and grad_out between NaN areas that no
    result may meet (the zero padding of a tile does not absorb a NaN)."""
    from sigsvgd_amd import _lib, ops

    ws = GuardedWorkspace(fill="ones").install(monkeypatch)
    g = 64 * max(B, D, 64) + 64  # a tile of rows at the longest row of the launch, and a little
    for form, kind in (("integer", "unit"), ("float", "imq")):
        inp, d = inputs(A, B, D, form, metric, gpu)
        hh = V.half_inv_h2(D, metric)
        names = ("X", "Y", "go") + (("XM", "YM") if metric else ())
        fin = {n: Fenced(getattr(d, n), g) for n in names}
        assert all(bool(torch.isnan(f.buf[:g]).all()) and bool(torch.isnan(f.buf[-g:]).all()) for f in fin.values())
        Kf, dKf = Fenced(torch.zeros(A, B, device=gpu), g, seed=21), Fenced(torch.zeros(A, D, device=gpu), g, seed=22)
        ptr = lambda n: fin[n].t.data_ptr() if n in fin else None
        args = (ptr("X"), ptr("Y"), ptr("XM"), ptr("YM"), ptr("go"), A, B, D, _lib.F32, kind_code(kind), 2 * hh,
                inp.grad_scale, Kf.t.data_ptr(), dKf.t.data_ptr())
        ops._launch(gpu, "vec_kernel_fused", args, "vec_fused_workspace_bytes", (A, B, D))
        torch.cuda.synchronize(gpu)
        ws.check()
        assert Kf.intact(), "K: a guard changed"
        assert dKf.intact(), "dK: a guard changed"
        check_fused(inp, kind, Kf.t, dKf.t, f"guarded ({A}, {B}, {D}) {form} {kind}")
        K0, dK0 = fused(ops, inp, d, kind, hh)
        ws.check()
        assert torch.equal(Kf.t, K0) and torch.equal(dKf.t, dK0)
    assert ws.sizes.count(V.fused_workspace_bytes(A, B, D)) == len(ws.sizes) == 4


# ---- (d) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [False, True], ids=["plain", "metric"])
@pytest.mark.parametrize("n,shape", list(enumerate(V.SQDIST_SHAPES)), ids=lambda v: str(v).replace(" ", "") if isinstance(v, tuple) else None)
def test_sqdist_per_entry(gpu, n, shape, metric):
    from sigsvgd_amd import ops

    A, B, D = shape
    for dtype in (torch.float32, torch.float64) if n % 3 == 0 else (torch.float32,):
        fp64 = dtype == torch.float64
        for form in V.FORMS:
            inp, d = inputs(A, B, D, form, metric, gpu, dtype)
            sq = ops.vec_sqdist(d.X, d.Y, d.XM, d.YM)
            assert sq.shape == (A, B) and sq.dtype == dtype
            e = expected(inp, "unit", "two_launch", fp64)
            worst = V.assert_vec(host(sq), e.sq, e.e_sq, f"sqdist ({A}, {B}, {D}) {form} {'fp64' if fp64 else 'fp32'}", "sq")
            assert worst == 0.0 or form == "float"


@pytest.mark.parametrize("n,shape", list(enumerate(V.KGRAD_SHAPES)), ids=lambda v: str(v).replace(" ", "") if isinstance(v, tuple) else None)
def test_vec_kernel_per_entry(gpu, n, shape):
    from sigsvgd_amd import ops

    A, B, D = shape
    metric = n % 2 == 1
    for dtype in (torch.float32, torch.float64) if n % 3 == 0 else (torch.float32,):
        fp64 = dtype == torch.float64
        path, u = "two_launch", V.U64 if fp64 else V.U32
        for form in V.FORMS:
            inp, d = inputs(A, B, D, form, metric, gpu, dtype)
            hh = V.half_inv_h2(D, metric)
            sq = ops.vec_sqdist(d.X, d.Y, d.XM, d.YM)
            for kind in kinds_of(form):
                where = f"vec_kernel ({A}, {B}, {D}) {form} {kind} {'fp64' if fp64 else 'fp32'}"
                for weighted in (True, False):
                    e = expected(inp, kind, path, fp64, weighted)
                    go = d.go if weighted else None
                    code, s = kind_code(kind), inp.grad_scale
                    if kind == "unit":  # only the gradient (the backward of the distance)
                        none, dK = ops.vec_kernel(sq, d.GXM, d.GYM, code, 2 * hh, s, grad_out=go, want_K=False)
                        worst = V.assert_vec(host(dK), e.dK, e.e_dK, where, "dK", stage=V.GC)
                        assert none is None and (worst == 0.0 or form == "float")
                        continue
                    K, dK = ops.vec_kernel(sq, d.GXM, d.GYM, code, 2 * hh, s, grad_out=go)
                    assert K.shape == (A, B) and dK.shape == (A, D) and K.dtype == dK.dtype == dtype
                    if form == "integer" and weighted:
                        note_f(path + ("64" if fp64 else ""), kind, K, e, u)
                    V.assert_vec(host(K), e.K, e.e_K, where, "K")  # every entry: complete with 1, 2 or 3 channel blocks
                    V.assert_vec(host(dK), e.dK, e.e_dK, where, "dK", stage=V.GC)
                    none, dK2 = ops.vec_kernel(sq, d.GXM, d.GYM, code, 2 * hh, s, grad_out=go, want_K=False)
                    assert none is None and torch.equal(dK2, dK)
                    K3, none = ops.vec_kernel(sq, None, None, code, 2 * hh, 0.0, want_grad=False)
                    assert none is None and torch.equal(K3, K)


# ---- (e) ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def routes(monkeypatch):
    """the names of the `ops` entry points the classes call, in order"""
    from sigsvgd_amd import ops

    seen = []

    def spy(name):
        fn = getattr(ops, name)

        def wrapper(*a, **k):
            seen.append(name)
            return fn(*a, **k)

        return wrapper

    for name in ("vec_sqdist", "vec_kernel", "vec_kernel_fused"):
        monkeypatch.setattr(ops, name, spy(name))
    return seen


@pytest.mark.parametrize("D,dtype,route", [(512, torch.float32, "fused"), (513, torch.float32, "two_launch"),
                                           (68, torch.float64, "two_launch")])
def test_classes_route_by_width_and_type(gpu, routes, D, dtype, route):
    from sigsvgd_amd.kernels import GaussianKernel, ScaledIMQKernel

    A = 65
    fp64 = dtype == torch.float64
    for cls, kind, metric in ((GaussianKernel, "gaussian", False), (ScaledIMQKernel, "imq", True)):
        base, d = inputs(A, A, D, "float", metric, gpu, dtype)
        hh = V.half_inv_h2(D, metric)
        h = float(np.sqrt(0.5 / hh))
        ker = cls()
        del routes[:]
        kw, XM, YM = {}, None, None
        if metric:  # the class forms XM = X @ M itself: the reference takes the operands the kernels were handed
            kw = dict(M=torch.as_tensor(V.metric_matrix(D), device=gpu, dtype=dtype))
            XM, YM = host(d.X @ kw["M"]), host(d.Y @ kw["M"])
        K, dK = ker(d.X, d.Y, h=h, **kw)
        assert routes == (["vec_kernel_fused"] if route == "fused" else ["vec_sqdist", "vec_kernel"]), routes
        inp = V.VecInputs(base.X, base.Y, base.go, XM, YM, ker._grad_scale(h * h), "float")
        e = V.expected(inp, kind, route, fp64=fp64, weighted=False)
        where = f"{cls.__name__} D = {D} {'fp64' if fp64 else 'fp32'}"
        assert K.dtype == dK.dtype == dtype
        V.assert_vec(host(K), e.K, e.e_K, where, "K")
        V.assert_vec(host(dK), e.dK, e.e_dK, where, "dK")
