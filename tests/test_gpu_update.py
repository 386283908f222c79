"""`ops.svgd_update` (svgd_update_kernel, csrc/svgd_phi.hip) against the fused launches, bit for bit.

Equality is exact by construction: without mask and state the fused launch writes v_raw = -((sv - gv) * invN) * 1.f, and
with mask and state it hands the same bits to the device function (`update_element`) that the update kernel runs on v_raw.
So for manual, Adagrad and Adam, with and without a mask, over three consecutive steps, `ops.svgd_update(v_raw, ...)` and
the fused `ops.svgd_phi` / `ops.svgd_adam`, each on its own copy of the state, must agree in v_out, X_out, the Adagrad sum,
exp_avg, exp_avg_sq and the step counter under torch.equal.

Equality says that the two kernels agree, not that either is right.  That evidence is in tests/test_gpu_phi.py: the fused
kernel's product per entry against the fp64 reference at these partial-tile shapes and two dozen more, and both kernels'
update rules per entry against `update_reference.check_update` at (5, 3), (33, 70), (68, 132) and (129, 63).

Shapes (N, D): (5, 3) the scalar path; (33, 70) partial 32 x 64 tiles of the fused kernel, and for the update kernel a D
that is no multiple of 4 with rows off the 16-byte grid; (64, 448) the 16-byte path over several grid-stride rounds (7168
accesses on 7 workgroups of 256 threads)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(5, 3), (33, 70), (64, 448)]
STEPS, LR = 3, 0.05
_INPUTS = {}


def inputs(N, D, gpu):
    """K [N, N], X [N, D], mask [N, D] (zeros and ones) and per step a score and a kernel gradient, from a fixed seed"""
    if (N, D) not in _INPUTS:
        rng = np.random.default_rng(1000 * N + D)
        t = lambda a: torch.as_tensor(a.astype(np.float32), device=gpu)
        _INPUTS[(N, D)] = dict(K=t(rng.uniform(0.2, 1.0, (N, N))), X=t(rng.standard_normal((N, D))),
                               mask=t((rng.uniform(size=(N, D)) > 0.3).astype(np.float64)),
                               s=[t(rng.standard_normal((N, D))) for _ in range(STEPS)],
                               gk=[t(rng.standard_normal((N, D))) for _ in range(STEPS)])
    return _INPUTS[(N, D)]


def adam_equal(a, b):
    return torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq) and int(a.step) == int(b.step) \
        and a.t_host == b.t_host


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("mode", ["manual", "adagrad", "adam"])
@pytest.mark.parametrize("N,D", SHAPES)
def test_update_kernel_has_the_fused_launch_bits(gpu, N, D, mode, masked):
    from sigsvgd_amd import ops

    I = inputs(N, D, gpu)
    mask = I["mask"] if masked else None
    Xf, Xu, Xi = I["X"].clone(), I["X"].clone(), I["X"].clone()  # fused, update out of place, update in place
    new_state = lambda: (torch.zeros(N, D, device=gpu) if mode == "adagrad" else
                         ops.AdamState(I["X"]) if mode == "adam" else None)
    sf, su, si = new_state(), new_state(), new_state()
    for k in range(STEPS):
        K, s, gk = I["K"], I["s"][k], I["gk"][k]
        v_raw = ops.svgd_phi(K, s, gk)
        keep = v_raw.clone()
        if mode == "adam":
            vf, Xf = ops.svgd_adam(K, s, gk, Xf, LR, sf, mask=mask)
            vu, Xu = ops.svgd_update(v_raw, Xu, LR, mask=mask, adam=su)
            vi, Xr = ops.svgd_update(v_raw, Xi, LR, mask=mask, adam=si, inplace=True)
            assert adam_equal(sf, su) and adam_equal(sf, si) and int(su.step) == k + 1
        else:
            vf, Xf = ops.svgd_phi(K, s, gk, mask=mask, X=Xf, lr=LR, adagrad_state=sf)
            vu, Xu = ops.svgd_update(v_raw, Xu, LR, mask=mask, adagrad_state=su)
            vi, Xr = ops.svgd_update(v_raw, Xi, LR, mask=mask, adagrad_state=si, inplace=True)
            if mode == "adagrad":
                assert torch.equal(sf, su) and torch.equal(sf, si)
        assert Xr is Xi and torch.equal(v_raw, keep)  # in place on X only: the velocity given is left alone
        if mode != "adam" and k == 0:  # want_v=False (v_out == NULL): the same particles, no velocity stored
            none, Xw = ops.svgd_update(v_raw, I["X"], LR, mask=mask, adagrad_state=None if sf is None else torch.zeros_like(sf),
                                       want_v=False)
            assert none is None and torch.equal(Xw, Xu)
        assert torch.equal(vf, vu) and torch.equal(vf, vi), (k, float((vf - vu).abs().max()))
        assert torch.equal(Xf, Xu) and torch.equal(Xf, Xi), (k, float((Xf - Xu).abs().max()))
        assert bool(torch.isfinite(Xf).all()) and not torch.equal(Xf, I["X"])
    if masked:
        still = I["mask"] == 0
        assert torch.equal(Xu[still], I["X"][still]) and bool(still.any()) and not bool(still.all())


def test_misaligned_operand_takes_the_scalar_path(gpu):
    """D % 4 == 0 with one pointer off the 16-byte grid: the kernel's own test sends the launch down the scalar path, to the
    same bits"""
    from sigsvgd_amd import ops

    N, D = 64, 448
    I = inputs(N, D, gpu)
    v = ops.svgd_phi(I["K"], I["s"][0], I["gk"][0])
    shifted = torch.empty(N * D + 1, device=gpu)[1:].view(N, D)
    shifted.copy_(v)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    a, b = ops.AdamState(I["X"]), ops.AdamState(I["X"])
    va, Xa = ops.svgd_update(v, I["X"], LR, mask=I["mask"], adam=a)
    vb, Xb = ops.svgd_update(shifted, I["X"], LR, mask=I["mask"], adam=b)
    assert torch.equal(va, vb) and torch.equal(Xa, Xb) and adam_equal(a, b)


def test_argument_checks(gpu):
    from sigsvgd_amd import ops

    v, X = torch.zeros(4, 6, device=gpu), torch.zeros(4, 6, device=gpu)
    with pytest.raises(ValueError):
        ops.svgd_update(v, X[:, :3], 0.1)
    with pytest.raises(ValueError):
        ops.svgd_update(v, X, 0.1, adagrad_state=torch.zeros(4, 6, device=gpu), adam=ops.AdamState(X))
    with pytest.raises(ValueError):
        ops.svgd_update(v, X, 0.1, adagrad_state=torch.zeros(4, 5, device=gpu))
    with pytest.raises(ValueError):
        ops.svgd_update(v, X, 0.1, adam=ops.AdamState(X[:, :3]))
    with pytest.raises(ValueError):
        ops.svgd_update(v, X.double(), 0.1, inplace=True)


def test_captured_adam_updates_replay_to_the_eager_result(gpu):
    """One captured graph of three Adam updates (one stream, no parallel branches): the step counter lives on the device and
    is advanced by a launch of its own, so the replay forms the three bias corrections the eager launches form"""
    from sigsvgd_amd import ops

    N, D = 33, 70
    I = inputs(N, D, gpu)
    vs = [ops.svgd_phi(I["K"], I["s"][k], I["gk"][k]) for k in range(STEPS)]
    eager, Xe = ops.AdamState(I["X"]), I["X"].clone()
    for v in vs:
        ops.svgd_update(v, Xe, LR, mask=I["mask"], adam=eager, inplace=True)

    st, Xg = ops.AdamState(I["X"]), I["X"].clone()

    def three():
        for v in vs:
            ops.svgd_update(v, Xg, LR, mask=I["mask"], adam=st, inplace=True)

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        three()  # warm-up outside the capture
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize(gpu)
    Xg.copy_(I["X"])
    st.exp_avg.zero_(), st.exp_avg_sq.zero_(), st.step.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        three()
    Xg.copy_(I["X"])  # (capture does not execute; keep the starting point explicit)
    st.exp_avg.zero_(), st.exp_avg_sq.zero_(), st.step.zero_()
    graph.replay()
    torch.cuda.synchronize(gpu)
    assert int(st.step) == STEPS
    assert torch.equal(Xg, Xe) and torch.equal(st.exp_avg, eager.exp_avg) and torch.equal(st.exp_avg_sq, eager.exp_avg_sq)
