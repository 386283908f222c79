"""Where `fp32_sweeps=True` goes in the Python layer, pinned on the CPU with recorders in the style of
tests/test_gram_routing_cpu.py: `SigKernel(..., fp32_sweeps=True)` hands the keyword to every fused launch and every
`ops.gram_takes` query it makes, the default `SigKernel` hands over no such keyword (the recorders of
tests/test_gram_routing_cpu.py have closed signatures and stay green), the long route never sees it, and
`ShardedSigSVGD.route()` takes the fused partial solve for kinds 2 and 3 only with it."""
import pytest
import torch

import sigsvgd_amd.sigkernel as sk
from sigsvgd_amd import _lib, ops
from sigsvgd_amd.distributed import ShardedSigSVGD

A, B, T, TY, D = 8, 6, 5, 4, 2


class Recorder:
    """every fused function notes the keywords it was called with; the long-route ones take none beyond their own"""

    def __init__(self, fused):
        self.fused, self.calls = fused, []

    def gram_takes(self, A, B, T, d, dyadic_order=0, static_kind=0, want_grad=True, naive=False, sym=False, y_is_x=False,
                   **kw):
        self.calls.append(("gram_takes", static_kind, dict(kw)))
        return self.fused

    def gram_fwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, naive=False, force_generic=False, y_is_x=False,
                 stored_forward=False, **kw):
        self.calls.append(("gram_fwd", static_kind, dict(kw)))
        return torch.zeros(X.shape[0], Y.shape[0], dtype=X.dtype)

    def gram_fwd_bwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False, y_is_x=False,
                     force_generic=False, check_regime=True, stored_forward=False, **kw):
        self.calls.append(("gram_fwd_bwd", static_kind, dict(kw)))
        return torch.zeros(X.shape[0], Y.shape[0], dtype=X.dtype), torch.zeros_like(X)

    def gram_long_fwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, naive=False):
        self.calls.append(("gram_long_fwd", static_kind, {}))
        return torch.zeros(X.shape[0], Y.shape[0], dtype=X.dtype)

    def gram_long_fwd_bwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False):
        self.calls.append(("gram_long_fwd_bwd", static_kind, {}))
        return torch.zeros(X.shape[0], Y.shape[0], dtype=X.dtype), torch.zeros_like(X)

    def gram_long_fwd_bwd2(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False,
                           y_is_x=False, want_gradX=True, want_gradY=True):
        self.calls.append(("gram_long_fwd_bwd2", static_kind, {}))
        K = torch.zeros(X.shape[0], Y.shape[0], dtype=X.dtype)
        return K, (torch.zeros_like(X) if want_gradX else None), (torch.zeros_like(Y) if want_gradY else None)


def paths(n, t, grad):
    return torch.linspace(0.0, 1.0, n * t * D, dtype=torch.float64).reshape(n, t, D).requires_grad_(grad)


def run_everything(kernel):
    """forward-only, speculated, weighted backward, grad_Y, sym, gram_and_grad and compute_kernel's diagonal route"""
    X, Y = paths(A, T, True), paths(B, TY, True)
    kernel.compute_Gram(X.detach(), Y.detach())
    K = kernel.compute_Gram(X, X)
    (K * torch.arange(1.0, K.numel() + 1.0, dtype=K.dtype).reshape(K.shape)).sum().backward()
    kernel.compute_Gram(X, Y, grad_Y=True).sum().backward()
    kernel.compute_Gram(X, X, sym=True).sum().backward()
    kernel.gram_and_grad(X.detach(), Y.detach())
    kernel.gram_and_grad(X.detach(), None, sym=True)


def record(monkeypatch, kernel, fused):
    rec = Recorder(fused)
    for name in ("gram_takes", "gram_fwd", "gram_fwd_bwd", "gram_long_fwd", "gram_long_fwd_bwd", "gram_long_fwd_bwd2"):
        monkeypatch.setattr(ops, name, getattr(rec, name))
    monkeypatch.setattr(sk, "_device_cus", lambda X: 256)
    run_everything(kernel)
    return rec.calls


FUSED = ("gram_takes", "gram_fwd", "gram_fwd_bwd")


@pytest.mark.parametrize("static,kind", [(sk.IMQStaticKernel, _lib.STATIC_IMQ), (sk.RationalQuadraticKernel, _lib.STATIC_RQ)])
def test_the_flagged_kernel_hands_the_keyword_to_every_fused_launch_and_query(monkeypatch, static, kind):
    calls = record(monkeypatch, sk.SigKernel(static(1.0), 0, fp32_sweeps=True), True)
    assert {c[0] for c in calls} == set(FUSED)
    assert len([c for c in calls if c[0] == "gram_fwd_bwd"]) >= 7 and len([c for c in calls if c[0] == "gram_fwd"]) == 1
    assert all(c[1] == kind and c[2] == {"fp32_sweeps": True} for c in calls), calls


def test_the_long_route_does_not_see_it(monkeypatch):
    calls = record(monkeypatch, sk.SigKernel(sk.IMQStaticKernel(1.0), 0, fp32_sweeps=True), False)
    assert {c[0] for c in calls} == {"gram_takes", "gram_long_fwd", "gram_long_fwd_bwd", "gram_long_fwd_bwd2"}
    assert all(c[2] == ({"fp32_sweeps": True} if c[0] == "gram_takes" else {}) for c in calls), calls


@pytest.mark.parametrize("static", [sk.RBFKernel, sk.IMQStaticKernel])
@pytest.mark.parametrize("fused", [True, False])
def test_the_default_kernel_hands_over_no_such_keyword(monkeypatch, static, fused):
    k = sk.SigKernel(static(1.0), 0)
    assert k.fp32_sweeps is False
    calls = record(monkeypatch, k, fused)
    assert calls and all(c[2] == {} for c in calls), calls


def test_signature_kernel_hands_it_on():
    from sigsvgd_amd.kernels import SignatureKernel

    assert SignatureKernel(lambda _: 1.0, depth=0, static_kernel="rq", fp32_sweeps=True).kernel.fp32_sweeps is True
    assert SignatureKernel(lambda _: 1.0, depth=0, static_kernel="rq").kernel.fp32_sweeps is False
    assert SignatureKernel(lambda _: 1.0, depth=0, static_kernel="rq", bandwidth=3).kernel.fp32_sweeps is False  # (ignored kwargs stay)


def test_sharded_route(monkeypatch):
    """route() with a faked `_partial_supported`: "partial" for kinds 2 and 3 at order 0 with the flag where the partial solve
    takes the shape and the path has at most 64 points; what it was in every other case"""
    X64, X65, X300 = torch.zeros(8, 64, 7), torch.zeros(8, 65, 7), torch.zeros(8, 300, 2)
    for kind in (_lib.STATIC_IMQ, _lib.STATIC_RQ):
        monkeypatch.setattr(ShardedSigSVGD, "_partial_supported", staticmethod(lambda X_full: True))
        assert ShardedSigSVGD(1.0, 0.1, static_kind=kind, fp32_sweeps=True).route(X64, 1) == "partial"
        assert ShardedSigSVGD(1.0, 0.1, static_kind=kind, fp32_sweeps=True).route(X64, 4) == "partial"
        assert ShardedSigSVGD(1.0, 0.1, static_kind=kind).route(X64, 1) == "rowwise"
        assert ShardedSigSVGD(1.0, 0.1, static_kind=kind, fp32_sweeps=True).route(X65, 1) == "rowwise"
        assert ShardedSigSVGD(1.0, 0.1, static_kind=kind, fp32_sweeps=True, dyadic_order=1).route(X64, 1) == "rowwise"
        assert ShardedSigSVGD(1.0, 0.1, static_kind=kind, fp32_sweeps=True, rowwise=True).route(X64, 1) == "rowwise"
        assert ShardedSigSVGD(1.0, 0.1, static_kind=kind, fp32_sweeps=True).route(X300, 1) == "long_partial"
        monkeypatch.setattr(ShardedSigSVGD, "_partial_supported", staticmethod(lambda X_full: False))
        assert ShardedSigSVGD(1.0, 0.1, static_kind=kind, fp32_sweeps=True).route(X64, 1) == "rowwise"
    monkeypatch.setattr(ShardedSigSVGD, "_partial_supported", staticmethod(lambda X_full: True))
    for kind in (_lib.STATIC_MATERN32, _lib.STATIC_LINEAR):
        assert ShardedSigSVGD(1.0, 0.1, static_kind=kind, fp32_sweeps=True).route(X64, 1) == "rowwise"
    assert ShardedSigSVGD(1.0, 0.1, fp32_sweeps=True).route(X64, 1) == ShardedSigSVGD(1.0, 0.1).route(X64, 1) == "partial"


def test_sharded_step_functions_carry_the_flag(monkeypatch):
    """the partial solve of a flagged step is ops.gram_sym_partial(..., static_kind=, fp32_sweeps=True), and its row-wise
    fallback passes the flag to the query and the launch; an unflagged step passes no such keyword"""
    calls = []
    monkeypatch.setattr(ops, "gram_sym_partial", lambda *a, **k: calls.append(("partial", k)))
    monkeypatch.setattr(ops, "gram_takes", lambda *a, **k: calls.append(("takes", k)) or True)
    monkeypatch.setattr(ops, "gram_fwd_bwd", lambda *a, **k: calls.append(("rows", k)))
    sh = ShardedSigSVGD(1.0, 0.1, static_kind=_lib.STATIC_IMQ, fp32_sweeps=True)
    sh.partial_fn(torch.zeros(8, 64, 7), 1.0, 0, 1, out=None, fold=True)
    sh.rows_fn(torch.zeros(4, 64, 7), torch.zeros(8, 64, 7), 1.0)
    assert calls == [("partial", {"static_kind": _lib.STATIC_IMQ, "out": None, "fold": True, "fp32_sweeps": True}),
                     ("takes", {"fp32_sweeps": True}), ("rows", {"fp32_sweeps": True})]
    del calls[:]
    plain = ShardedSigSVGD(1.0, 0.1, static_kind=_lib.STATIC_IMQ)
    assert plain.partial_fn is ops.gram_sym_partial
    plain.rows_fn(torch.zeros(4, 64, 7), torch.zeros(8, 64, 7), 1.0)
    assert calls == [("takes", {}), ("rows", {})]
