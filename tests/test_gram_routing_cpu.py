"""Which launch serves a Gram request (`SigKernel.compute_Gram`, its backward, `SigKernel.gram_and_grad`), pinned on the CPU.

The five launch functions of `sigsvgd_amd.ops` are replaced by recorders that return zero tensors of the right shapes,
`ops.gram_takes` by a recorder whose answer the case sets (True: the fused kernels take the launch; False: the long route)
and `sigkernel._device_cus` by a constant.  A = 8, T = 5, d = 2, fp64; the second batch of the two-tensor cases is B = 6,
TY = 4, so operand order shows in the recorded shapes.  At A = 8 the compute-unit counts 4 and 256 put both answers of
`_long_yx_route` on both sides: gradient 10 < 4 is false and 10 < 256 true, forward 36 >= 32 true and 36 >= 2048 false.

A recorded launch is (name, (A, TX), (B, TY), flags): the first two dimensions of the operands in the order passed, and the
routing arguments that were set, of "sym", "yx" (y_is_x), "gx" / "gy" (want_gradX / want_gradY, long2 only) and "w" (weights
passed).  A recorded query is the (want_grad, sym, y_is_x) of a `gram_takes` call.  The expected values were recorded from
the code as it stood before the routing moved into one function."""
import pytest
import torch

import sigsvgd_amd.sigkernel as sk
from sigsvgd_amd import ops

A, B, T, TY, D = 8, 6, 5, 4, 2


class Recorder:
    def __init__(self, fused):
        self.fused, self.launches, self.queries = fused, [], []

    def _note(self, name, X, Y, **flags):
        self.launches.append((name, tuple(X.shape[:2]), tuple(Y.shape[:2]), " ".join(k for k, v in flags.items() if v)))
        return torch.zeros(X.shape[0], Y.shape[0], dtype=X.dtype)

    def gram_takes(self, A, B, T, d, dyadic_order=0, static_kind=0, want_grad=True, naive=False, sym=False, y_is_x=False):
        self.queries.append((bool(want_grad), bool(sym), bool(y_is_x)))
        return self.fused

    def gram_fwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, naive=False, force_generic=False, y_is_x=False,
                 stored_forward=False):
        return self._note("gram_fwd", X, Y, yx=y_is_x)

    def gram_fwd_bwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False, y_is_x=False,
                     force_generic=False, check_regime=True, stored_forward=False):
        assert grad_out is None or tuple(grad_out.shape) == (X.shape[0], Y.shape[0])
        return self._note("gram_fwd_bwd", X, Y, sym=sym, yx=y_is_x, w=grad_out is not None), torch.zeros_like(X)

    def gram_long_fwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, naive=False):
        return self._note("gram_long_fwd", X, Y)

    def gram_long_fwd_bwd(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False):
        return self._note("gram_long_fwd_bwd", X, Y, sym=sym, w=grad_out is not None), torch.zeros_like(X)

    def gram_long_fwd_bwd2(self, X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False,
                           y_is_x=False, want_gradX=True, want_gradY=True):
        K = self._note("gram_long_fwd_bwd2", X, Y, sym=sym, yx=y_is_x, gx=want_gradX, gy=want_gradY, w=grad_out is not None)
        return K, (torch.zeros_like(X) if want_gradX else None), (torch.zeros_like(Y) if want_gradY else None)


def paths(n, t, grad):
    return torch.linspace(0.0, 1.0, n * t * D, dtype=torch.float64).reshape(n, t, D).requires_grad_(grad)


def weights(K):
    return torch.arange(1.0, K.numel() + 1.0, dtype=K.dtype).reshape(K.shape)


def gram(two, grad=True, speculate=True, backward=None, **kw):
    """compute_Gram on one tensor in both slots, or (`two`) on two tensors of different batch and length; then, with
    `backward`, the backward pass of uniform ("sum") or non-uniform ("weighted") weights"""
    def run(kernel):
        kernel.speculate_ones = speculate
        X = paths(A, T, grad)
        Y = paths(B, TY, grad and kw.get("grad_Y", False)) if two else X
        K = kernel.compute_Gram(X, Y, **kw)
        if backward is not None:
            (K.sum() if backward == "sum" else (K * weights(K)).sum()).backward()
    return run


def gram_and_grad(two, **kw):
    def run(kernel):
        X = paths(A, T, False)
        kernel.gram_and_grad(X, paths(B, TY, False) if two else None, **kw)
    return run


SCENARIOS = {
    "forward, one tensor": gram(False, grad=False),
    "forward, two tensors": gram(True, grad=False),
    "speculated, one tensor": gram(False),
    "speculated, two tensors": gram(True),
    "speculated, sym": gram(False, sym=True),
    "speculated, grad_Y, one tensor": gram(False, grad_Y=True),
    "speculated, grad_Y, two tensors": gram(True, grad_Y=True),
    "speculated, uniform backward": gram(True, backward="sum"),
    "speculated, weighted backward, one tensor": gram(False, backward="weighted"),
    "speculated, weighted backward, two tensors": gram(True, backward="weighted"),
    "speculated, weighted backward, sym": gram(False, sym=True, backward="weighted"),
    "speculated, weighted backward, grad_Y": gram(True, grad_Y=True, backward="weighted"),
    "not speculated, forward, one tensor": gram(False, speculate=False),
    "not speculated, uniform backward, one tensor": gram(False, speculate=False, backward="sum"),
    "not speculated, weighted backward, two tensors": gram(True, speculate=False, backward="weighted"),
    "not speculated, weighted backward, grad_Y": gram(True, speculate=False, grad_Y=True, backward="weighted"),
    "gram_and_grad, Y omitted": gram_and_grad(False),
    "gram_and_grad, Y given": gram_and_grad(True),
    "gram_and_grad, sym": gram_and_grad(False, sym=True),
    "gram_and_grad, weights": gram_and_grad(True, grad_out=torch.ones(A, B, dtype=torch.float64)),
}

# scenario -> {route: (launches, queries)}; route "fused" holds for both compute-unit counts
EXPECTED = {"forward, one tensor": {"fused": ([("gram_fwd", (8, 5), (8, 5), "yx")], [(False, False, True)]),
                         "long, 4 units": ([("gram_long_fwd_bwd2", (8, 5), (8, 5), "yx")], [(False, False, True)]),
                         "long, 256 units": ([("gram_long_fwd", (8, 5), (8, 5), "")], [(False, False, True)])},
 "forward, two tensors": {"fused": ([("gram_fwd", (8, 5), (6, 4), "")], [(False, False, False)]),
                          "long, 4 units": ([("gram_long_fwd", (8, 5), (6, 4), "")], [(False, False, False)]),
                          "long, 256 units": ([("gram_long_fwd", (8, 5), (6, 4), "")], [(False, False, False)])},
 "speculated, one tensor": {"fused": ([("gram_fwd_bwd", (8, 5), (8, 5), "yx")], [(True, False, True)]),
                            "long, 4 units": ([("gram_long_fwd_bwd", (8, 5), (8, 5), "")], [(True, False, True)]),
                            "long, 256 units": ([("gram_long_fwd_bwd2", (8, 5), (8, 5), "yx gx")], [(True, False, True)])},
 "speculated, two tensors": {"fused": ([("gram_fwd_bwd", (8, 5), (6, 4), "")], [(True, False, False)]),
                             "long, 4 units": ([("gram_long_fwd_bwd", (8, 5), (6, 4), "")], [(True, False, False)]),
                             "long, 256 units": ([("gram_long_fwd_bwd", (8, 5), (6, 4), "")], [(True, False, False)])},
 "speculated, sym": {"fused": ([("gram_fwd_bwd", (8, 5), (8, 5), "sym yx")], [(True, True, True)]),
                     "long, 4 units": ([("gram_long_fwd_bwd", (8, 5), (8, 5), "sym")], [(True, True, True)]),
                     "long, 256 units": ([("gram_long_fwd_bwd2", (8, 5), (8, 5), "sym yx gx")], [(True, True, True)])},
 "speculated, grad_Y, one tensor": {"fused": ([("gram_fwd_bwd", (8, 5), (8, 5), ""), ("gram_fwd_bwd", (8, 5), (8, 5), "")],
                                              [(True, False, False)]),
                                    "long, 4 units": ([("gram_long_fwd_bwd2", (8, 5), (8, 5), "gx gy")],
                                                      [(True, False, False)]),
                                    "long, 256 units": ([("gram_long_fwd_bwd2", (8, 5), (8, 5), "gx gy")],
                                                        [(True, False, False)])},
 "speculated, grad_Y, two tensors": {"fused": ([("gram_fwd_bwd", (8, 5), (6, 4), ""), ("gram_fwd_bwd", (6, 4), (8, 5), "")],
                                               [(True, False, False)]),
                                     "long, 4 units": ([("gram_long_fwd_bwd2", (8, 5), (6, 4), "gx gy")],
                                                       [(True, False, False)]),
                                     "long, 256 units": ([("gram_long_fwd_bwd2", (8, 5), (6, 4), "gx gy")],
                                                         [(True, False, False)])},
 "speculated, uniform backward": {"fused": ([("gram_fwd_bwd", (8, 5), (6, 4), "")], [(True, False, False)]),
                                  "long, 4 units": ([("gram_long_fwd_bwd", (8, 5), (6, 4), "")], [(True, False, False)]),
                                  "long, 256 units": ([("gram_long_fwd_bwd", (8, 5), (6, 4), "")], [(True, False, False)])},
 "speculated, weighted backward, one tensor": {"fused": ([("gram_fwd_bwd", (8, 5), (8, 5), "yx"),
                                                          ("gram_fwd_bwd", (8, 5), (8, 5), "w")],
                                                         [(True, False, True), (True, False, False)]),
                                               "long, 4 units": ([("gram_long_fwd_bwd", (8, 5), (8, 5), ""),
                                                                  ("gram_long_fwd_bwd", (8, 5), (8, 5), "w")],
                                                                 [(True, False, True), (True, False, False)]),
                                               "long, 256 units": ([("gram_long_fwd_bwd2", (8, 5), (8, 5), "yx gx"),
                                                                    ("gram_long_fwd_bwd2", (8, 5), (8, 5), "yx gx w")],
                                                                   [(True, False, True), (True, False, False)])},
 "speculated, weighted backward, two tensors": {"fused": ([("gram_fwd_bwd", (8, 5), (6, 4), ""),
                                                           ("gram_fwd_bwd", (8, 5), (6, 4), "w")],
                                                          [(True, False, False), (True, False, False)]),
                                                "long, 4 units": ([("gram_long_fwd_bwd", (8, 5), (6, 4), ""),
                                                                   ("gram_long_fwd_bwd", (8, 5), (6, 4), "w")],
                                                                  [(True, False, False), (True, False, False)]),
                                                "long, 256 units": ([("gram_long_fwd_bwd", (8, 5), (6, 4), ""),
                                                                     ("gram_long_fwd_bwd", (8, 5), (6, 4), "w")],
                                                                    [(True, False, False), (True, False, False)])},
 "speculated, weighted backward, sym": {"fused": ([("gram_fwd_bwd", (8, 5), (8, 5), "sym yx"),
                                                   ("gram_fwd_bwd", (8, 5), (8, 5), "sym w")],
                                                  [(True, True, True), (True, True, False)]),
                                        "long, 4 units": ([("gram_long_fwd_bwd", (8, 5), (8, 5), "sym"),
                                                           ("gram_long_fwd_bwd", (8, 5), (8, 5), "sym w")],
                                                          [(True, True, True), (True, True, False)]),
                                        "long, 256 units": ([("gram_long_fwd_bwd2", (8, 5), (8, 5), "sym yx gx"),
                                                             ("gram_long_fwd_bwd2", (8, 5), (8, 5), "sym yx gx w")],
                                                            [(True, True, True), (True, True, False)])},
 "speculated, weighted backward, grad_Y": {"fused": ([("gram_fwd_bwd", (8, 5), (6, 4), ""),
                                                      ("gram_fwd_bwd", (6, 4), (8, 5), ""),
                                                      ("gram_fwd_bwd", (8, 5), (6, 4), "w"),
                                                      ("gram_fwd_bwd", (6, 4), (8, 5), "w")],
                                                     [(True, False, False), (True, False, False)]),
                                           "long, 4 units": ([("gram_long_fwd_bwd2", (8, 5), (6, 4), "gx gy"),
                                                              ("gram_long_fwd_bwd2", (8, 5), (6, 4), "gx gy w")],
                                                             [(True, False, False), (True, False, False)]),
                                           "long, 256 units": ([("gram_long_fwd_bwd2", (8, 5), (6, 4), "gx gy"),
                                                                ("gram_long_fwd_bwd2", (8, 5), (6, 4), "gx gy w")],
                                                               [(True, False, False), (True, False, False)])},
 "not speculated, forward, one tensor": {"fused": ([("gram_fwd", (8, 5), (8, 5), "yx")], [(False, False, True)]),
                                         "long, 4 units": ([("gram_long_fwd_bwd2", (8, 5), (8, 5), "yx")],
                                                           [(False, False, True)]),
                                         "long, 256 units": ([("gram_long_fwd", (8, 5), (8, 5), "")],
                                                             [(False, False, True)])},
 "not speculated, uniform backward, one tensor": {"fused": ([("gram_fwd", (8, 5), (8, 5), "yx"),
                                                             ("gram_fwd_bwd", (8, 5), (8, 5), "w")],
                                                            [(False, False, True), (True, False, False)]),
                                                  "long, 4 units": ([("gram_long_fwd_bwd2", (8, 5), (8, 5), "yx"),
                                                                     ("gram_long_fwd_bwd", (8, 5), (8, 5), "w")],
                                                                    [(False, False, True), (True, False, False)]),
                                                  "long, 256 units": ([("gram_long_fwd", (8, 5), (8, 5), ""),
                                                                       ("gram_long_fwd_bwd2", (8, 5), (8, 5), "yx gx w")],
                                                                      [(False, False, True), (True, False, False)])},
 "not speculated, weighted backward, two tensors": {"fused": ([("gram_fwd", (8, 5), (6, 4), ""),
                                                               ("gram_fwd_bwd", (8, 5), (6, 4), "w")],
                                                              [(False, False, False), (True, False, False)]),
                                                    "long, 4 units": ([("gram_long_fwd", (8, 5), (6, 4), ""),
                                                                       ("gram_long_fwd_bwd", (8, 5), (6, 4), "w")],
                                                                      [(False, False, False), (True, False, False)]),
                                                    "long, 256 units": ([("gram_long_fwd", (8, 5), (6, 4), ""),
                                                                         ("gram_long_fwd_bwd", (8, 5), (6, 4), "w")],
                                                                        [(False, False, False), (True, False, False)])},
 "not speculated, weighted backward, grad_Y": {"fused": ([("gram_fwd", (8, 5), (6, 4), ""),
                                                          ("gram_fwd_bwd", (8, 5), (6, 4), "w"),
                                                          ("gram_fwd_bwd", (6, 4), (8, 5), "w")],
                                                         [(False, False, False), (True, False, False)]),
                                               "long, 4 units": ([("gram_long_fwd", (8, 5), (6, 4), ""),
                                                                  ("gram_long_fwd_bwd2", (8, 5), (6, 4), "gx gy w")],
                                                                 [(False, False, False), (True, False, False)]),
                                               "long, 256 units": ([("gram_long_fwd", (8, 5), (6, 4), ""),
                                                                    ("gram_long_fwd_bwd2", (8, 5), (6, 4), "gx gy w")],
                                                                   [(False, False, False), (True, False, False)])},
 "gram_and_grad, Y omitted": {"fused": ([("gram_fwd_bwd", (8, 5), (8, 5), "yx")], [(True, False, True)]),
                              "long, 4 units": ([("gram_long_fwd_bwd", (8, 5), (8, 5), "")], [(True, False, True)]),
                              "long, 256 units": ([("gram_long_fwd_bwd2", (8, 5), (8, 5), "yx gx")],
                                                  [(True, False, True)])},
 "gram_and_grad, Y given": {"fused": ([("gram_fwd_bwd", (8, 5), (6, 4), "")], [(True, False, False)]),
                            "long, 4 units": ([("gram_long_fwd_bwd", (8, 5), (6, 4), "")], [(True, False, False)]),
                            "long, 256 units": ([("gram_long_fwd_bwd", (8, 5), (6, 4), "")], [(True, False, False)])},
 "gram_and_grad, sym": {"fused": ([("gram_fwd_bwd", (8, 5), (8, 5), "sym yx")], [(True, True, True)]),
                        "long, 4 units": ([("gram_long_fwd_bwd", (8, 5), (8, 5), "sym")], [(True, True, True)]),
                        "long, 256 units": ([("gram_long_fwd_bwd2", (8, 5), (8, 5), "sym yx gx")], [(True, True, True)])},
 "gram_and_grad, weights": {"fused": ([("gram_fwd_bwd", (8, 5), (6, 4), "w")], [(True, False, False)]),
                            "long, 4 units": ([("gram_long_fwd_bwd", (8, 5), (6, 4), "w")], [(True, False, False)]),
                            "long, 256 units": ([("gram_long_fwd_bwd", (8, 5), (6, 4), "w")], [(True, False, False)])}}


def record(monkeypatch, scenario, fused, cus):
    rec = Recorder(fused)
    for name in ("gram_takes", "gram_fwd", "gram_fwd_bwd", "gram_long_fwd", "gram_long_fwd_bwd", "gram_long_fwd_bwd2"):
        monkeypatch.setattr(ops, name, getattr(rec, name))
    monkeypatch.setattr(sk, "_device_cus", lambda X: cus)
    SCENARIOS[scenario](sk.SigKernel(sk.RBFKernel(1.0), 0))
    return rec.launches, rec.queries


@pytest.mark.parametrize("cus", [4, 256])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "long"])
@pytest.mark.parametrize("scenario", list(SCENARIOS))
def test_launch_of_a_gram_request(monkeypatch, scenario, fused, cus):
    launches, queries = record(monkeypatch, scenario, fused, cus)
    want_launches, want_queries = EXPECTED[scenario]["fused" if fused else f"long, {cus} units"]
    assert launches == want_launches
    assert queries == want_queries


def test_every_launch_function_and_both_pair_orders_are_met():
    """the table itself: all five launch functions, and on the long route both the ordered and the unordered launch of a
    one-tensor request, forward-only and with a gradient"""
    met = {(route, launch[0], launch[3]) for per_route in EXPECTED.values() for route, (launches, _) in per_route.items()
           for launch in launches}
    assert {name for _, name, _ in met} == {"gram_fwd", "gram_fwd_bwd", "gram_long_fwd", "gram_long_fwd_bwd",
                                            "gram_long_fwd_bwd2"}
    assert ("long, 4 units", "gram_long_fwd_bwd2", "yx") in met and ("long, 256 units", "gram_long_fwd", "") in met
    assert ("long, 256 units", "gram_long_fwd_bwd2", "yx gx") in met and ("long, 4 units", "gram_long_fwd_bwd", "") in met
