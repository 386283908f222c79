"""Host-side checks of the three fused velocity entry points, `sigsvgd_svgd_phi`, `sigsvgd_svgd_step` and
`sigsvgd_svgd_adam_step` (include/sigsvgd_hip.h; tests/test_update_cabi.py holds the same for `sigsvgd_svgd_update`): the
symbols, the ABI version they leave alone, and every argument rule of `phi_launch` and of the Adam wrapper, each refused with
SIGSVGD_E_BADARG and a message before any device work (no device needed: no call below gets past its argument checks), and
the checks `ops.svgd_phi` and `ops.svgd_adam` make before they reach the library."""
import re

import pytest
import torch

from cabi import assert_exported, BADARG, FAKE, lib
from sigsvgd_amd import _lib, ops

NAMES = ("sigsvgd_svgd_phi", "sigsvgd_svgd_step", "sigsvgd_svgd_adam_step")


def call(name, K=FAKE, score=FAKE, grad_k=FAKE, mask=None, N=4, D=6, v_out=FAKE, X_in=FAKE, X_out=FAKE, lr=0.1, adagrad=None,
         beta1=0.9, beta2=0.999, eps=1e-8, exp_avg=FAKE, exp_avg_sq=FAKE, step=FAKE):
    head = (K, score, grad_k, mask, N, D, v_out, X_in, X_out, lr)
    if name == "sigsvgd_svgd_phi":
        return lib().sigsvgd_svgd_phi(*head, None)
    if name == "sigsvgd_svgd_step":
        return lib().sigsvgd_svgd_step(*head, adagrad, None)
    return lib().sigsvgd_svgd_adam_step(*head, beta1, beta2, eps, exp_avg, exp_avg_sq, step, None)


def test_fused_symbols_exported():
    assert_exported(NAMES, abi=10)
    with open(_lib.HEADERS[-1]) as f:
        header = f.read()
    for name in NAMES:
        assert len(re.findall(r"^int " + name + r"\(", header, flags=re.M)) == 1, name


# the rules of phi_launch, which all three entry points reach: (arguments, text of the message)
LAUNCH = {
    "N<1": (dict(N=0), "N=0"),
    "N<0": (dict(N=-4), "N=-4"),
    "D<1": (dict(D=0), "D=0"),
    "K NULL": (dict(K=None), "bad arguments"),
    "score NULL": (dict(score=None), "bad arguments"),
    "grad_k NULL": (dict(grad_k=None), "bad arguments"),
    "v_out NULL": (dict(v_out=None), "bad arguments"),
}
# X_in / X_out: phi_launch's rule for the first two entry points; the Adam wrapper needs both, and says so itself
PARTICLES = {"X_in only": dict(X_out=None), "X_out only": dict(X_in=None)}
ADAM = {
    "without exp_avg": (dict(exp_avg=None), "null state"),
    "without exp_avg_sq": (dict(exp_avg_sq=None), "null state"),
    "without the counter": (dict(step=None), "null state"),
    "without X": (dict(X_in=None, X_out=None), "null state"),
    "X_in only": (dict(X_out=None), "null state"),
    "X_out only": (dict(X_in=None), "null state"),
    "beta1 = 1": (dict(beta1=1.0), "hyper-parameters"),
    "beta1 < 0": (dict(beta1=-0.1), "hyper-parameters"),
    "beta2 = 1": (dict(beta2=1.0), "hyper-parameters"),
    "beta2 < 0": (dict(beta2=-0.1), "hyper-parameters"),
    "eps < 0": (dict(eps=-1e-8), "hyper-parameters"),
    "beta1 nan": (dict(beta1=float("nan")), "hyper-parameters"),
    "beta2 nan": (dict(beta2=float("nan")), "hyper-parameters"),
    "eps nan": (dict(eps=float("nan")), "hyper-parameters"),
}


def refused(name, kw, text, prefix):
    lib().sigsvgd_gram_sym_tile_rows(64, 7)  # (any call in between: the message below is this call's)
    assert call(name, **kw) == BADARG
    assert text in _lib.last_error() and prefix in _lib.last_error(), _lib.last_error()


@pytest.mark.parametrize("case", list(LAUNCH))
@pytest.mark.parametrize("name", NAMES)
def test_launch_rules(name, case):
    refused(name, *LAUNCH[case], "svgd_phi")


@pytest.mark.parametrize("case", list(PARTICLES))
@pytest.mark.parametrize("name", NAMES[:2])
def test_particles_come_in_pairs(name, case):
    refused(name, PARTICLES[case], "both", "svgd_phi")


def test_adagrad_state_alone_is_no_error_of_the_arguments():
    """what the rules above do NOT refuse still gets as far as the next one: a state pointer with a NULL K"""
    refused("sigsvgd_svgd_step", dict(adagrad=FAKE, K=None), "bad arguments", "svgd_phi")


@pytest.mark.parametrize("case", list(ADAM))
def test_adam_rules(case):
    refused("sigsvgd_svgd_adam_step", *ADAM[case], "svgd_adam_step")


@pytest.fixture
def no_library(monkeypatch):
    """`ops` with its device test answered and its launch barred: CPU tensors then reach every check behind the first, and a
    call that gets through all of them fails here instead of in the library"""

    def launch(dev, name, args, *a, **k):
        raise AssertionError(f"ops reached the library: sigsvgd_{name}")

    monkeypatch.setattr(ops, "_require_gpu", lambda *tensors: torch.device("cpu"))
    monkeypatch.setattr(ops, "_launch", launch)


def test_ops_refuse_cpu_tensors_first():
    K, s = torch.eye(4), torch.zeros(4, 3, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.svgd_phi(K, s, s)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.svgd_phi(K, s, s, X=s, lr=0.1, adagrad_state=torch.zeros(4, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.svgd_adam(K, s, s, s, 0.1, ops.AdamState(s))


def test_ops_checks_come_before_the_library(no_library):
    K, s = torch.eye(4), torch.zeros(4, 3, 2)
    st = lambda like=s: ops.AdamState(like)
    with pytest.raises(AssertionError, match="reached the library: sigsvgd_svgd_step"):  # the fixture bars a good call
        ops.svgd_phi(K, s, s, mask=torch.ones(4, 1, 1), X=s, lr=0.1, adagrad_state=torch.zeros(4, 3, 2))
    with pytest.raises(AssertionError, match="reached the library: sigsvgd_svgd_adam_step"):
        ops.svgd_adam(K, s, s, s, 0.1, st())
    for bad_K in (torch.zeros(4, 5), torch.zeros(4), torch.zeros(4, 4, 1)):
        with pytest.raises(ValueError, match="square"):
            ops.svgd_phi(bad_K, s, s)
        with pytest.raises(ValueError, match="square"):
            ops.svgd_adam(bad_K, s, s, s, 0.1, st())
    with pytest.raises(ValueError, match="rows"):  # 8 rows of 3 would pass for 4 rows of 6
        ops.svgd_phi(K, torch.zeros(8, 3), torch.zeros(8, 3))
    with pytest.raises(ValueError, match="rows"):
        ops.svgd_adam(K, torch.zeros(8, 3), torch.zeros(8, 3), torch.zeros(8, 3), 0.1, st(torch.zeros(4, 6)))
    with pytest.raises(ValueError, match="grad_k"):
        ops.svgd_phi(K, s, torch.zeros(4, 3))
    with pytest.raises(ValueError, match="share the shape"):
        ops.svgd_adam(K, s, torch.zeros(4, 3), s, 0.1, st())
    # X of another shape: the kernel would index it, and X_out, by the score's D
    with pytest.raises(ValueError, match="X shape"):
        ops.svgd_phi(K, s, s, X=torch.zeros(4, 3), lr=0.1)
    with pytest.raises(ValueError, match="X shape"):
        ops.svgd_phi(K, s, s, X=torch.zeros(4, 3), lr=0.1, inplace=True)
    with pytest.raises(ValueError, match="share the shape"):
        ops.svgd_adam(K, s, s, torch.zeros(4, 3), 0.1, st())
    with pytest.raises(ValueError, match="share the shape"):
        ops.svgd_adam(K, s, s, s, 0.1, st(torch.zeros(4, 3)))
    half = st()
    half.exp_avg_sq = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="share the shape"):
        ops.svgd_adam(K, s, s, s, 0.1, half)
    for bad_state in (torch.zeros(4, 5), torch.zeros(4, 6, dtype=torch.float64), torch.zeros(6, 4).t()):
        with pytest.raises(ValueError, match="adagrad_state"):
            ops.svgd_phi(K, s, s, X=s, lr=0.1, adagrad_state=bad_state)
    with pytest.raises(ValueError, match="lr is required"):
        ops.svgd_phi(K, s, s, X=s)
    for bad_X in (torch.zeros(2, 3, 4).permute(2, 1, 0), torch.zeros(4, 3, 2, dtype=torch.float64)):
        assert bad_X.shape == s.shape
        with pytest.raises(ValueError, match="inplace"):
            ops.svgd_phi(K, s, s, X=bad_X, lr=0.1, inplace=True)
        with pytest.raises(ValueError, match="inplace"):
            ops.svgd_adam(K, s, s, bad_X, 0.1, st(), inplace=True)
    with pytest.raises(RuntimeError):  # a mask that does not broadcast to the score
        ops.svgd_phi(K, s, s, mask=torch.ones(4, 2, 2))
