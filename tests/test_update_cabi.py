"""Host-side checks of `sigsvgd_svgd_update` (include/sigsvgd_hip.h): the symbol, the ABI version it leaves alone, and every
argument rule, each refused with SIGSVGD_E_BADARG and a message before any device work (no device needed: no call below gets
past its argument checks), and of the checks `ops.svgd_update` makes before it reaches the library."""
import re

import pytest
import torch

from cabi import assert_exported, BADARG, FAKE, lib
from sigsvgd_amd import _lib, ops

NAME = "sigsvgd_svgd_update"


def update(v_in=FAKE, mask=None, N=4, D=6, v_out=FAKE, X_in=FAKE, X_out=FAKE, lr=0.1, adagrad=None, exp_avg=None,
           exp_avg_sq=None, step=None, beta1=0.9, beta2=0.999, eps=1e-8):
    return lib().sigsvgd_svgd_update(v_in, mask, N, D, v_out, X_in, X_out, lr, adagrad, exp_avg, exp_avg_sq, step, beta1,
                                     beta2, eps, None)


def test_update_symbol_exported():
    assert_exported((NAME,), abi=10)  # an added entry point: the version stays
    with open(_lib.HEADERS[-1]) as f:
        assert len(re.findall(r"^int " + NAME + r"\(", f.read(), flags=re.M)) == 1


ADAM = dict(exp_avg=FAKE, exp_avg_sq=FAKE, step=FAKE)
CASES = {
    "N<1": (dict(N=0), "N=0"),
    "D<1": (dict(D=0), "D=0"),
    "v_in NULL": (dict(v_in=None), "bad arguments"),
    "X_in only": (dict(X_out=None), "both"),
    "X_out only": (dict(X_in=None), "both"),
    "adam without exp_avg_sq": (dict(ADAM, exp_avg_sq=None), "Adam needs"),
    "adam without exp_avg": (dict(ADAM, exp_avg=None), "Adam needs"),
    "adam without the counter": (dict(ADAM, step=None), "Adam needs"),
    "adam without X": (dict(ADAM, X_in=None, X_out=None), "Adam needs"),
    "adam with adagrad": (dict(ADAM, adagrad=FAKE), "Adam needs"),
    "beta1": (dict(ADAM, beta1=1.0), "hyper-parameters"),
    "beta2": (dict(ADAM, beta2=-0.1), "hyper-parameters"),
    "eps": (dict(ADAM, eps=-1e-8), "hyper-parameters"),
    "beta nan": (dict(ADAM, beta1=float("nan")), "hyper-parameters"),
    "nothing to write": (dict(v_out=None, X_in=None, X_out=None), "nothing to write"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_update_bad_arguments(case):
    kw, text = CASES[case]
    lib().sigsvgd_gram_sym_tile_rows(64, 7)  # (any call in between: the message below is this call's)
    assert update(**kw) == BADARG
    assert text in _lib.last_error(), _lib.last_error()
    assert "svgd_update" in _lib.last_error()


def test_ops_checks_come_first():
    """`ops.svgd_update` refuses CPU tensors (there is no CPU path) and, like `ops.svgd_phi` / `ops.svgd_adam`, mismatched
    shapes and state before any launch"""
    v, X = torch.zeros(4, 3, 2), torch.zeros(4, 3, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.svgd_update(v, X, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.svgd_update(v, X, 0.1, adam=ops.AdamState(X))
    assert "svgd_update" in ops.__dict__ and ops.svgd_update.__doc__
