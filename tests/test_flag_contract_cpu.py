"""Which entry point of the C ABI takes which flag, as data, and every call's status predicted from it (host only).

CONTRACT is the table of include/sigsvgd_hip.h (asserted equal below): one row per family of entry points, one cell per flag.
`predict` maps a flag word to the status the library must give; the enumeration runs all 8192 words through every entry point
that has a `flags` argument, on small valid arguments, in every gradient form.  The per-flag files (test_exact_adjoint_cpu.py,
test_nan_tails_cpu.py, test_log_k_cpu.py, test_normalized_cpu.py, test_normalized_fused_cpu.py) each cover one bit; this one
covers the matrix, so a new flag is a new column here and a new row of csrc/capi.hip's table."""
import collections
import ctypes
import functools
import re

import pytest
import torch

from cabi import BADARG, FAKE, OK, UNSUPPORTED, WORKSPACE, lib
from sigsvgd_amd import _lib

NAMES = ("NAIVE_SOLVER", "SYM", "Y_IS_X", "FORCE_GENERIC", "WS_CLEAN", "STORED_FORWARD", "FOLD_TILES", "FP32_SWEEPS",
         "EXACT_ADJOINT", "NAN_TAILS", "LOG_K", "NORMALIZED", "NORMALIZED_FUSED")
BITS = tuple(1 << k for k in range(13))
NV, SYM, YX, FG, WC, SF, FOLD, FP32, EX, NT, LK, NM, NF = BITS
WORDS = 1 << 13
DEFINE = {b: "SIGSVGD_FLAG_" + n for b, n in zip(BITS, NAMES)}

# T: taken (acted on)   i: taken and ignored   G: taken by the gradient forms, an unknown bit otherwise
# U: SIGSVGD_E_UNSUPPORTED, "not built for this entry point", ahead of every other check of the flags
# R: SIGSVGD_E_UNSUPPORTED from the choice of kernel (the partial solve has the fp32-sweep kernels only)
# B: an unknown bit, SIGSVGD_E_BADARG (a family without B or G cells does not look for unknown bits)
#                           NV SYM YX FG WC SF FOLD FP32 EX NT LK NM NF
CONTRACT = {
    "gram_workspace_bytes": "T  i   T  T  i  i  i    T    U  i  i  i  T",
    "gram_fwd":             "T  T   T  T  i  i  i    T    i  i  i  i  T",
    "gram_fwd_bwd":         "T  T   T  T  i  i  i    T    U  i  i  i  T",
    "gram_sym_partial":     "R  T   i  R  i  i  T    T    U  i  i  i  U",
    "pde":                  "T  B   B  B  B  B  B    B    G  B  B  B  B",
    "gram_long":            "T  T   i  B  B  B  B    B    G  U  B  B  B",
    "pair":                 "T  B   B  B  B  B  B    B    G  T  T  B  B",
    "gram_long2":           "T  T   T  B  B  B  B    B    G  T  T  T  B",
    "gram_long_h":          "T  T   T  B  B  B  B    B    T  U  B  B  B",
    "pair_h":               "T  B   B  B  B  B  B    B    T  U  B  B  B",
    "gram_long_partial":    "T  T   i  B  B  B  T    B    U  U  B  B  B",
    "sqdist_select":        "B  B   T  B  B  B  B    B    B  B  B  B  B",
}
# the pairs that are not built: SIGSVGD_E_UNSUPPORTED wherever the first flag is taken, before the unknown bits; the message
# names the first flag and the first of the others, in this order
PAIRS = ((NT, (EX,)), (LK, (NV, EX, NT)), (NM, (NV, EX, NT, LK)), (NF, (NV,)))
LONG_ROUTE = ("gram_long", "pair", "gram_long2", "gram_long_h", "pair_h", "gram_long_partial")
TWO_SIDED = ("gram_long2", "gram_long_h")
RBF, IMQ, F64 = _lib.STATIC_RBF, _lib.STATIC_IMQ, _lib.F64


@functools.lru_cache(maxsize=None)
def cells(family, letters):
    """the bits of `family`'s row whose cell is one of `letters`"""
    return sum(b for b, c in zip(BITS, CONTRACT[family].split()) if c in letters)


def misshapen(entry, family, flags, same):
    """the flags that need one shape in both slots, where the slots differ"""
    if same:
        return False
    if entry == "gram_fwd_bwd" or family in TWO_SIDED or family == "sqdist_select":
        return bool(flags & (SYM | YX) & cells(family, "T"))
    return bool(flags & SYM & cells(family, "T")) and entry != "gram_workspace_bytes"


def predict(entry, family, flags, grad, kind=RBF, same=True, gradY=False):
    """-> (status or None where the flags are taken, what the message must name)"""
    fused = family.startswith("gram_") and family not in LONG_ROUTE
    if fused and misshapen(entry, family, flags, same):  # (the fused launches check their shape first)
        return BADARG, ()
    for b in BITS:
        if flags & b & cells(family, "U"):
            return UNSUPPORTED, (DEFINE[b],)
    for flag, others in PAIRS:
        for other in others:
            if flags & flag & cells(family, "T") and flags & other:
                return UNSUPPORTED, (DEFINE[flag], DEFINE[other])
    unknown = flags & (cells(family, "B") | (0 if grad else cells(family, "G")))
    if unknown:
        return BADARG, (f"unknown flag bits 0x{unknown:x} (",)
    if flags & cells(family, "R") or (family == "gram_sym_partial" and kind == IMQ and not flags & FP32):
        return UNSUPPORTED, ()
    if entry == "gram_fwd" and flags & NF and flags & YX and not same:  # (the normalised launch validates its own shape)
        return BADARG, ()
    if not fused and flags & SYM and misshapen(entry, family, flags & SYM, same):
        return BADARG, ()
    if family in LONG_ROUTE and flags & NV and kind == IMQ:  # (fp64 kernels only: default stencil only on the long route)
        return UNSUPPORTED, (DEFINE[NV],)
    if not fused and misshapen(entry, family, flags, same):
        return BADARG, ()
    if family in TWO_SIDED and flags & (SYM | YX) and gradY:  # (they give the first-slot gradient only)
        return BADARG, ()
    return None, ()


# ---- the enumeration ---------------------------------------------------------------------------------------------------------------
Form = collections.namedtuple("Form", "entry family call launch facts")


def forms():
    """every call of the enumeration: (entry point, family, flags -> status, whether it is a launch, predict's other arguments)"""
    L, out = lib(), []
    nbytes, n1, n2 = (ctypes.byref(c) for c in (ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_int(0)))
    nows = (None, 0, None)  # workspace, workspace_bytes, stream
    ptr = {0: None, 1: FAKE}

    def add(entry, family, pre, post, **facts):
        fn = getattr(L, "sigsvgd_" + entry)
        out.append(Form(entry, family, lambda flags: fn(*pre, flags, *post), not entry.endswith(("_bytes", "_plan", "_schedule")),
                        facts))

    # the fused route: A = B = 8 (8 x 5 for the rules of SYM and Y_IS_X), T = 32, d = 2, order 0
    for kind, A, B in ((RBF, 8, 8), (IMQ, 8, 8), (RBF, 8, 5)):
        f = dict(kind=kind, same=A == B)
        for g in (0, 1):
            add("gram_workspace_bytes", "gram_workspace_bytes", (A, B, 32, 2, 0, kind, g), (nbytes,), grad=bool(g), **f)
        launch = (FAKE, FAKE, A, B, 32, 2, F64, 1.0, 0, kind)
        add("gram_fwd", "gram_fwd", launch, (FAKE, *nows), grad=False, **f)
        add("gram_fwd_bwd", "gram_fwd_bwd", launch, (None, FAKE, FAKE, *nows), grad=True, **f)
        if A == B:
            add("gram_sym_partial", "gram_sym_partial", (FAKE, A, 32, 2, F64, 1.0, kind), (0, 1, None, FAKE, FAKE, *nows),
                grad=True, **f)
    # the PDE on a caller's grid: 4 x 30 x 20
    for g in (0, 1):
        add("pde_workspace_bytes", "pde", (4, 30, 20, 0, g), (nbytes,), grad=bool(g))
    add("pde_fwd", "pde", (FAKE, 4, 30, 20, F64, 0), (FAKE, *nows), grad=False)
    add("pde_fwd_bwd", "pde", (FAKE, 4, 30, 20, F64, 0), (None, FAKE, FAKE, *nows), grad=True)
    # the long route: A = B = 3 (3 x 2 for the rules of SYM and Y_IS_X), TX = TY = 300, d = 2, orders 0 and 2, RBF and IMQ
    both = ((0, 0), (1, 0), (0, 1), (1, 1))
    for kind, n, A, B in [(k, n, 3, 3) for k in (RBF, IMQ) for n in (0, 2)] + [(RBF, 0, 3, 2)]:
        f = dict(kind=kind, same=A == B)
        query, launch = (A, B, 300, 300, 2, n, kind), (FAKE, FAKE, A, B, 300, 300, 2, F64, 1.0, n, kind)
        for g in (0, 1):
            add("gram_long_workspace_bytes", "gram_long", (*query, g), (nbytes,), grad=bool(g), **f)
        add("gram_long_fwd", "gram_long", launch, (FAKE, *nows), grad=False, **f)
        add("gram_long_fwd_bwd", "gram_long", launch, (None, FAKE, FAKE, *nows), grad=True, **f)
        for gx, gy in both:
            f2 = dict(gradY=bool(gy), **f)
            add("gram_long2_workspace_bytes", "gram_long2", (*query, gx, gy), (nbytes,), grad=bool(gx or gy), **f2)
            add("gram_long_fwd_bwd2", "gram_long2", launch, (None, FAKE, ptr[gx], ptr[gy], *nows), grad=bool(gx or gy), **f2)
            add("gram_long_h_workspace_bytes", "gram_long_h", (*query, gx, gy), (nbytes,), grad=True, **f2)
            add("gram_long_fwd_bwd_h", "gram_long_h", launch, (None, FAKE, ptr[gx], ptr[gy], FAKE, *nows), grad=True, **f2)
        if A != B:
            continue
        query, launch = (A, 300, 300, 2, n, kind), (FAKE, FAKE, A, 300, 300, 2, F64, 1.0, n, kind)
        for g in (0, 1):
            add("pair_workspace_bytes", "pair", (*query, g), (nbytes,), grad=bool(g), **f)
            add("pair_schedule", "pair", (*query, g), (n1, n2, nbytes), grad=bool(g), **f)
        add("pair_fwd", "pair", launch, (FAKE, *nows), grad=False, **f)
        add("pair_h_workspace_bytes", "pair_h", query, (nbytes,), grad=True, **f)
        for gx, gy in both:
            if gx or gy:
                add("pair_fwd_bwd", "pair", launch, (None, FAKE, ptr[gx], ptr[gy], *nows), grad=True, **f)
            add("pair_fwd_bwd_h", "pair_h", launch, (None, FAKE, ptr[gx], ptr[gy], FAKE, *nows), grad=True, **f)
        part = (6, 300, 2, n, kind)
        add("gram_long_partial_plan", "gram_long_partial", part, (2, n1, n2), grad=True, **f)
        add("gram_long_partial_workspace_bytes", "gram_long_partial", part, (0, 2, nbytes), grad=True, **f)
        add("gram_long_sym_partial", "gram_long_partial", (FAKE, 6, 300, 2, F64, 1.0, n, kind),
            (0, 2, None, FAKE, FAKE, *nows), grad=True, **f)
    for A, B in ((4, 4), (4, 3)):
        add("sqdist_select_workspace_bytes", "sqdist_select", (A, B, 9, 9, 2), (nbytes,), grad=False, same=A == B)
        add("sqdist_select", "sqdist_select", (FAKE, FAKE, A, B, 9, 9, 2, F64), (0, FAKE, *nows), grad=False, same=A == B)
    return out


ENTRIES = sorted(name[len("sigsvgd_"):] for name, argtypes in _lib.ARGTYPES.items() if ctypes.c_uint in argtypes)
FEW_SET = frozenset(w for w in range(WORDS) if bin(w).count("1") <= 3)  # (the words whose messages are read too)
HIP = _lib.E_HIP


def no_workspace(form, flags):
    """the launches that store nothing outside their outputs: the forward-only ones of the PDE and of the long route's plain
    solve (the variable-length, log-domain and normalised solves keep lengths, exponents or diagonals there)"""
    return (form.family in ("pde", "gram_long", "pair", "gram_long2") and not form.facts["grad"]
            and not flags & (NT | LK | NM))


def run(entry, launches, words=range(WORDS)):
    mine = [f for f in forms() if f.entry == entry and f.launch == launches]
    wrong = []
    for form in mine:
        for flags in words:
            want, named = predict(form.entry, form.family, flags, **form.facts)
            if want is None:  # (taken: a query answers, a launch stops at its workspace -- or, where it needs none, at its
                want = OK if not form.launch else HIP if no_workspace(form, flags) else WORKSPACE  # first HIP call: no device)
            rc = form.call(flags)
            if rc != want:
                wrong.append((hex(flags), form.facts, rc, want, _lib.last_error()))
            elif flags in FEW_SET and not all(n in _lib.last_error() for n in named):
                wrong.append((hex(flags), form.facts, rc, named, _lib.last_error()))
    return len(mine), wrong


def test_every_entry_point_with_flags_is_enumerated():
    assert len(ENTRIES) == 25
    assert sorted({f.entry for f in forms()}) == ENTRIES
    assert {f.family for f in forms()} == set(CONTRACT)


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e.endswith(("_bytes", "_plan", "_schedule"))])
def test_query_answers_every_flag_word_as_the_table_says(entry):
    count, wrong = run(entry, launches=False)
    assert count and not wrong, (len(wrong), wrong[:8])


@pytest.mark.parametrize("entry", [e for e in ENTRIES if not e.endswith(("_bytes", "_plan", "_schedule"))])
def test_launch_answers_every_flag_word_as_the_table_says(entry):
    """dummy pointers and no workspace: a launch whose flags are taken stops at SIGSVGD_E_WORKSPACE, before any device work --
    or, the launches of `no_workspace`, at SIGSVGD_E_HIP for want of a device, which is why a HIP device skips this test"""
    if torch.cuda.is_available():
        pytest.skip("the dummy pointers must not reach a kernel launch on a HIP device")
    count, wrong = run(entry, launches=True)
    assert count and not wrong, (len(wrong), wrong[:8])


def test_the_header_states_the_same_table():
    header = open(_lib.HEADERS[-1]).read()
    row = re.compile(r"^ \* (\w+)((?:\s+[TiGURB]){13})\s*$", re.M)
    stated = {name: " ".join(c.split()) for name, c in row.findall(header)}
    assert stated == {family: " ".join(c.split()) for family, c in CONTRACT.items()}
    assert re.search(r"^ \*\s+NV\s+SYM\s+YX\s+FG\s+WC\s+SF\s+FOLD\s+FP32\s+EX\s+NT\s+LK\s+NM\s+NF\s*$", header, re.M)
