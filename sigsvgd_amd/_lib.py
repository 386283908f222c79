"""ctypes binding of libsigsvgd_hip.so (C ABI in include/sigsvgd_hip.h) + in-tree build helper.

There is deliberately NO fallback: if the shared library is missing or fails to load, every hot-path
op raises.  `build()` cross-compiles for gfx950 with hipcc (works without a GPU).
"""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_PKG, "csrc")
# SIGSVGD_LIB_PATH: A/B benchmarking of two builds on the same GPU box (scripts/ab.py); never set in tests
LIB_PATH = os.environ.get("SIGSVGD_LIB_PATH") or os.path.join(_PKG, "libsigsvgd_hip.so")
SOURCES = ["capi.hip", "gram_generic.hip", "gram_fast.hip", "gram_fast_radial.hip", "gram_fast_wide.hip", "sweep_host.hip",
           "gram_quad.hip", "svgd_phi.hip", "vec_kernels.hip", "vec_fused.hip", "cost_kernels.hip", "sig_backward.hip", "gram_dyad.hip",
           "gram_band.hip", "sig_pde.hip", "gram_long.hip", "gram_long_matern.hip", "pair_bands.hip", "pair_bands_f32.hip",
           "pair_bands_matern.hip", "sqdist_select.hip", "sig_pde_exact.hip", "gram_long_exact.hip",
           "gram_long_exact_matern.hip", "gram_long_nantail.hip", "gram_long_nantail_matern.hip", "gram_long_logk.hip",
           "gram_long_logk_matern.hip", "gram_long_norm.hip", "gram_long_norm_matern.hip", "gram_norm_fused.hip"]
# every header of csrc/ (a source includes headers only), then the public header, which stays the last element
HEADERS = [os.path.join(_CSRC, h) for h in ("sig_common.h", "sweep_scaffold.h", "quad_sweeps.h", "ring_sweep.h", "long_static.h",
                                            "pair_bands.h", "gram_fast_kernel.h", "gram_long_kernels.h", "pair_bands_kernel.h",
                                            "sig_pde_kernel.h")] + \
          [os.path.join(_PKG, "..", "include", "sigsvgd_hip.h")]

# mirror of include/sigsvgd_hip.h
F32, F64 = 0, 1
STATIC_RBF, STATIC_LINEAR, STATIC_IMQ, STATIC_RQ = 0, 1, 2, 3
STATIC_MATERN32, STATIC_MATERN52 = 6, 7  # (4 and 5 are reserved: the library refuses them)
FLAG_NAIVE_SOLVER, FLAG_SYM, FLAG_Y_IS_X, FLAG_FORCE_GENERIC, FLAG_WS_CLEAN, FLAG_STORED_FORWARD = 1, 2, 4, 8, 16, 32
FLAG_FOLD_TILES = 64
FLAG_FP32_SWEEPS = 128
FLAG_EXACT_ADJOINT = 256
FLAG_NAN_TAILS = 512
FLAG_LOG_K = 1024
FLAG_NORMALIZED = 2048
FLAG_NORMALIZED_FUSED = 4096
VEC_GAUSSIAN, VEC_IMQ, VEC_UNIT = 0, 1, 2
E_BADARG, E_UNSUPPORTED, E_WORKSPACE, E_HIP = -1, -2, -3, -4
ABI_VERSION = 10

# Every entry point of include/sigsvgd_hip.h with its argtypes: a new one is declared here and nowhere else (`load` applies the
# table, EXPORTS lists its names).  All return int except sigsvgd_last_error, a string.
_vp, _ci, _cd, _cu, _cf, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_uint, ctypes.c_float, ctypes.c_size_t
_out = ctypes.POINTER
ARGTYPES = {
    "sigsvgd_abi_version": [],
    "sigsvgd_last_error": [],
    "sigsvgd_gram_workspace_bytes": [_ci, _ci, _ci, _ci, _ci, _ci, _ci, _cu, _out(_sz)],
    "sigsvgd_gram_fwd": [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _cd, _ci, _ci, _cu, _vp, _vp, _sz, _vp],
    "sigsvgd_gram_fwd_bwd": [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _cd, _ci, _ci, _cu, _vp, _vp, _vp, _vp, _sz, _vp],
    "sigsvgd_gram_sym_partial": [_vp, _ci, _ci, _ci, _ci, _cd, _ci, _cu, _ci, _ci, _vp, _vp, _vp, _vp, _sz, _vp],
    "sigsvgd_gram_sym_tile_rows": [_ci, _ci],
    "sigsvgd_svgd_phi": [_vp, _vp, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _cf, _vp],
    "sigsvgd_svgd_step": [_vp, _vp, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _cf, _vp, _vp],
    "sigsvgd_svgd_adam_step": [_vp, _vp, _vp, _vp, _ci, _ci, _vp, _vp, _vp, _cd, _cd, _cd, _cd, _vp, _vp, _vp, _vp],
    "sigsvgd_svgd_update": [_vp, _vp, _ci, _ci, _vp, _vp, _vp, _cd, _vp, _vp, _vp, _vp, _cd, _cd, _cd, _vp],
    "sigsvgd_vec_sqdist": [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _vp],
    "sigsvgd_vec_kernel": [_vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _cd, _cd, _vp, _vp, _vp],
    "sigsvgd_vec_kernel_fused": [_vp, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _cd, _cd, _vp, _vp, _vp, _sz, _vp],
    "sigsvgd_vec_fused_workspace_bytes": [_ci, _ci, _ci, _out(_sz)],
    "sigsvgd_signature": [_vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _out(ctypes.c_longlong), _vp],
    "sigsvgd_signature_backward": [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _vp],
    "sigsvgd_obstacle_cost": [_vp, _ci, _ci, _ci, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _ci, _cf, _cf, _vp, _vp, _vp, _vp],
    "sigsvgd_pde_workspace_bytes": [_ci, _ci, _ci, _ci, _ci, _cu, _out(_sz)],
    "sigsvgd_pde_fwd": [_vp, _ci, _ci, _ci, _ci, _ci, _cu, _vp, _vp, _sz, _vp],
    "sigsvgd_pde_fwd_bwd": [_vp, _ci, _ci, _ci, _ci, _ci, _cu, _vp, _vp, _vp, _vp, _sz, _vp],
    "sigsvgd_gram_long_workspace_bytes": [_ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _cu, _out(_sz)],
    "sigsvgd_gram_long_fwd": [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _cd, _ci, _ci, _cu, _vp, _vp, _sz, _vp],
    "sigsvgd_gram_long_fwd_bwd": [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _cd, _ci, _ci, _cu, _vp, _vp, _vp, _vp, _sz, _vp],
    "sigsvgd_pair_workspace_bytes": [_ci, _ci, _ci, _ci, _ci, _ci, _ci, _cu, _out(_sz)],
    "sigsvgd_pair_fwd": [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _cd, _ci, _ci, _cu, _vp, _vp, _sz, _vp],
    "sigsvgd_pair_fwd_bwd": [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _cd, _ci, _ci, _cu, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "sigsvgd_pair_schedule": [_ci, _ci, _ci, _ci, _ci, _ci, _ci, _cu, _out(_ci), _out(_ci), _out(_sz)],
    "sigsvgd_gram_long2_workspace_bytes": [_ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _cu, _out(_sz)],
    "sigsvgd_gram_long_fwd_bwd2": [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _cd, _ci, _ci, _cu, _vp, _vp, _vp, _vp, _vp, _sz,
                                   _vp],
    "sigsvgd_gram_long_h_workspace_bytes": [_ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _cu, _out(_sz)],
    "sigsvgd_gram_long_fwd_bwd_h": [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _cd, _ci, _ci, _cu, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _sz, _vp],
    "sigsvgd_pair_h_workspace_bytes": [_ci, _ci, _ci, _ci, _ci, _ci, _cu, _out(_sz)],
    "sigsvgd_pair_fwd_bwd_h": [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _cd, _ci, _ci, _cu, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "sigsvgd_gram_long_partial_plan": [_ci, _ci, _ci, _ci, _ci, _cu, _ci, _out(_ci), _out(_ci)],
    "sigsvgd_gram_long_partial_workspace_bytes": [_ci, _ci, _ci, _ci, _ci, _cu, _ci, _ci, _out(_sz)],
    "sigsvgd_gram_long_sym_partial": [_vp, _ci, _ci, _ci, _ci, _cd, _ci, _ci, _cu, _ci, _ci, _vp, _vp, _vp, _vp, _sz, _vp],
    "sigsvgd_sqdist_select_workspace_bytes": [_ci, _ci, _ci, _ci, _ci, _cu, _out(_sz)],
    "sigsvgd_sqdist_select": [_vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _cu, ctypes.c_ulonglong, _vp, _vp, _sz, _vp],
}
EXPORTS = list(ARGTYPES)

_lib = None


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm's hipcc to build libsigsvgd_hip.so)")


def needs_build() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(_CSRC, s) for s in SOURCES] + HEADERS
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build(force: bool = False, verbose: bool = False, out_path: str = None, objdir: str = None, defines=()) -> str:
    """hipcc --offload-arch=gfx950 -shared -> sigsvgd_amd/libsigsvgd_hip.so (in-tree).  `out_path` / `objdir`: build somewhere
    else from scratch (tests/test_cabi.py builds into a temporary directory to show the sources alone produce the library;
    scripts/dev builds diagnostic variants with `defines`)."""
    if out_path is not None:
        return _build_to(out_path, objdir or os.path.join(os.path.dirname(out_path), "_obj"), verbose, tuple(defines))
    if not force and not needs_build():
        return LIB_PATH
    return _build_to(LIB_PATH, os.path.join(_PKG, "_obj"), verbose, tuple(defines))


def _build_to(lib_path: str, objdir: str, verbose: bool, defines=()) -> str:
    # one hipcc per source, side by side (the four pair-solver files take 30-50 s each, the two
    # of pair_bands about 2 min each: 7 min in a row, 2 min in parallel),
    # then one link; objects under sigsvgd_amd/_obj/ (git-ignored)
    from concurrent.futures import ThreadPoolExecutor

    os.makedirs(objdir, exist_ok=True)
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + [f"-D{d}" for d in defines]

    def compile_one(src):
        obj = os.path.join(objdir, os.path.splitext(src)[0] + ".o")
        cmd = [_hipcc()] + flags + ["-c", os.path.join(_CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{r.stderr}")
        return obj

    with ThreadPoolExecutor(max_workers=min(len(SOURCES), max(1, (os.cpu_count() or 2) - 1))) as pool:
        objs = list(pool.map(compile_one, SOURCES))
    cmd = [_hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared", "-o", lib_path] + objs + ["-ldl"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    _check_dpp_hazards(lib_path)
    return lib_path


def _check_dpp_hazards(lib_path: str) -> None:
    """The kernels' inline-asm DPP moves/adds rely on hipcc's schedule for the 2 wait states after a VALU
    write of their source (csrc/gram_fast_kernel.h); verify that on the disassembly of what was just built and
    refuse the library otherwise (scripts/check_dpp_hazards.py)."""
    import importlib.util

    script = os.path.join(_PKG, "..", "scripts", "check_dpp_hazards.py")
    if not os.path.exists(script):
        return
    spec = importlib.util.spec_from_file_location("check_dpp_hazards", script)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    total, bad = 0, []
    for text in mod.disassemble(lib_path):
        n, b = mod.check_disassembly(text)
        total += n
        bad += b
    if bad or total == 0:
        os.replace(lib_path, lib_path + ".rejected")
        raise RuntimeError(f"sigsvgd_amd: {len(bad)} DPP data hazards (of {total} DPP instructions) in the library "
                           f"hipcc produced, e.g. {bad[:2]}; kept as {lib_path}.rejected")


def load():
    """Load the library and declare signatures.  Raises RuntimeError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"sigsvgd_amd: HIP extension {LIB_PATH} is not built; run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). There is no CPU fallback."
        )
    # PyTorch-ROCm ships its own libamdhip64/libhsa-runtime64; they must be the ones already in the
    # process when this library's NEEDED entries are resolved, or two HIP runtimes end up loaded
    # (symptom: "no ROCm-capable device is detected" from the second one).
    import torch  # noqa: F401

    L = ctypes.CDLL(LIB_PATH)
    for name, argtypes in ARGTYPES.items():
        fn = getattr(L, name)
        fn.restype = ctypes.c_char_p if name == "sigsvgd_last_error" else ctypes.c_int
        fn.argtypes = argtypes
    if L.sigsvgd_abi_version() != ABI_VERSION:
        raise RuntimeError("sigsvgd_amd: libsigsvgd_hip.so ABI version mismatch; rebuild it")
    _lib = L
    return L


def last_error() -> str:
    return load().sigsvgd_last_error().decode("utf-8", "replace")


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"sigsvgd_amd: {what} failed (rc={rc}): {last_error()}")
