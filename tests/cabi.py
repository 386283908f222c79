"""What the host-only C-ABI tests (test_*_cabi.py) share: the library handle, the status codes of include/sigsvgd_hip.h, a
pointer no call dereferences, and the export check of an entry point.  (tests/test_cabi.py has its own `lib`, which builds
the library where it is missing; the one here never builds.)"""
import ctypes
import re
import subprocess

import pytest

from sigsvgd_amd import _lib

OK, BADARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
FAKE = ctypes.c_void_p(4096)  # never dereferenced: every call that takes it fails its argument checks first


def lib():
    try:
        return _lib.load()
    except RuntimeError as e:
        pytest.fail(f"library not built: {e}")


def exported_symbols():
    """the sigsvgd_* functions the shared library defines, from its dynamic symbol table"""
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r"\bT (sigsvgd_\w+)", syms))


def assert_exported(names, abi=10):
    """every name is defined by the library, listed in `_lib.EXPORTS` and bound by ctypes; the ABI version is `abi`"""
    exported = exported_symbols()
    for name in names:
        assert name in exported and name in _lib.EXPORTS
        getattr(lib(), name)
    assert lib().sigsvgd_abi_version() == _lib.ABI_VERSION == abi
