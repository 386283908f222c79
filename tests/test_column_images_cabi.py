"""Host only: the workspace of the column images (gram_fast.hip, `colimg`; DESIGN.md 5.1, "Column images").

Symmetric Gram + gradient launches of 64-point paths in 7 channels run the half-offset twin that stages every column from an
image formed once per launch: [64][8] doubles as the kernel's LDS holds a column and the 8 doubles of its first point, 4,160 B
per column, in an area behind the column slab (rounded up to 256 B like every area).  The plan records the choice, so the query
and the launch agree: with SIGSVGD_COLUMN_IMAGES=off, or SIGSVGD_HALF_OFFSET=off, the query is the one without the area, and
the ordered query, d = 8 and T = 63 -- launches that never reach the twin -- do not move with the switch."""
import ctypes

import pytest

from cabi import lib
from plans import device_cus, gram_ordered_grad_bytes
from sigsvgd_amd import _lib

HOOK = "SIGSVGD_COLUMN_IMAGES"
IMAGE_BYTES = (64 * 8 + 8) * 8  # per column


def image_area(B):
    return (B * IMAGE_BYTES + 255) & ~255


def query(A, B, T, d, flags):
    b = ctypes.c_size_t(0)
    assert lib().sigsvgd_gram_workspace_bytes(A, B, T, d, 0, _lib.STATIC_RBF, 1, flags, ctypes.byref(b)) == 0, _lib.last_error()
    return b.value


def on_off(monkeypatch, *args):
    monkeypatch.delenv(HOOK, raising=False)
    on = query(*args)
    monkeypatch.setenv(HOOK, "off")
    off = query(*args)
    monkeypatch.delenv(HOOK, raising=False)
    return on, off


def sym_bytes_without_images(N, cus):
    """[row segments of (tiles + grid) x 8 paths, fp64][column slab: one fp32 path per item] + 256 (gram_fast.hip's fast_plan)"""
    r256 = lambda b: (b + 255) & ~255
    ntile = -(-N // 8)
    items = sum(N - 8 * t for t in range(ntile))
    grid = min(items, cus)
    return r256((ntile + grid) * 8 * 448 * 8) + r256(items * 448 * 4) + 256


@pytest.mark.parametrize("N", [8, 9, 17, 24, 200, 1024])
def test_symmetric_query_grows_by_the_image_area(monkeypatch, N):
    monkeypatch.delenv("SIGSVGD_HALF_OFFSET", raising=False)
    assert IMAGE_BYTES == 4160
    on, off = on_off(monkeypatch, N, N, 64, 7, _lib.FLAG_Y_IS_X)
    assert off == sym_bytes_without_images(N, device_cus())
    assert on == off + image_area(N)
    if N % 16 == 0:
        assert on - off == N * IMAGE_BYTES


def test_without_the_half_offset_twin_there_are_no_images(monkeypatch):
    monkeypatch.setenv("SIGSVGD_HALF_OFFSET", "off")
    on, off = on_off(monkeypatch, 200, 200, 64, 7, _lib.FLAG_Y_IS_X)
    assert on == off == sym_bytes_without_images(200, device_cus())


@pytest.mark.parametrize("T,d", [(64, 8), (63, 7), (64, 6), (32, 7)])
def test_other_symmetric_shapes_are_unchanged(monkeypatch, T, d):
    monkeypatch.delenv("SIGSVGD_HALF_OFFSET", raising=False)
    on, off = on_off(monkeypatch, 200, 200, T, d, _lib.FLAG_Y_IS_X)
    assert on == off


def test_ordered_queries_are_unchanged(monkeypatch):
    monkeypatch.delenv("SIGSVGD_HALF_OFFSET", raising=False)
    for (A, B) in [(43, 97), (300, 8), (8, 300)]:
        on, off = on_off(monkeypatch, A, B, 64, 7, 0)
        assert on == off == gram_ordered_grad_bytes(A, B, 64, 7, 0, device_cus())


@pytest.mark.parametrize("kind", [_lib.STATIC_IMQ, _lib.STATIC_RQ])
def test_radial_kinds_are_sized_like_the_rbf_launch(monkeypatch, kind):
    """IMQ / rational quadratic with SIGSVGD_FLAG_FP32_SWEEPS: the RBF launch's workspace (tests/test_fp32_static_cabi.py), the
    image area included although their kernels do not read it -- on either setting of the switch"""
    monkeypatch.delenv("SIGSVGD_HALF_OFFSET", raising=False)
    flags = _lib.FLAG_Y_IS_X | _lib.FLAG_FP32_SWEEPS
    for hook in (None, "off"):
        if hook:
            monkeypatch.setenv(HOOK, hook)
        else:
            monkeypatch.delenv(HOOK, raising=False)
        b = ctypes.c_size_t(0)
        assert lib().sigsvgd_gram_workspace_bytes(17, 17, 64, 7, 0, kind, 1, flags, ctypes.byref(b)) == 0, _lib.last_error()
        assert b.value == query(17, 17, 64, 7, _lib.FLAG_Y_IS_X)
    monkeypatch.delenv(HOOK, raising=False)


def test_square_query_without_the_flag_covers_the_symmetric_launch(monkeypatch):
    """A == B without Y_IS_X covers the ordered and the symmetric launch: the larger of the two, so it never shrinks"""
    monkeypatch.delenv("SIGSVGD_HALF_OFFSET", raising=False)
    on, off = on_off(monkeypatch, 1024, 1024, 64, 7, 0)
    assert on == off + image_area(1024)
    assert on == query(1024, 1024, 64, 7, _lib.FLAG_Y_IS_X)
