"""The self-attention K cache layout (csrc/swx_kernels.h: KLayout / swx_kidx), host side, no GPU: the index function every reader and
writer of the cache goes through is a bijection of a cache row onto itself, states the documented formula, and the re-layout helper
(row-major -> chunked -> row-major) returns the original array."""
import ctypes

import numpy as np
import pytest

SHAPES = [(6, 448), (20, 448), (8, 64)]          # (H, n_ctx)


@pytest.fixture(scope="module")
def lib():
    from stable_ts_amd import _lib
    return _lib.load()


def _offsets(lib, chunked, H, n_ctx):
    d = 64 * H
    off = np.empty((n_ctx, H, 8), np.int64)
    for pos in range(n_ctx):
        for h in range(H):
            for c in range(8):
                off[pos, h, c] = lib.swx_test_kcache_index(chunked, n_ctx, d, pos, h, c)
    return off


@pytest.mark.parametrize("H,n_ctx", SHAPES)
def test_index_function_is_a_bijection_of_the_row(lib, H, n_ctx):
    d = 64 * H
    for chunked in (0, 1):
        off = _offsets(lib, chunked, H, n_ctx)
        assert off.min() == 0 and off.max() == n_ctx * d - 8 and (off % 8 == 0).all()
        # every 8-element chunk of the row is hit exactly once -> with the 8 dims of a chunk contiguous, every element is
        assert np.array_equal(np.sort(off.ravel()), np.arange(0, n_ctx * d, 8))
    pos, h, c = np.meshgrid(np.arange(n_ctx), np.arange(H), np.arange(8), indexing="ij")
    assert np.array_equal(_offsets(lib, 0, H, n_ctx), (pos * H + h) * 64 + c * 8)
    assert np.array_equal(_offsets(lib, 1, H, n_ctx), ((h * 8 + c) * n_ctx + pos) * 8)


def test_index_function_refuses_arguments_out_of_range(lib):
    for args in ((1, 448, 384, 448, 0, 0), (1, 448, 384, 0, 6, 0), (1, 448, 384, 0, 0, 8), (1, 448, 380, 0, 0, 0), (0, 0, 384, 0, 0, 0),
                 (1, 448, 384, -1, 0, 0)):
        assert lib.swx_test_kcache_index(*args) < 0, args


@pytest.mark.parametrize("H,n_ctx", SHAPES)
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_relayout_there_and_back(lib, H, n_ctx, dtype):
    d, rows = 64 * H, 3
    a = np.arange(rows * n_ctx * d, dtype=np.int64).astype(dtype if dtype == np.float32 else np.uint16).view(dtype).reshape(rows, n_ctx, d)
    a = np.ascontiguousarray(a)
    b, c = np.zeros_like(a), np.zeros_like(a)
    p = lambda x: ctypes.c_void_p(x.ctypes.data)
    assert lib.swx_test_kcache_relayout(p(a), p(b), rows, n_ctx, d, a.itemsize, 1) == 0
    assert lib.swx_test_kcache_relayout(p(b), p(c), rows, n_ctx, d, a.itemsize, 0) == 0
    bits = np.uint16 if dtype == np.float16 else np.uint32
    assert np.array_equal(c.view(bits), a.view(bits))
    # ... and the chunked array is the documented one: [rows][H][8][n_ctx][8]
    want = a.view(bits).reshape(rows, n_ctx, H, 8, 8).transpose(0, 2, 3, 1, 4)
    assert np.array_equal(b.view(bits).reshape(rows, H, 8, n_ctx, 8), want)
    assert lib.swx_test_kcache_relayout(p(a), p(a), rows, n_ctx, d, a.itemsize, 1) < 0       # in place is refused
