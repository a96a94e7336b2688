"""Helpers of tests/test_frame_taps.py: the digest and the difference histogram of a texture tap (include/wrhip.h,
WrhipTapTexture) restated in numpy, and the mapping from a tap rect to the bytes the harness reads back.

Stored bytes.  A tap reduces pixels as the texture stores them: RGBA8 textures hold B, G, R, A, and row r of a rect at (x, y) is
texture row y + r.
  Device.read_texture    returns the stored bytes (GL_BGRA / GL_RED), texture row 0 first: stored_words() of it, as it is
  Renderer.read_pixels   returns the window through glReadPixels(GL_RGBA): R and B swapped back, rows in the same order -- row 0
                         of the array is texture row 0 (window_stored)
The row order is checked once, by test_*_row_orientation, on a frame whose top and bottom halves differ."""
import numpy as np

C0, C1 = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
M1, M2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def stored_words(px):
    """(h, w, 4) stored bytes -> (h, w) little-endian words; an (h, w) R8 array -> its bytes, widened"""
    px = np.ascontiguousarray(px)
    if px.ndim == 3:
        assert px.shape[2] == 4 and px.dtype == np.uint8
        return px.view("<u4")[:, :, 0].astype(np.uint64)
    return px.astype(np.uint64)


def window_stored(rgba):
    """Renderer.read_pixels / render_direct's window (RGBA bytes) -> the bytes the window texture stores (BGRA)"""
    return np.ascontiguousarray(rgba[:, :, [2, 1, 0, 3]])


def crop(px, rect):
    x, y, w, h = rect
    assert 0 <= x and 0 <= y and x + w <= px.shape[1] and y + h <= px.shape[0]
    return px[y:y + h, x:x + w]


def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(M1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(M2)
    return z ^ (z >> np.uint64(31))


def digest(px):
    """The two 64-bit sums of a rect's stored pixels (all of `px`), as Python ints"""
    v = stored_words(px).ravel()
    k = (np.arange(v.size, dtype=np.uint64) << np.uint64(32)) | v
    out = []
    for c in (C0, C1):
        with np.errstate(over="ignore"):
            z = _mix(k + np.uint64(c))
            out.append(int(np.add.reduce(z, dtype=np.uint64)))
    return tuple(out)


def differences(a, b):
    """wrench's per-pixel difference of two stored arrays of one shape: the largest absolute channel difference"""
    assert a.shape == b.shape and a.dtype == np.uint8 and b.dtype == np.uint8
    d = np.abs(a.astype(np.int16) - b.astype(np.int16))
    return d.max(axis=2) if d.ndim == 3 else d


def histogram(a, b):
    """-> (hist over all pixels as a list of 256, max difference, differing pixels)"""
    d = differences(a, b)
    hist = np.bincount(d.ravel(), minlength=256)
    return [int(n) for n in hist], int(d.max()), int((d > 0).sum())


def check_digest(res, px, fmt):
    """A tap result without an expected texture against the stored bytes `px` of its rect"""
    h, w = px.shape[:2]
    assert (res["status"], res["width"], res["height"], res["format"]) == (0, w, h, fmt), res
    assert tuple(res["digest"]) == digest(px), (res["digest"], digest(px))
    assert res["hist"][0] == w * h and sum(res["hist"]) == w * h
    assert res["max_diff"] == 0 and res["differing"] == 0
