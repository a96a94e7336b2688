"""The reference's reftest comparison, restated once (wrench/src/reftest.rs), over the fixtures of tests/golden/make_reftest_pngs.py.

  compare()      ReftestImage::compare (reftest.rs:267-304): a pixel differs if any of its four channels differs, its difference is the
                 max over the channels; -> (max difference, differing pixels, histogram over the differing pixels)
  within_fuzz()  Reftest::check_and_report_equality_failure (:121-210): range j bounds the number of pixels whose difference is above
                 range j-1's max and at or below its own; nothing above the last range's max is allowed
  region()       what wrench compares: the image-sized BOTTOM-LEFT rectangle of the GL framebuffer (:949-954) against the PNG flipped on
                 load (:913-922) -- in display orientation, the image-sized top-left corner of the window.  render_direct returns the
                 window as glReadPixels does, bottom row first.
"""
import json
import os
import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_fx = None


def fixtures():
    """-> (json document, {manifest line: RGBA8 pixels, first row = top of the window})"""
    global _fx
    if _fx is None:
        with open(os.path.join(GOLDEN, "reftest_png.json")) as f:
            doc = json.load(f)
        with np.load(os.path.join(GOLDEN, "reftest_png.npz")) as z:
            _fx = (doc, {k: z[k] for k in z.files})
    return _fx


def region(window, size, upside_down=False):
    w, h = size
    shown = window if upside_down else window[::-1]
    return shown[:h, :w]


def compare(a, b):
    assert a.shape == b.shape and a.dtype == np.uint8 and b.dtype == np.uint8
    d = np.abs(a.astype(np.int16) - b.astype(np.int16)).max(axis=2)
    hist = np.bincount(d[d > 0].ravel(), minlength=256)
    return int(d.max()), int((d > 0).sum()), hist


def within_fuzz(hist, fuzz):
    prefix = np.cumsum(hist)
    prev = 0
    ok = True
    for max_diff, num in fuzz:
        m = min(255, int(max_diff))
        ok &= int(prefix[m] - prev) <= int(num)
        prev = int(prefix[m])
    return bool(ok and int(prefix[255] - prev) == 0)
