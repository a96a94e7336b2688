"""Frame sequences for the streamed parity tests (harness.render_streamed): shared by tests/test_stream_parity.py (host simulation) and
tests/test_gpu_parity.py (MI355X).  Every sequence is checked by its LAST frame, against the oracle's render of that frame alone.

The per-flush scratch of libwrhip comes in two sets used alternately (flush_seq & 1), each grown to twice what a flush needed when it
falls short.  A growth sequence sets both up with two frames, then asks more of set 0 in the third, for one buffer only: the prims, bin
counters and pool still fit, the coverage masks (n_words) or the vertex tables (vtab_cursor) do not.  That third flush replaces the buffers
while the second one's raster launches are held back (Context::Tail, WrhipStats::scratch_grown_held)."""
import numpy as np
from webrender_amd import scenes

W = dict(width=512, height=512)

GROWTH = [
    # coverage masks, rects: 64 prims / 128 mask words twice, then 129 prims (fit 130) and 384 words (do not fit 258)
    ("masks_rects", lambda: [scenes.cfg2_overlapping_rects(n=n, **W) for n in (64, 64, 129)]),
    # ... the same with brush-encoded rects (prim headers and GPU cache instead of quad headers), another seed in the last frame
    ("masks_rects_brush", lambda: [scenes.cfg2_overlapping_rects(n=n, seed=s, encoding="brush", **W)
                                   for n, s in ((64, 30), (64, 30), (129, 31))]),
    # ... masked rects (clip-mask atlas sampled per prim)
    ("masks_masked_rects", lambda: [scenes.masked_rects(n=n, seed=12, **W) for n in (64, 64, 129)]),
    # vertex tables: the image atlas is resident from the first frame on (same seed: same atlas); 80 prims / 9216 table rows twice,
    # then 103 prims (fit 162) and 22528 rows (do not fit 18434)
    ("vtab_images", lambda: [scenes.image_grid(n=n, seed=51, **W) for n in (16, 16, 40)]),
]

# the data textures (prim headers, GPU cache) grow and are uploaded whole by the last frame, whose setup stage reads them
UPLOAD_CARRY = ("data_textures_grow", lambda: [scenes.cfg2_overlapping_rects(n=60, seed=45, encoding="brush", **W),
                                               scenes.cfg2_overlapping_rects(n=60, seed=45, encoding="brush", **W),
                                               scenes.cfg2_overlapping_rects(n=110, seed=46, encoding="brush", **W)])

# the last frame brings a static texture the backend has not seen (the gradient frames' stops, the image atlas)
NEW_STATIC = ("new_static_texture", lambda: [scenes.cfg2_overlapping_rects(n=60, seed=47, **W),
                                             scenes.cfg2_overlapping_rects(n=60, seed=47, **W),
                                             scenes.image_grid(n=40, seed=53, **W)])

# the menu of tests/sweep_pipelined.py
MENU = [
    lambda: scenes.cfg2_overlapping_rects(n=60, seed=40, **W),
    lambda: scenes.masked_rects(n=40, **W),
    lambda: scenes.cfg2_overlapping_rects(n=70, seed=41, encoding="brush", fractional=True, **W),
    lambda: scenes.image_grid(n=40, **W),
    lambda: scenes.gradient_grid(n=20, **W),
    lambda: scenes.gradient_grid(n=20, seed=62, **W),
    lambda: scenes.gradient_grid(n=20, rotate=True, seed=66, **W),
    lambda: scenes.rotated_rects(n=30, opaque_frac=0.3, **W),
    lambda: scenes.add_slivers(scenes.image_grid(n=40, **W), pitch=3),
    lambda: scenes.gradient_grid(n=20, perspective=True, seed=67, **W),
    lambda: scenes.masked_rects(n=40, rotate=True, seed=13, **W),
    lambda: scenes.add_occluders(scenes.gradient_grid(n=20, seed=64, **W), n=20, zmax=40, seed=9),
    lambda: scenes.cfg5_many_rects(n=1500, **W),
    lambda: scenes.quad_masks(n=30, rotate=True, seed=86, **W),
    lambda: scenes.filter_grid(n=30, seed=71, **W),
]

# menu entries whose held-back raster launches offer no carrier: none of them has a variant of the fused setup kernel (pick_variant in
# wrhip.hip -- the general-quad, shading and filter feature sets), so the flush after one of them runs its setup stage on its own
NO_CARRIER = {6, 10, 13, 14}

# menu entries the device does not draw bit for bit like the oracle: filter_grid's FILTER_HUE_ROTATE takes its matrix from the device's
# cosf / sinf (<= 1 LSB, tests/test_gpu_parity.py::test_hip_filter_hue_rotate_are_a_bounded_deviation) -- on the device a streamed
# sequence ending in one of them is checked against the device's own render of that frame alone
DEVICE_INEXACT = {14}


def carriers_expected(seq):
    """Flushes of a streamed menu sequence that must have had their setup stage carried: every frame's but the first, unless the
    frame before it is one of NO_CARRIER."""
    return sum(1 for k in range(1, len(seq)) if seq[k - 1] not in NO_CARRIER)


def menu_ok():
    """The menu entries that can share one Renderer: static textures are kept by name, so two entries whose textures have one name
    and different pixels cannot both be in a sequence -- the later one is left out."""
    import hashlib
    seen, ok = {}, []
    for i, m in enumerate(MENU):
        good = True
        for ref in m().static_textures:
            h = hashlib.sha1(np.ascontiguousarray(ref.pixels).tobytes()).hexdigest() if ref.pixels is not None else None
            if seen.setdefault(ref.name, h) != h:
                good = False
        if good:
            ok.append(i)
    return ok


def random_sequences(seed, count, lo=4, hi=10):
    """`count` sequences of lo..hi menu indices (a fixed seed: the same sequences on every run)."""
    ok = menu_ok()
    rng = np.random.default_rng(seed)
    return [[int(rng.choice(ok)) for _ in range(int(rng.integers(lo, hi + 1)))] for _ in range(count)]


def check_streamed(lib, oracle, frames, carried=None):
    """Streams `frames` through `lib` and compares the window with the oracle's render of the last frame alone, byte for byte.
    At least `carried` flushes (default: all but the first two) must have had their setup stage carried by a held-back launch -- a
    change that drains the tail between frames would otherwise leave these tests passing on another path -- and no flush may find
    its planned carrier gone.  Returns the library's statistics."""
    from webrender_amd.harness import render_direct, render_streamed
    got, st = render_streamed(lib, frames)
    want, _ = render_direct(oracle, frames[-1])
    assert st["carrier_lost"] == 0, st
    assert st["setup_carried"] >= (len(frames) - 2 if carried is None else carried), st
    assert st["gl_error"] == 0, st
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes of the window differ; {st}"
    return st
