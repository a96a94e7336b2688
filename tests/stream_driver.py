"""Helper of tests/test_stream_parity.py (run as a subprocess: the staging ring's size, WRHIP_STAGING_BYTES, is read once per
process).  Records a frame's draws, then -- before those draws are flushed -- closes the open upload batch and laps the staging ring
with uploads to a texture the frame does not use, then Finishes; prints one JSON line: the window's sha256, GetError() and the
library's statistics.  usage: stream_driver.py <backend.so> <mode>

  readback  the batch is closed by a readback of another texture, then the ring is lapped twice
  wrap      the batch is closed by the ring wrapping under the uploads themselves
  realloc   one upload larger than the ring: the ring (and its device mirror) is reallocated
  pool      a gradient frame is flushed (WrhipFlush: its pool word is in the staging mirror), the ring is lapped with bytes that read as
            a plausible pool count, Finish; then the same frame once more, Finish -- the window is the second frame's"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from webrender_amd import glconst as G, scenes  # noqa: E402
from webrender_amd.glapi import GL  # noqa: E402
from webrender_amd.renderer import Renderer  # noqa: E402

W = dict(width=512, height=512)


def frame_for(mode):
    if mode == "pool":
        return scenes.gradient_grid(n=20, **W)
    return scenes.cfg2_overlapping_rects(n=200, seed=44, encoding="brush", **W)


def lap_ring(d, tex, side, laps):
    """Uploads to `tex` (side x side RGBA8, not sampled by the frame) of `laps` times the ring's size.  Every 8-byte word reads as
    0x04000000: more than a flush's pool holds, far less than a device could -- what a stale pool word would be taken for."""
    ring = int(os.environ["WRHIP_STAGING_BYTES"])
    word = np.array([0x04000000], dtype="<u8").view(np.uint8)
    data = np.ascontiguousarray(np.tile(word, side * side * 4 // 8))
    for _ in range(max(1, laps * ring // (side * side * 4))):
        d.upload_texture(tex, 0, 0, side, side, G.GL_RGBA, G.GL_UNSIGNED_BYTE, data)


def main(lib, mode):
    gl = GL(lib)
    frame = frame_for(mode)
    r = Renderer(gl, frame.width, frame.height)
    d = r.device
    side = 1024 if mode == "realloc" else 128
    junk = d.create_texture(side, side, G.GL_RGBA8, render_target=True)
    other = d.create_texture(16, 16, G.GL_RGBA8, render_target=True)
    d.upload_texture(other, 0, 0, 16, 16, G.GL_RGBA, G.GL_UNSIGNED_BYTE, np.full((16, 16, 4), 7, np.uint8))
    r.finish()
    gl.WrhipResetStats()
    r.render(frame)                           # recorded, not flushed: its draws read the data textures of the open batch
    if mode == "pool":
        gl.WrhipFlush()                       # ... flushed: the pool word of this flush sits in the staging mirror
        lap_ring(d, junk, side, 2)
        r.finish()
        r.render(frame)
    elif mode == "readback":
        d.read_texture(other)                 # closes the batch the draws' data textures are in
        lap_ring(d, junk, side, 2)
    elif mode == "wrap":
        lap_ring(d, junk, side, 2)
    elif mode == "realloc":
        lap_ring(d, junk, side, 1)            # (one upload of 4 MB: larger than the ring)
    else:
        raise SystemExit(f"unknown mode {mode}")
    r.finish()
    err = gl.GetError()
    px = r.read_pixels()
    st = gl.stats() if gl.is_wrhip else {}
    r.destroy()
    print(json.dumps({"digest": hashlib.sha256(np.ascontiguousarray(px).tobytes()).hexdigest(), "gl_error": int(err), "stats": st}))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
