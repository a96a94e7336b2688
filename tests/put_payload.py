"""Helpers of tests/test_put_payload.py: payloads for a payload put (include/wrhip.h, WrhipPutTexturePayload) built in numpy -- plain
delta entries, packed entries (tests/grab_packed.py) and COPY entries (tests/grab_scroll.py) in any order --, frame sequences that
make a delta grab emit every kind of entry, and a session that puts a payload and checks what the put may cost.

Stored bytes are the grabs' (tests/frame_grabs.py): (h, w, 4) B, G, R, A or (h, w) R8.  Nothing here has a tolerance."""
import numpy as np
from webrender_amd import glapi, glconst as G
import frame_grabs as fg
import grab_packed as gp
import grab_scroll as gs

BLOCK, HEADER = fg.BLOCK, fg.HEADER
DELTA = glapi.GRAB_DELTA
PACKED = DELTA | glapi.GRAB_PACKED
SCROLL = PACKED | glapi.GRAB_SCROLL
MODES = {"delta": (DELTA,), "packed": (PACKED,), "scroll": (SCROLL,), "alternating": (DELTA, PACKED, SCROLL)}
DYS = (1, 7, 63, 64, 65, -1, -37, -64)
FMT = {4: G.GL_RGBA8, 1: G.GL_R8}


def shape(w, h, bpp):
    return (h, w, 4) if bpp == 4 else (h, w)


def noise(w, h, bpp, seed):
    return np.random.default_rng(seed).integers(0, 256, shape(w, h, bpp), dtype=np.uint8)


def payload_of(entries, dy=0):
    """header (word 0: the bytes of the entries, word 1: dy) + entries"""
    body = b"".join(entries)
    return np.array([len(body), dy & 0xFFFFFFFF, 0, 0], "<u4").tobytes() + body


def encode_plain(img, rec):
    """The entry of a plain delta grab: the record x, y, w, h and the block at the fixed pitch, zeros beyond the cut block"""
    x, y, w, h = rec
    bpp = fg.bpp_of(img)
    body = np.zeros((BLOCK, BLOCK * bpp), np.uint8)
    body[:h, :w * bpp] = np.ascontiguousarray(img[y:y + h, x:x + w]).reshape(h, w * bpp)
    return np.array([x, y, w, h], "<u4").tobytes() + body.tobytes()


def entries_of(payload, flags, bpp):
    """-> (entries, COPY entries) of a payload, walked here (a block may be named by a COPY and by another entry)"""
    if not flags & glapi.GRAB_PACKED:
        assert (len(payload) - HEADER) % fg.entry_bytes(bpp) == 0
        return (len(payload) - HEADER) // fg.entry_bytes(bpp), 0
    n = copies = 0
    at = HEADER
    while at < len(payload):
        whm, aux = (int(q) for q in np.frombuffer(payload, "<u4", 2, at + 8))
        h, mode = (whm >> 8) & 255, whm >> 16
        at += 16 if mode in (gp.SOLID, gs.COPY) else 16 + BLOCK * BLOCK * bpp if mode == gp.RAW else 16 + gp.align16(8 * h + aux * bpp)
        n += 1
        copies += mode == gs.COPY
    assert at == len(payload)
    return n, copies


def scrolled(prev, dy, rng):
    """`prev` scrolled by dy -- row r shows what row r + dy showed -- with the exposed strip new"""
    h = prev.shape[0]
    assert 0 < abs(dy) < h
    cur = rng.integers(0, 256, prev.shape, dtype=np.uint8)
    if dy > 0:
        cur[:h - dy] = prev[dy:]
    else:
        cur[-dy:] = prev[:h + dy]
    return cur


def change_blocks(img, rng, n):
    """n of the image's blocks changed: to one value, to rows of runs, to noise, in turn"""
    h, w = img.shape[:2]
    bpp = fg.bpp_of(img)
    ch = (4,) if bpp == 4 else ()
    recs = fg.blocks_of(w, h)
    out = img.copy()
    for k, i in enumerate(rng.choice(len(recs), min(n, len(recs)), replace=False)):
        x, y, bw, bh = recs[int(i)]
        if k % 3 == 0:
            blk = np.broadcast_to(rng.integers(0, 256, ch, dtype=np.uint8), (bh, bw) + ch)
        elif k % 3 == 1:
            run = rng.integers(0, 256, ((bw + 6) // 7,) + ch, dtype=np.uint8)
            blk = np.broadcast_to(np.repeat(run, 7, axis=0)[:bw].reshape((1, bw) + ch), (bh, bw) + ch)
        else:
            blk = rng.integers(0, 256, (bh, bw) + ch, dtype=np.uint8)
        out[y:y + bh, x:x + bw] = blk
    return out


def sequence(w, h, bpp, case):
    """Six frames of a w x h rect: flat, run-structured and noise blocks; a few changed blocks; the frame before scrolled by three
    of DYS (which three: `case`), with the exposed strip new and, once, a changed block on top.  A rect too short for a vector gets
    changed blocks instead."""
    rng = np.random.default_rng([w, h, bpp, case])
    dys = [DYS[(3 * case + k) % len(DYS)] for k in range(3)]
    frames = [gp.mixed_content(h, w, bpp, 100 + case)]

    def scroll(dy):
        return scrolled(frames[-1], dy, rng) if abs(dy) < h else change_blocks(frames[-1], rng, 2)
    frames.append(change_blocks(frames[-1], rng, 3))
    frames.append(scroll(dys[0]))
    frames.append(change_blocks(scroll(dys[1]), rng, 1))
    frames.append(change_blocks(frames[-1], rng, 4))
    frames.append(scroll(dys[2]))
    return frames


class Session(fg.Session):
    """fg.Session with a small window, textures of both formats, and puts whose cost is checked"""

    def __init__(self, lib):
        fg.Session.__init__(self, lib, 64, 64)

    def make_px(self, px):
        t = self.make(px, FMT[fg.bpp_of(px)])
        return t

    def read(self, t):
        return self.d.read_texture(t).copy()

    def put(self, t, rect, payload, flags, quiet=True, what=""):
        """The put under test, and its cost (include/wrhip.h): 0, 1 or 2 launches by the entries the payload has, nothing read back,
        at most the payload and 16 bytes per entry staged; quiet: nothing pending touches the texture, so nothing else is launched
        and no recorded work is flushed"""
        n, copies = entries_of(payload, flags, 1 if t.format == G.GL_R8 else 4)
        a = self.stats()
        rc = self.gl.put_texture_payload(t.id, rect, payload, flags)
        b = self.stats()
        assert rc == 0, (what, rc, self.gl.GetError())
        launches = (1 if copies else 0) + (1 if n > copies else 0)
        assert b["d2h_bytes"] == a["d2h_bytes"], (what, a, b)
        if n == 0:
            assert b["h2d_bytes"] == a["h2d_bytes"] and b["kernel_launches"] == a["kernel_launches"], (what, a, b)
        else:
            assert len(payload) <= b["h2d_bytes"] - a["h2d_bytes"] <= len(payload) + 16 * n, (what, len(payload), n, a, b)
        if quiet:
            assert b["kernel_launches"] == a["kernel_launches"] + launches and b["flushes"] == a["flushes"], (what, launches, a, b)
        else:
            assert b["kernel_launches"] >= a["kernel_launches"] + launches, (what, launches, a, b)
        return launches


def decoded(gl, payload, flags, before):
    """What WrhipGrabDecode leaves in an image of the rect that held `before`"""
    img = np.ascontiguousarray(before).copy()
    gl.grab_decode(payload, FMT[fg.bpp_of(img)], flags, img)
    return img


def differing(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a != b).sum())
