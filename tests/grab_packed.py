"""Helpers of tests/test_grab_packed.py: the packed payload of a delta grab (include/wrhip.h, "THE PACKED PAYLOAD") restated in
numpy -- the encoding of one block, the entry-size rule, a payload decoder -- independently of the library's own decoder
(webrender_amd/csrc/wr_grab_codec.h), and blocks constructed to have given run starts.

Images are stored bytes as in tests/frame_grabs.py: (h, w, 4) B, G, R, A or (h, w) R8."""
import numpy as np
import frame_grabs as fg

BLOCK = fg.BLOCK
HEADER = fg.HEADER
RAW, SOLID, RUNS = 0, 1, 2


def align16(n):
    return (n + 15) & ~15


def values_of(blk):
    """The values of a block's pixels in row-major order: the 4 stored bytes as a little-endian word, or the byte"""
    blk = np.ascontiguousarray(blk)
    if blk.ndim == 3:
        return blk.reshape(-1, 4).view("<u4").reshape(-1)
    return blk.reshape(-1)


def run_starts(blk):
    """-> (values, starts): pixel i starts a run if i == 0 or its value differs from pixel i - 1's"""
    v = values_of(blk)
    start = np.ones(v.size, bool)
    start[1:] = v[1:] != v[:-1]
    return v, start


def entry_size(h, n, bpp):
    """(mode, bytes) of the entry of a cut block of h rows with n run starts; a tie between RUNS and RAW goes to RAW"""
    raw = 16 + BLOCK * BLOCK * bpp
    runs = 16 + align16(8 * h + n * bpp)
    if n == 1:
        return SOLID, 16
    if runs < raw:
        return RUNS, runs
    return RAW, raw


def encode_block(img, rec):
    """The entry of block `rec` = (x, y, w, h) of `img`, byte for byte"""
    x, y, w, h = rec
    bpp = fg.bpp_of(img)
    blk = np.ascontiguousarray(img[y:y + h, x:x + w])
    v, start = run_starts(blk)
    n = int(start.sum())
    mode, size = entry_size(h, n, bpp)
    aux = int(v[0]) if mode == SOLID else n if mode == RUNS else 0
    out = np.array([x, y, w | h << 8 | mode << 16, aux], "<u4").tobytes()
    if mode == RAW:
        body = np.zeros((BLOCK, BLOCK * bpp), np.uint8)
        body[:h, :w * bpp] = blk.reshape(h, w * bpp)
        out += body.tobytes()
    elif mode == RUNS:
        bits = np.zeros((h, 64), np.uint8)
        bits[:, :w] = start.reshape(h, w)
        body = np.packbits(bits, axis=1, bitorder="little").tobytes() + v[start].astype("<u4" if bpp == 4 else np.uint8).tobytes()
        out += body + bytes(align16(len(body)) - len(body))
    assert len(out) == size and size % 16 == 0
    return out


def predicted_bytes(img, records):
    """What crosses for a packed grab that sends `records` of `img`: the header and the entries"""
    return HEADER + sum(len(encode_block(img, r)) for r in records)


def split(payload, bpp):
    """A packed payload as it crossed (header first) -> {record (x, y, w, h): (mode, the entry's bytes)}"""
    assert len(payload) >= HEADER and int(np.frombuffer(payload, "<u4", 1)[0]) == len(payload) - HEADER, "the header's count is not the payload's size"
    out, at = {}, HEADER
    while at < len(payload):
        assert at % 16 == 0 and at + 16 <= len(payload)
        x, y, whm, aux = (int(q) for q in np.frombuffer(payload, "<u4", 4, at))
        w, h, mode = whm & 255, (whm >> 8) & 255, whm >> 16
        assert mode in (RAW, SOLID, RUNS) and 1 <= w <= BLOCK and 1 <= h <= BLOCK, (x, y, w, h, mode)
        size = 16 if mode == SOLID else 16 + BLOCK * BLOCK * bpp if mode == RAW else 16 + align16(8 * h + aux * bpp)
        assert at + size <= len(payload) and (x, y, w, h) not in out
        out[(x, y, w, h)] = (mode, payload[at:at + size])
        at += size
    return out


def decode(payload, img):
    """Patch a packed payload (header first) into `img`; -> the number of entries"""
    bpp = fg.bpp_of(img)
    shape = lambda w, h: (h, w, 4) if bpp == 4 else (h, w)
    entries = split(payload, bpp)
    for (x, y, w, h), (mode, e) in entries.items():
        aux = int(np.frombuffer(e, "<u4", 1, 12)[0])
        if mode == SOLID:
            img[y:y + h, x:x + w] = np.array([aux], "<u4").view(np.uint8) if bpp == 4 else aux
        elif mode == RAW:
            body = np.frombuffer(e, np.uint8, BLOCK * BLOCK * bpp, 16).reshape(BLOCK, BLOCK * bpp)
            img[y:y + h, x:x + w] = body[:h, :w * bpp].reshape(shape(w, h))
        else:
            bm = np.frombuffer(e, np.uint8, 8 * h, 16).reshape(h, 8)
            start = np.unpackbits(bm, axis=1, bitorder="little")[:, :w].reshape(-1).astype(bool)
            assert start[0] and int(start.sum()) == aux
            lit = np.frombuffer(e, np.uint8, aux * bpp, 16 + 8 * h).reshape(aux, bpp)
            img[y:y + h, x:x + w] = lit[np.cumsum(start) - 1].reshape(shape(w, h))
    return len(entries)


def block_with_starts(w, h, starts, bpp, seed=0):
    """A w x h block whose run starts are exactly the pixel indices `starts` (0 among them): run k has a value that differs from
    run k - 1's"""
    starts = sorted(set(int(s) for s in starts))
    assert starts[0] == 0 and starts[-1] < w * h
    mark = np.zeros(w * h, bool)
    mark[starts] = True
    k = np.cumsum(mark) - 1
    if bpp == 4:
        v = ((k + 1 + seed).astype(np.uint64) * 2654435761 % (1 << 32)).astype("<u4")      # (odd multiplier: k -> value is one to one)
        blk = v.view(np.uint8).reshape(h, w, 4)
    else:
        blk = ((k + seed) % 251).astype(np.uint8).reshape(h, w)
    assert np.array_equal(np.flatnonzero(run_starts(blk)[1]), starts)
    return np.ascontiguousarray(blk)


def block_with_n_starts(n, bpp, seed):
    """A full 64 x 64 block with exactly n run starts at random places"""
    rng = np.random.default_rng(seed)
    rest = rng.choice(BLOCK * BLOCK - 1, n - 1, replace=False) + 1 if n > 1 else []
    return block_with_starts(BLOCK, BLOCK, [0] + list(rest), bpp, seed)


def mixed_content(h, w, bpp, seed):
    """An image whose blocks are, in turn: flat, a few rects, noise, a horizontal 1-px gradient, a vertical gradient"""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w, 4) if bpp == 4 else (h, w), np.uint8)
    ch = (4,) if bpp == 4 else ()
    for i, (x, y, bw, bh) in enumerate(fg.blocks_of(w, h)):
        kind = i % 5
        if kind == 0:
            blk = np.broadcast_to(rng.integers(0, 256, ch, dtype=np.uint8), (bh, bw) + ch)
        elif kind == 1:
            blk = np.empty((bh, bw) + ch, np.uint8)
            blk[...] = rng.integers(0, 256, ch, dtype=np.uint8)
            for _ in range(4):
                x0, y0 = int(rng.integers(0, bw)), int(rng.integers(0, bh))
                blk[y0:y0 + int(rng.integers(1, 40)), x0:x0 + int(rng.integers(1, 40))] = rng.integers(0, 256, ch, dtype=np.uint8)
        elif kind == 2:
            blk = rng.integers(0, 256, (bh, bw) + ch, dtype=np.uint8)
        elif kind == 3:
            ramp = (np.arange(bw) * 3 + i).astype(np.uint8)
            blk = np.broadcast_to(ramp.reshape((1, bw) + (1,) * len(ch)), (bh, bw) + ch)
        else:
            ramp = (np.arange(bh) * 3 + i).astype(np.uint8)
            blk = np.broadcast_to(ramp.reshape((bh, 1) + (1,) * len(ch)), (bh, bw) + ch)
        img[y:y + bh, x:x + bw] = blk
    return img
