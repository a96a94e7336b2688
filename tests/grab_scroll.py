"""Helpers of tests/test_grab_scroll.py: the scroll grab's contract (include/wrhip.h, WRHIP_GRAB_SCROLL) restated in numpy -- the
vote over the segments, the classification of the blocks, the payload's entries and the in-place decoder -- independently of the
library's kernels and of its codec (webrender_amd/csrc/wr_grab_codec.h).  Segment equality is exact here; the tests' content makes
every segment unique, or periodic on purpose, so the library's freedom to vote by hashes does not show.

Images are stored bytes as in tests/frame_grabs.py: (h, w, 4) B, G, R, A or (h, w) R8."""
import numpy as np
import frame_grabs as fg
import grab_packed as gp

BLOCK = fg.BLOCK
HEADER = fg.HEADER
COPY = 3
SCROLL_MAX = 512


def _segment_ids(prev, cur):
    """Per block column: (ids of cur's rows, ids of prev's rows) -- two segments of the column have one id exactly if their bytes
    are equal"""
    h, w = cur.shape[:2]
    out = []
    for x in range(0, w, BLOCK):
        both = np.concatenate([np.ascontiguousarray(cur[:, x:x + BLOCK]).reshape(h, -1), np.ascontiguousarray(prev[:, x:x + BLOCK]).reshape(h, -1)])
        inv = np.unique(both, axis=0, return_inverse=True)[1].reshape(-1)
        out.append((inv[:h], inv[h:]))
    return out


def votes(prev, cur):
    """{dy: votes} for 1 <= |dy| <= D: the segments (r, c) with 0 <= r + dy < h, cur(r, c) != prev(r, c), cur(r, c) == prev(r + dy, c)"""
    h = cur.shape[0]
    D = min(SCROLL_MAX, h - 1)
    ids = _segment_ids(prev, cur)
    out = {}
    for dy in range(-D, D + 1):
        if dy == 0:
            continue
        lo, hi = max(0, -dy), min(h, h - dy)
        n = sum(int(((c[lo:hi] != p[lo:hi]) & (c[lo:hi] == p[lo + dy:hi + dy])).sum()) for c, p in ids)
        if n:
            out[dy] = n
    return out


def scroll_dy(prev, cur):
    """The dy with the most votes; ties go to the smaller |dy|, then to the positive one; 0 without a vote"""
    v = votes(prev, cur)
    if not v:
        return 0
    return max(v, key=lambda dy: (v[dy], -abs(dy), dy > 0))


def classify(prev, cur):
    """-> (scroll_dy, {record: "same" | "copy" | "send"}) by exact comparison of the blocks"""
    h, w = cur.shape[:2]
    dy = scroll_dy(prev, cur)
    kinds = {}
    for rec in fg.blocks_of(w, h):
        x, y, bw, bh = rec
        blk = cur[y:y + bh, x:x + bw]
        if np.array_equal(blk, prev[y:y + bh, x:x + bw]):
            kinds[rec] = "same"
        elif dy != 0 and 0 <= y + dy and y + dy + bh <= h and np.array_equal(blk, prev[y + dy:y + dy + bh, x:x + bw]):
            kinds[rec] = "copy"
        else:
            kinds[rec] = "send"
    return dy, kinds


def encode_copy(rec):
    x, y, w, h = rec
    return np.array([x, y, w | h << 8 | COPY << 16, 0], "<u4").tobytes()


def expected_entries(prev, cur):
    """-> (scroll_dy, {record: the entry's bytes}) of a scroll grab of `cur` against the retained `prev`"""
    dy, kinds = classify(prev, cur)
    return dy, {rec: encode_copy(rec) if k == "copy" else gp.encode_block(cur, rec) for rec, k in kinds.items() if k != "same"}


def split(payload, bpp):
    """A scroll payload as it crossed (header first) -> (dy, {record: (mode, the entry's bytes)})"""
    assert len(payload) >= HEADER and int(np.frombuffer(payload, "<u4", 1)[0]) == len(payload) - HEADER, "the header's count is not the payload's size"
    dy = int(np.frombuffer(payload, "<i4", 1, 4)[0])
    assert bytes(payload[8:16]) == bytes(8)
    out, at = {}, HEADER
    while at < len(payload):
        assert at % 16 == 0 and at + 16 <= len(payload)
        x, y, whm, aux = (int(q) for q in np.frombuffer(payload, "<u4", 4, at))
        w, h, mode = whm & 255, (whm >> 8) & 255, whm >> 16
        assert mode in (gp.RAW, gp.SOLID, gp.RUNS, COPY) and 1 <= w <= BLOCK and 1 <= h <= BLOCK, (x, y, w, h, mode)
        assert mode != COPY or aux == 0
        size = 16 if mode in (gp.SOLID, COPY) else 16 + BLOCK * BLOCK * bpp if mode == gp.RAW else 16 + gp.align16(8 * h + aux * bpp)
        assert at + size <= len(payload) and (x, y, w, h) not in out
        out[(x, y, w, h)] = (mode, payload[at:at + size])
        at += size
    return dy, out


def decode(payload, img):
    """Patch a scroll payload (header first) into `img`, in place: the COPY entries first -- by ascending y for dy > 0, descending y
    for dy < 0, so that a block's source rows are still the old ones -- then every other entry; -> (entries, COPY entries)"""
    bpp = fg.bpp_of(img)
    dy, entries = split(payload, bpp)
    copies = sorted((rec for rec, (mode, _) in entries.items() if mode == COPY), key=lambda rec: rec[1], reverse=dy < 0)
    for (x, y, w, h) in copies:
        assert dy != 0 and 0 <= y + dy and y + dy + h <= img.shape[0]
        rows = range(h) if dy > 0 else range(h - 1, -1, -1)
        for r in rows:
            img[y + r, x:x + w] = img[y + r + dy, x:x + w]
    rest = {rec: me for rec, me in entries.items() if me[0] != COPY}
    if rest:
        body = b"".join(e for _, e in rest.values())
        head = np.array([len(body), 0, 0, 0], "<u4").tobytes()
        assert gp.decode(head + body, img) == len(rest)
    return len(entries), len(copies)


def page(rows, w, bpp, seed):
    """A tall page of random bytes: every segment of it is unique"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (rows, w, 4) if bpp == 4 else (rows, w), dtype=np.uint8)
