"""Frame harness: records the C-ABI call stream of rendering a scene and
replays it natively -- the stand-in for `wrench png` / `wrench perf`
(wrench/src/main.rs:517-814, perf.rs:198-270).

  setup trace  CreateContext .. first frame .. Finish   (resource creation, untimed)
  frame trace  one steady-state frame .. Finish         (what `perf` times: the
               full tile-raster + composite stream is re-issued every iteration,
               see BASELINE.md §1 on why wrench's own loop would only re-composite)
  read trace   ReadPixels of the window (reftest.rs:306-319)
"""
import numpy as np
from . import glconst as G
from .glapi import GL
from .renderer import Renderer
from .trace import Trace, NativeReplayer, TAG_SCRATCH


class RecordedScene:
    def __init__(self, width, height, setup, frame, read, read_offset, stream=None):
        self.width, self.height = width, height
        self.setup, self.frame, self.read, self.read_offset = setup, frame, read, read_offset
        self.stream = stream or frame
        self.texture_ids = {}     # TextureRef.name -> backend texture id (deterministic across replays)
        self.tile_rects = {}      # TextureRef.name -> composite rect (x0,y0,x1,y1) in device px


def record_scene(recording_backend_path, frame):
    """Run `frame` twice through the Python Renderer mirror against
    `recording_backend_path`, capturing the call stream."""
    tr = Trace()
    gl = GL(recording_backend_path, tr)
    r = Renderer(gl, frame.width, frame.height)
    r.render(frame)
    r.finish()
    setup = tr.serialize()
    tr2 = Trace()
    tr2.scratch = 0
    gl.trace = tr2
    r.render(frame)
    stream_bytes = tr2.serialize()      # the frame without a trailing Finish (throughput loops)
    r.finish()
    frame_bytes = tr2.serialize()
    tr3 = Trace()
    gl.trace = tr3
    px = r.read_pixels()
    read_bytes = tr3.serialize()
    read_off = [v for (_, args) in tr3.calls for (tag, _, v) in args if tag == TAG_SCRATCH][-1]
    gl.trace = None
    rec = RecordedScene(frame.width, frame.height, setup, frame_bytes, read_bytes, read_off, stream_bytes)
    rec.texture_ids = {name: t.id for name, t in r.textures.items()}
    rec.tile_rects = {t.texture.name: t.rect for t in frame.composite_tiles}
    r.destroy()
    return rec, px


class ScenePlayer:
    """Replays a RecordedScene against a backend library natively."""

    def __init__(self, backend_path, scene):
        self.scene = scene
        self.rp = NativeReplayer(backend_path)
        self.rp.exec(scene.setup)

    def frames(self, warmup, iters):
        return self.rp.loop(self.scene.frame, warmup, iters)

    def stream(self, iters):
        """`iters` frames back to back, one Finish at the end; total wall ms."""
        return self.rp.stream(self.scene.stream, iters)

    def read_pixels(self):
        self.rp.exec(self.scene.read)
        n = self.scene.width * self.scene.height * 4
        buf = self.rp.scratch(self.scene.read_offset, n)
        return np.frombuffer(buf, dtype=np.uint8).reshape(self.scene.height, self.scene.width, 4).copy()

    def symbol(self, name):
        return self.rp.symbol(name)


def render_direct(backend_path, frame, frames=1):
    """Render through the Python mirror without tracing; returns RGBA8 window
    pixels, or {texture name: pixels, "window": ...} when the frame asks for
    render-target readbacks (Frame.readback)."""
    gl = GL(backend_path)
    r = Renderer(gl, frame.width, frame.height)
    for _ in range(frames):
        r.render(frame)
    r.finish()
    err = gl.GetError()            # (libwrhip: GL_INVALID_OPERATION when a prim was on a path it cannot draw exactly)
    px = r.read_pixels()
    extra = {ref.name: r.device.read_texture(r.resolve(ref)) for ref in getattr(frame, "readback", [])}
    stats = gl.stats() if gl.is_wrhip else None
    if stats is not None:
        stats["gl_error"] = int(err)
    r.destroy()
    if extra:
        extra["window"] = px
        return extra, stats
    return px, stats


def render_pipelined(backend_path, frames):
    """Issue `frames` (same window size) back to back WITHOUT a Finish in between; after each
    frame the window is blitted (device-side, asynchronous) into a keeper texture.  One Finish at
    the end, then the keepers are read back: [BGRA8 pixels per frame].  Exercises the backend's
    cross-frame pipelining (uploads of frame k+1 against the raster work of frame k)."""
    gl = GL(backend_path)
    w, h = frames[0].width, frames[0].height
    r = Renderer(gl, w, h)
    d = r.device
    keepers = [d.create_texture(w, h, G.GL_RGBA8, render_target=True) for _ in frames]
    for f, k in zip(frames, keepers):
        r.render(f)
        gl.BindFramebuffer(G.GL_READ_FRAMEBUFFER, 0)
        gl.BindFramebuffer(G.GL_DRAW_FRAMEBUFFER, k.fbo)
        gl.BlitFramebuffer(0, 0, w, h, 0, 0, w, h, G.GL_COLOR_BUFFER_BIT, G.GL_NEAREST)
        gl.BindFramebuffer(G.GL_DRAW_FRAMEBUFFER, 0)
    r.finish()
    out = [d.read_texture(k) for k in keepers]
    r.destroy()
    return out


def render_streamed(backend_path, frames):
    """Render `frames` (same window size) back to back through one Renderer with nothing between them that drains the
    backend's held-back raster launches -- no Finish, readback, blit or query -- then one Finish: the window (RGBA8, as
    render_direct returns it), which shows the LAST frame, and the backend's statistics (libwrhip; None otherwise).
    This is the path a frame loop takes: every flush's setup stage and upload scatter ride in the first workgroups of a
    raster launch the flush before held back (WrhipStats::setup_carried)."""
    gl = GL(backend_path)
    w, h = frames[0].width, frames[0].height
    r = Renderer(gl, w, h)
    for f in frames:
        assert (f.width, f.height) == (w, h), "render_streamed: one window size"
        r.render(f)
    r.finish()
    err = gl.GetError()
    px = r.read_pixels()
    stats = gl.stats() if gl.is_wrhip else None
    if stats is not None:
        stats["gl_error"] = int(err)
    r.destroy()
    return px, stats


def render_streamed_tapped(backend_path, frames):
    """render_streamed with every frame looked at: after each frame's render the window is tapped (GL.tap_texture: a digest taken
    on the device, in stream order behind that frame) -- still nothing between the frames that drains the held-back raster launches,
    no Finish, no readback.  The results are fetched after the one Finish at the end.  Returns the final window (RGBA8), the
    backend's statistics and the list of per-frame tap results (GL.tap_result dicts, frame 0 first).  libwrhip only."""
    gl = GL(backend_path)
    assert gl.is_wrhip, "render_streamed_tapped: taps are a libwrhip addition"
    w, h = frames[0].width, frames[0].height
    r = Renderer(gl, w, h)
    window = gl.WrhipGetFramebufferTexture(0)
    tickets = []
    for f in frames:
        assert (f.width, f.height) == (w, h), "render_streamed_tapped: one window size"
        r.render(f)
        tickets.append(gl.tap_texture(window))
    r.finish()
    err = gl.GetError()
    assert all(t >= 0 for t in tickets), tickets
    taps = [gl.tap_result(t) for t in tickets]
    px = r.read_pixels()
    stats = gl.stats()
    stats["gl_error"] = int(err)
    r.destroy()
    return px, stats, taps


def screenshot_size(window_size, buffer_size):
    """The size the reference's screenshot grabber scales a window of `window_size` = (w, h) to so that it fits a buffer of
    `buffer_size` (screen_capture.rs:121-124): scale = min(bw / w, bh / h), each dimension times it, rounded half away from
    zero -- all in float32, as the Rust expression evaluates it."""
    f = np.float32
    w, h = f(window_size[0]), f(window_size[1])
    scale = min(f(buffer_size[0]) / w, f(buffer_size[1]) / h)

    def rnd(v):
        # (f32::round on a value >= 0: the fraction v - trunc(v) is exact, which v + 0.5 need not be)
        t = np.trunc(v)
        return int(t) + (1 if v - t >= f(0.5) else 0)
    return rnd(w * scale), rnd(h * scale)


def render_streamed_grabbed(backend_path, frames, delta=False, rect=None, packed=False, scale_to=None, scroll=False):
    """render_streamed_tapped with the pixels: after each frame's render `rect` of the window (None: all of it) is grabbed
    (GL.grab_texture: packed on the device in stream order behind that frame, carried to the host on the library's second
    stream) -- still nothing between the frames that drains the held-back raster launches.  Results are fetched in order as they
    arrive, and the oldest is waited for (that ticket alone) only when the ring of 8 would otherwise lose it, so any number of
    frames goes through.  delta=True: delta grabs, patched one after the other into one host image; packed=True (with delta):
    their blocks cross in the packed form (glapi.GRAB_PACKED); scroll=True (with delta and packed): scroll grabs (glapi.GRAB_SCROLL).
    scale_to=(w, h) (without delta): every grab is the scaled one
    (GL.grab_texture_scaled) and every image the (h, w, 4) result.
    Returns the final window (RGBA8), the backend's statistics, the host's image of the rect after every frame's grab (stored
    bytes, B, G, R, A) and the grabs' info dicts.  libwrhip only."""
    from . import glapi
    gl = GL(backend_path)
    assert gl.is_wrhip, "render_streamed_grabbed: grabs are a libwrhip addition"
    w, h = frames[0].width, frames[0].height
    r = Renderer(gl, w, h)
    window = gl.WrhipGetFramebufferTexture(0)
    rect = (0, 0, w, h) if rect is None else tuple(rect)
    host = np.zeros((rect[3], rect[2], 4), np.uint8)
    waiting, images, infos = [], [], []

    def fetch(wait):
        while waiting:
            res = gl.grab_result(waiting[0], wait=wait, into=host if delta else None)
            if res is None:
                return
            waiting.pop(0)
            infos.append(res[0])
            images.append(host.copy() if delta else res[1])
            wait = False
    for f in frames:
        assert (f.width, f.height) == (w, h), "render_streamed_grabbed: one window size"
        r.render(f)
        if len(waiting) == 8:
            fetch(True)
        if scale_to is not None:
            assert not delta, "render_streamed_grabbed: a scaled grab is a full one"
            t = gl.grab_texture_scaled(window, rect, scale_to)
        else:
            assert not scroll or (delta and packed), "render_streamed_grabbed: a scroll grab is a packed delta one"
            t = gl.grab_texture(window, rect, (glapi.GRAB_DELTA if delta else 0) | (glapi.GRAB_PACKED if packed else 0) | (glapi.GRAB_SCROLL if scroll else 0))
        assert t >= 0, (t, gl.GetError())
        waiting.append(t)
        fetch(False)
    r.finish()
    err = gl.GetError()
    while waiting:
        fetch(True)
    px = r.read_pixels()
    stats = gl.stats()
    stats["gl_error"] = int(err)
    r.destroy()
    return px, stats, images, infos


def render_streamed_tensors(backend_path, frames, size, dtype, layout, channels, scale, bias):
    """render_streamed with every frame kept ON THE DEVICE as a tensor: one [N, ...] batch is allocated there (GL.device_alloc) and,
    after frame k's render, the window is tensor-grabbed (GL.grab_texture_tensor: scaled to `size` = (w, h) as grab_texture_scaled
    scales, converted to `dtype` elements in `layout` with `channels` channels, times `scale` plus `bias`) into slot k -- nothing
    between the frames drains the held-back raster launches, no Finish, and nothing but 16 bytes per frame crosses to the host.
    Only the LAST ticket is waited for: the grabs run on one stream, in order, so every slot is written by then.  Tickets that
    happen to have arrived are fetched on the way; one the ring of 8 overwrote first leaves None in the infos -- its slot is
    written all the same.  Returns the batch read back ([N, C, h, w] or [N, h, w, C]; uint8, float16, float32, or the uint16
    patterns of bfloat16), the backend's statistics and the grabs' info dicts.  libwrhip only."""
    from . import glapi
    gl = GL(backend_path)
    assert gl.is_wrhip, "render_streamed_tensors: grabs are a libwrhip addition"
    w, h = frames[0].width, frames[0].height
    r = Renderer(gl, w, h)
    window = gl.WrhipGetFramebufferTexture(0)
    elem = glapi.TENSOR_ELEM_BYTES[dtype]
    shape = (channels, size[1], size[0]) if layout == glapi.TENSOR_CHW else (size[1], size[0], channels)
    slot = size[0] * size[1] * channels * elem
    slot16 = (slot + 15) & ~15                      # slots start on 16 bytes: every grab takes the wide stores
    batch = gl.device_alloc(slot16 * len(frames))
    assert batch, gl.GetError()
    tickets, infos = [], [None] * len(frames)

    def fetch(k, wait):
        try:
            res = gl.grab_result(tickets[k], wait=wait)
        except KeyError:
            return True                             # overwritten in the ring: nothing to learn any more
        if res is not None:
            infos[k] = res[0]
        return res is not None
    oldest = 0
    for k, f in enumerate(frames):
        assert (f.width, f.height) == (w, h), "render_streamed_tensors: one window size"
        r.render(f)
        t = gl.grab_texture_tensor(window, (0, 0, w, h), batch + k * slot16, slot, size=size, dtype=dtype, layout=layout,
                                   channels=channels, scale=scale, bias=bias)
        assert t >= 0, (t, gl.GetError())
        tickets.append(t)
        while oldest < k and fetch(oldest, False):
            oldest += 1
    fetch(len(frames) - 1, True)
    for k in range(oldest, len(frames) - 1):
        fetch(k, False)
    err = gl.GetError()
    raw = gl.device_read(batch, slot16 * len(frames)).reshape(len(frames), slot16)[:, :slot]
    np_dtype = {glapi.TENSOR_U8: np.uint8, glapi.TENSOR_F16: np.float16, glapi.TENSOR_BF16: np.uint16, glapi.TENSOR_F32: np.float32}[dtype]
    out = np.ascontiguousarray(raw).view(np_dtype).reshape((len(frames),) + shape)
    stats = gl.stats()
    stats["gl_error"] = int(err)
    gl.device_free(batch)
    r.finish()
    r.destroy()
    return out, stats, infos


def render_streamed_yuv(backend_path, frames, format, color_space, device=False, flags=0, delta=False, key_every=None, scale_to=None, renditions=1, scroll=False):
    """render_streamed_grabbed for a video encoder: after each frame's render the whole window is YUV-grabbed (GL.grab_texture_yuv:
    one launch in stream order behind that frame, 8-bit planes in `format` of the ranged colour space `color_space`) -- nothing
    between the frames drains the held-back raster launches, no Finish.  Frame k's ticket is fetched after frame k + 1 has been
    rendered and grabbed, so the host never waits for the frame it has just submitted; the last one is waited for at the end.
    device=False: the planes cross to the host as the tickets' payloads.  device=True: each frame's planes go, tight, into a buffer
    of its own in device memory (GL.device_alloc) -- where an encoder on the card would take them -- 16 bytes per frame cross, and
    the buffers are read back at the end.  Returns the per-frame planes (glapi.yuv_split's lists), the backend's statistics
    (`setup_carried` included) and the grabs' info dicts.  libwrhip only.
    delta=True: a delta YUV grab per frame (GL.grab_texture_yuv_delta) into ONE set of planes that lives across the frames -- a flat
    host array the tickets' blocks are patched into, or one device buffer the blocks are written to -- so only the 64 x 64 blocks
    whose samples changed cross or are written; the planes returned for frame k are a copy of the accumulated ones once frame k's
    ticket has been fetched (device: read back then, while frame k + 1's grab is still parked).  key_every=N: every N-th grab passes GRAB_KEY.
    scroll=True (with delta): every grab passes GRAB_SCROLL -- scrolled blocks cross as COPY entries, or are written from the retained planes.
    scale_to=(w, h) (without delta): every grab is the scaled one (GL.grab_texture_yuv_scaled) with `renditions` renditions -- levels
    0 .. renditions - 1 of the chain to scale_to -- and a frame's planes are glapi.yuv_split_renditions' list of them."""
    from . import glapi
    gl = GL(backend_path)
    assert gl.is_wrhip, "render_streamed_yuv: grabs are a libwrhip addition"
    w, h = frames[0].width, frames[0].height
    r = Renderer(gl, w, h)
    window = gl.WrhipGetFramebufferTexture(0)
    nbytes = sum(rows * row for rows, row in glapi.yuv_plane_shapes(w, h, format))
    if delta:
        assert scale_to is None, "render_streamed_yuv: a scaled YUV grab is a full one"
        return _render_streamed_yuv_delta(gl, r, window, frames, format, color_space, device, flags, key_every, nbytes, scroll)
    assert not scroll, "render_streamed_yuv: a scroll YUV grab is a delta one"
    # (scaled: rendition k is scale_to << k; a frame's renditions lie one after another, on the host and in the frame's device buffer)
    sizes = [(scale_to[0] << k, scale_to[1] << k) for k in range(renditions)] if scale_to is not None else []
    each = [sum(rows * row for rows, row in glapi.yuv_plane_shapes(sw, sh, format)) for sw, sh in sizes]
    if scale_to is not None:
        nbytes = sum(each)
    bufs = [gl.device_alloc(nbytes) for _ in frames] if device else []
    assert all(bufs), gl.GetError()
    tickets, flats, infos = [], [], []

    def fetch(k):
        info, flat = gl.grab_result(tickets[k])
        infos.append(info)
        flats.append(flat)
    for k, f in enumerate(frames):
        assert (f.width, f.height) == (w, h), "render_streamed_yuv: one window size"
        r.render(f)
        if scale_to is not None:
            dsts = [(bufs[k] + sum(each[:i]), each[i]) for i in range(renditions)] if device else None
            t = gl.grab_texture_yuv_scaled(window, (0, 0, w, h), scale_to, format, color_space, flags, renditions=renditions, dsts=dsts)
        else:
            t = gl.grab_texture_yuv(window, (0, 0, w, h), format, color_space, flags, dst=bufs[k] if device else None,
                                    dst_bytes=nbytes if device else 0)
        assert t >= 0, (t, gl.GetError())
        tickets.append(t)
        if k >= 1:
            fetch(k - 1)
    fetch(len(frames) - 1)
    err = gl.GetError()
    stats = gl.stats()
    stats["gl_error"] = int(err)
    if device:
        flats = [gl.device_read(b, nbytes) for b in bufs]
        for b in bufs:
            gl.device_free(b)
    r.finish()
    r.destroy()
    if scale_to is not None:
        return [glapi.yuv_split_renditions(fl, scale_to, renditions, format) for fl in flats], stats, infos
    return [glapi.yuv_split(fl, w, h, format) for fl in flats], stats, infos


def _render_streamed_yuv_delta(gl, r, window, frames, format, color_space, device, flags, key_every, nbytes, scroll=False):
    """render_streamed_yuv(delta=True): frame k - 1's ticket is fetched after frame k has been rendered and grabbed, as in the full
    loop.  Frame k's grab is then parked behind frame k's held-back launches, so the accumulated planes -- the host's, or the device
    buffer read back on the draw stream -- are frame k - 1's when they are copied"""
    from . import glapi
    w, h = frames[0].width, frames[0].height
    host = np.zeros(nbytes, np.uint8)
    acc = gl.device_alloc(nbytes) if device else 0
    assert acc or not device, gl.GetError()
    tickets, flats, infos = [], [], []

    def fetch(k):
        infos.append(gl.grab_result(tickets[k], into=None if device else host)[0])
        flats.append(gl.device_read(acc, nbytes) if device else host.copy())
    for k, f in enumerate(frames):
        assert (f.width, f.height) == (w, h), "render_streamed_yuv: one window size"
        r.render(f)
        t = gl.grab_texture_yuv_delta(window, (0, 0, w, h), format, color_space, flags, dst=acc if device else None,
                                      dst_bytes=nbytes if device else 0, key=bool(key_every) and k % key_every == 0, scroll=scroll)
        assert t >= 0, (t, gl.GetError())
        tickets.append(t)
        if k >= 1:
            fetch(k - 1)
    fetch(len(frames) - 1)
    err = gl.GetError()
    stats = gl.stats()
    stats["gl_error"] = int(err)
    if device:
        gl.device_free(acc)
    r.finish()
    r.destroy()
    return [glapi.yuv_split(fl, w, h, format) for fl in flats], stats, infos


def render_streamed_mirrored(backend_path, frames, packed=True, scroll=False, check=True):
    """A mirror on the device: after each frame's render the window is delta-grabbed (GL.grab_texture with GRAB_DELTA, GRAB_PACKED if
    `packed`, GRAB_SCROLL if `scroll` -- a scroll grab is a packed one), the payload is fetched as it crossed (GL.grab_payload: that
    ticket alone is waited for) and forwarded into a second, window-sized RGBA8 texture of the same context with a payload put
    (GL.put_texture_payload) -- what a viewer at the other end of a link does.  No Finish, no ReadPixels and no TexSubImage2D of the
    mirror anywhere in the loop: the mirror's pixels reach it only as payloads.  check: after every put the window and the mirror
    are both grabbed whole (plain grabs, in stream order behind the put), fetched one frame later.
    Returns the mirror's stored bytes after the last frame (B, G, R, A; read after one Finish), the backend's statistics at the end
    of the loop, the windows and the mirrors after every frame (empty without check) and the bytes of every payload.  libwrhip only."""
    from . import glapi
    gl = GL(backend_path)
    assert gl.is_wrhip, "render_streamed_mirrored: grabs and puts are libwrhip additions"
    assert packed or not scroll, "render_streamed_mirrored: a scroll grab is a packed delta one"
    w, h = frames[0].width, frames[0].height
    r = Renderer(gl, w, h)
    d = r.device
    window = gl.WrhipGetFramebufferTexture(0)
    mirror = d.create_texture(w, h, G.GL_RGBA8, render_target=True)      # (a render target: read_texture reads it at the end)
    d.upload_texture(mirror, 0, 0, w, h, G.GL_BGRA, G.GL_UNSIGNED_BYTE, np.zeros((h, w, 4), np.uint8))
    flags = glapi.GRAB_DELTA | (glapi.GRAB_PACKED if packed else 0) | (glapi.GRAB_SCROLL if scroll else 0)
    rect = (0, 0, w, h)
    windows, mirrors, crossed, waiting = [], [], [], []

    def fetch():
        while waiting:
            windows.append(gl.grab_result(waiting.pop(0))[1])
            mirrors.append(gl.grab_result(waiting.pop(0))[1])
    for f in frames:
        assert (f.width, f.height) == (w, h), "render_streamed_mirrored: one window size"
        r.render(f)
        t = gl.grab_texture(window, rect, flags)
        assert t >= 0, (t, gl.GetError())
        payload = gl.grab_payload(t)
        fetch()                          # (the frame before: in stream order ahead of the payload that has just arrived)
        crossed.append(len(payload))
        rc = gl.put_texture_payload(mirror.id, rect, payload, flags)
        assert rc == 0, (rc, gl.GetError())
        if check:
            for tex in (window, mirror.id):
                t = gl.grab_texture(tex, [rect], 0)
                assert t >= 0, (t, gl.GetError())
                waiting.append(t)
    stats = gl.stats()
    fetch()
    r.finish()
    stats["gl_error"] = int(gl.GetError())
    px = d.read_texture(mirror).copy()
    d.delete_texture(mirror)
    r.destroy()
    return px, stats, windows, mirrors, crossed


def _fed_bytes(window_bgra):
    """What render_streamed_fed feeds back, restated in numpy for a backend without tensor calls: the window's stored bytes (B, G, R,
    A) as a tensor grab's F16 elements of R, G, B with scale 1 / 255 (a float32 multiply, then the rounding to float16), and those as
    a tensor put's bytes with scale 255 (the float16 widened, a float32 multiply, clamped, rounded to nearest even), alpha 255"""
    x = window_bgra[:, :, :3].astype(np.float32) * (np.float32(1.0) / np.float32(255.0))
    y = x.astype(np.float16).astype(np.float32) * np.float32(255.0)
    out = np.empty_like(window_bgra)
    out[:, :, :3] = np.where(y >= 255, 255, np.rint(np.clip(y, 0, 255))).astype(np.uint8)
    out[:, :, 3] = 255
    return out


def render_streamed_fed(backend_path, frames, feed_name, feed=True, initial=None):
    """A closed loop: frame k + 1 draws images textured from frame k's window.  `frames` (one window size) sample a window-sized
    RGBA8 texture they call `feed_name`; two such textures are used alternately -- frame k samples number k % 2 and its window is
    fed into the other one --, both holding `initial` (stored bytes B, G, R, A; None: zeros) at the start.
    libwrhip: after frame k's render the window is tensor-grabbed into device memory (F16, CHW, R, G, B, scale 1 / 255), that tensor
    is put into the other texture (GL.put_texture_tensor, scale 255, alpha 255), and the frame is presented by a plain grab -- no
    Finish, no ReadPixels and no TexSubImage2D of the fed texture anywhere in the loop: the pixels never leave the device except as
    the presented frame.  Any other backend: ReadPixels, the same two conversions in numpy, TexSubImage2D.
    feed=False: the loop without the feedback (both textures keep `initial`), the measure of what the frames themselves cost.
    Returns the presented frames (stored bytes, B, G, R, A) and the backend's statistics (libwrhip; None otherwise)."""
    from . import glapi
    from .device import Texture
    gl = GL(backend_path)
    w, h = frames[0].width, frames[0].height
    r = Renderer(gl, w, h)
    d = r.device
    first = np.zeros((h, w, 4), np.uint8) if initial is None else np.ascontiguousarray(initial, np.uint8)
    assert first.shape == (h, w, 4), first.shape
    ref = None
    for f in frames:
        assert (f.width, f.height) == (w, h), "render_streamed_fed: one window size"
        for t in f.static_textures:
            if t.name == feed_name:
                ref = t
    assert ref is not None and (ref.w, ref.h, ref.fmt) == (w, h, G.GL_RGBA8), "render_streamed_fed: a window-sized RGBA8 texture called feed_name"
    fed = [d.create_texture(w, h, G.GL_RGBA8, ref.filter) for _ in range(2)]
    for t in fed:
        d.upload_texture(t, 0, 0, w, h, G.GL_BGRA, G.GL_UNSIGNED_BYTE, first)
    images, waiting = [], []
    if gl.is_wrhip:
        window = gl.WrhipGetFramebufferTexture(0)
        nbytes = 3 * w * h * 2
        buf = gl.device_alloc(nbytes) if feed else 0
        assert buf or not feed, gl.GetError()
        inv = [float(np.float32(1.0) / np.float32(255.0))] * 4
    for k, f in enumerate(frames):
        r.textures[feed_name] = fed[k % 2]
        r.render(f)
        if not gl.is_wrhip:
            px = d.read_texture(Texture(0, w, h, G.GL_RGBA8, fbo=0)).copy()
            images.append(px)
            if feed:
                d.upload_texture(fed[(k + 1) % 2], 0, 0, w, h, G.GL_BGRA, G.GL_UNSIGNED_BYTE, _fed_bytes(px))
            continue
        if feed:
            t = gl.grab_texture_tensor(window, (0, 0, w, h), buf, nbytes, dtype=glapi.TENSOR_F16, layout=glapi.TENSOR_CHW, channels=3, scale=inv)
            assert t >= 0, (t, gl.GetError())
            rc = gl.put_texture_tensor(fed[(k + 1) % 2].id, (0, 0, w, h), buf, nbytes, dtype=glapi.TENSOR_F16, layout=glapi.TENSOR_CHW,
                                       channels=3, scale=[255.0] * 4, alpha=255)
            assert rc == 0, (rc, gl.GetError())
        if len(waiting) == 8:
            images.append(gl.grab_result(waiting.pop(0))[1])
        t = gl.grab_texture(window, [(0, 0, w, h)], 0)
        assert t >= 0, (t, gl.GetError())
        waiting.append(t)
    stats = None
    if gl.is_wrhip:
        stats = gl.stats()                  # (the loop's: before the results are fetched and the last launches drained)
        images += [gl.grab_result(t)[1] for t in waiting]
        if feed:
            gl.device_free(buf)
    r.finish()
    err = gl.GetError()
    if stats is not None:
        stats["gl_error"] = int(err)
    del r.textures[feed_name]
    for t in fed:
        d.delete_texture(t)
    r.destroy()
    return images, stats
