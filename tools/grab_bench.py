#!/usr/bin/env python3
"""Measurements of texture grabs (include/wrhip.h, WrhipGrabTexture) on the MI355X: DESIGN.md section 6.2.

  pack       wr_grab_pack_kernel on the 3840 x 2160 RGBA8 window (hipEvents, WrhipSetProfiling(1)): full mode, a keyframe delta,
             a delta with nothing changed, a delta with ~2 % of the blocks changed; the three delta lines again with
             WRHIP_GRAB_PACKED (wr_grab_pack_runs_kernel); all of it on a window of noise (every block RAW) and on the cfg2 frame
  transport  33.2 MB from the device slot to the pinned host slot: wr_grab_push_kernel at 8 / 32 / 128 workgroups against
             hipMemcpyAsync, grab call to arrival on the host clock (the pack's time is in it; `pack` says how much that is)
  stream     cfg2 at 4K streamed -- one native replay call per frame from a Python loop, one Finish at the end --, frames/s:
             no grab, a tap per frame, a full grab per frame, a delta grab per frame (identical frames), a ReadPixels per frame;
             then cfg2 frames of different seeds in turn: no grab, a delta grab per frame, a packed delta grab per frame, with the
             bytes per frame that crossed
  scaled     WrhipGrabTextureScaled, the 4K window -> 350 x 197 (L = 3: 2800x1576, 1400x788, 700x394, 350x197), on noise and on the
             cfg2 frame: wr_grab_scale_kernel by hipEvents (kind 15 feat 3); then 50 grabs enqueued back to back with one Finish
             behind them, on the host clock, against the same chain as libwrhip ran it before -- four BlitFramebuffer calls
             (wr_blit_kernel, which has no entry in the kernel statistics: hence the host clock for both) and a full grab of
             level 0; then cfg2 streamed as in `stream`: no grab, a full grab per frame, a scaled grab per frame, frames/s
  tensor     WrhipGrabTextureTensor: wr_grab_tensor_kernel on the 4K window by hipEvents (kind 15 feat 4; F32 CHW 3 is 33.2 MB read +
             99.5 MB written), on noise and on the cfg2 frame; then the 4K cfg2 window -> 3 x 288 x 512 F16 (L = 2, one launch) and
             -> 3 x 224 x 224 F16 (L = 4, two launches), 50 enqueued and one Finish on the host clock, against the path a caller has
             without tensor grabs (BlitFramebuffer chain, WrhipGetTextureDevicePtr, torch gather / permute / cast / scale / bias /
             cast on the draw stream); then cfg2 streamed: no grab, that path per frame, a tensor grab per frame.  With --ab the
             parent-path lines are taken again in a child process that loads the other library
  put        WrhipPutTextureTensor: wr_put_tensor_kernel into the 4K RGBA8 window by hipEvents (kind 16): F16 CHW 3, U8 HWC 4 and F32
             CHW 3 (the tensor grab's headline case the other way); then the same content over the only route there is without it --
             WrhipDeviceRead, the conversion in numpy, TexSubImage2D -- each followed by a tap of the texture as the consumer, host
             clock per frame; then image_grid at 2048 x 2048 streamed by native replay with its window fed back into its atlas every
             frame: a tensor grab and a put, against a tensor grab, WrhipDeviceRead, numpy and TexSubImage2D, frames/s
  yuv        WrhipGrabTextureYuv: wr_grab_yuv_kernel per launch for I420, NV12 and I444, host and device sink, beside the full-mode
             pack of the same job; the cfg2 stream with an I420 host grab per frame against a full grab plus numpy on the host
  yuv_scaled WrhipGrabTextureYuvScaled on the 4K cfg2 window, NV12 and I420: one rendition at 1920 x 1080 (L = 0) and 960 x 540 (L = 1)
             against L + 1 BlitFramebuffer calls plus a WrhipGrabTextureYuv of the last level, 50 enqueued and one Finish on the host
             clock, the new call's launches by hipEvents (kind 15 feat 7); the 1080p / 540p / 270p ladder as one call of three
             renditions against three calls of one; 3840 x 2158 -> 1920 x 1079 I420 with and without FLIP_ROWS (the two routes of
             rendition 0); then cfg2 streamed: no grab, a full-size NV12 grab per frame, a scaled NV12 grab per frame
  scroll     WRHIP_GRAB_SCROLL on a 4K window onto a tall page of noise: the grab's launches (kind 15 feat 8, one entry) beside the one
             launch of DELTA | PACKED on the same frames -- nothing changed, 40 blocks changed, a scroll by 37, both -- with the bytes
             crossed; then 200 frames each scrolled by 37, a grab per frame patched into the caller's image, against DELTA | PACKED and
             no grab.  --scroll-case CASE runs one case's scroll grabs alone for a profiler's kernel trace (the launches one by one)
  yuvscroll  WrhipGrabTextureYuvDelta with GRAB_SCROLL on a 4K window onto a tall page of noise, I420, host sink: the grab's launches
             (kind 15 feat 9, one entry) beside the plain delta YUV grab's one launch on the same frames -- a scroll by 64, nothing
             changed, 40 blocks changed -- with the bytes crossed; then frames each scrolled by 64 and uploaded, a grab per frame,
             host and device sink, with and without GRAB_SCROLL, against no grab
  mirror     WrhipPutTexturePayload into a second 4K texture: the COPY pass and the patch pass by hipEvents (kind 16 feat 2 / feat 1) and
             the put on the host clock, with the bytes staged, for a packed keyframe of cfg2, 40 changed blocks, a keyframe of noise
             (all RAW) and a scroll by 37 -- beside the path there is without it on the same payloads, WrhipGrabDecode into a host
             image and TexSubImage2D of the damage rect; then frames mirrored in a loop without Finish, the scroll case and cfg2 frames
             of four seeds in turn, put against that path, frames/s and bytes per frame each way
  ab         plain bench.py against another build of the library (WRHIP_LIB_PATH), alternated, no grab issued

Every section runs three alternated rounds.  Needs the GPU: there is no fallback.
  python tools/grab_bench.py [--sections pack,transport,stream,scaled,tensor,put,yuv,yuv_delta,yuv_scaled,scroll,yuvscroll,mirror] [--ab PATH_TO_OTHER_LIBWRHIP] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from webrender_amd import glapi, scenes, glconst as G      # noqa: E402
from webrender_amd.renderer import Renderer                # noqa: E402
from webrender_amd.harness import record_scene, ScenePlayer, screenshot_size  # noqa: E402

W, H = 3840, 2160
ROUNDS = 3
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def kernel_stats(gl, kind):
    arr = (glapi.WrhipKernelStat * 64)()
    n = gl.WrhipGetKernelStats(arr, 64)
    return [arr[i] for i in range(n) if arr[i].kind == kind]


class Window:
    """A context with a 4K window of noise, or of the cfg2 frame"""

    def __init__(self, lib, content="noise"):
        self.gl = glapi.GL(lib)
        self.r = Renderer(self.gl, W, H)
        self.tex = self.gl.WrhipGetFramebufferTexture(0)
        if content == "noise":
            self.upload(0, 0, np.random.default_rng(1).integers(0, 256, (H, W, 4), dtype=np.uint8))
        else:
            self.r.render(scenes.make_workload(content, width=W, height=H))
        self.r.finish()

    def upload(self, x, y, px):
        gl = self.gl
        gl.ActiveTexture(G.GL_TEXTURE0)
        gl.BindTexture(G.GL_TEXTURE_2D, self.tex)
        gl.TexSubImage2D(G.GL_TEXTURE_2D, 0, x, y, px.shape[1], px.shape[0], G.GL_BGRA, G.GL_UNSIGNED_BYTE, np.ascontiguousarray(px))

    def grab(self, flags=0, wait=True):
        t = self.gl.grab_texture(self.tex, None, flags)
        assert t >= 0, self.gl.GetError()
        info = glapi.WrhipGrabInfo()
        if wait:
            assert self.gl.WrhipGrabResultGet(t, C.byref(info), None, 0, 1) == 0
        return info

    def close(self):
        self.r.destroy()


def section_pack(lib, content="noise"):
    say(f"## pack: wr_grab_pack_kernel / wr_grab_pack_runs_kernel, {W}x{H} RGBA8 window of {content}, hipEvents (WrhipSetProfiling(1)), us per launch")
    w = Window(lib, content)
    gl = w.gl
    DP = glapi.GRAB_DELTA | glapi.GRAB_PACKED
    for flags in (0, glapi.GRAB_DELTA, DP):          # (untimed: code objects, slots, the retained copy)
        for _ in range(8):
            w.grab(flags)
    rng = np.random.default_rng(2)
    nblocks = (W // 64) * ((H + 63) // 64)
    some = rng.choice(nblocks, size=max(1, nblocks // 50), replace=False)          # ~2 % of the blocks
    patches = [rng.integers(0, 256, (16, 16, 4), dtype=np.uint8) for _ in range(2)]
    gl.WrhipSetProfiling(1)
    rows = {}
    for rnd in range(ROUNDS):
        for name, flags, n in (("full", 0, 30), ("delta keyframe", glapi.GRAB_DELTA | glapi.GRAB_KEY, 30), ("delta unchanged", glapi.GRAB_DELTA, 30),
                               ("delta ~2% changed", glapi.GRAB_DELTA, 10),
                               ("packed keyframe", DP | glapi.GRAB_KEY, 30), ("packed unchanged", DP, 30), ("packed ~2% changed", DP, 10)):
            if name.endswith("unchanged"):
                w.grab(glapi.GRAB_DELTA)
            gl.WrhipResetStats()
            blocks, crossed = [], []
            for k in range(n):
                if name.endswith("~2% changed"):
                    for b in some:
                        w.upload(int(b % (W // 64)) * 64 + 5, int(b // (W // 64)) * 64 + 3, patches[(k + rnd) & 1])
                    gl.WrhipFlush()
                info = w.grab(flags)
                blocks.append(info.blocks)
                crossed.append(info.bytes)
            ks = kernel_stats(gl, 15)
            feat = 2 if flags & glapi.GRAB_PACKED else 1 if flags & glapi.GRAB_DELTA else 0
            assert len(ks) == 1 and ks[0].launches == n and ks[0].feat == feat, [(k.kind, k.feat, k.launches) for k in ks]
            rows.setdefault(name, []).append((ks[0].ns / n / 1e3, ks[0].workgroups // n, int(np.median(blocks)), int(np.median(crossed))))
    gl.WrhipSetProfiling(0)
    for name, v in rows.items():
        say(f"  {name:20s} " + "  ".join(f"{us:8.1f}" for us, _, _, _ in v) + f"   us   ({v[0][1]} workgroups; blocks sent {v[0][2]} of {nblocks}; {v[0][3]} bytes crossed)")
    if content == "noise":
        say("  (beside: wr_tap_kernel 28.9 / 32.4 us for 33.2 / 66.4 MB read; the 6.1 TB/s copy ceiling gives 10.9 us for 33.2 MB read + 33.2 MB written)")
    w.close()


def section_transport(lib):
    say("## transport: the window (33.2 MB at 4K), device slot -> pinned host slot, grab call to arrival (host clock, median of 20; the pack is in it), GB/s")
    variants = [("push kernel, 8 workgroups", "kernel", "8"), ("push kernel, 32 workgroups", "kernel", "32"),
                ("push kernel, 128 workgroups", "kernel", "128"), ("hipMemcpyAsync", "memcpy", "32")]
    rows = {}
    for rnd in range(ROUNDS):
        for name, mode, wgs in variants:
            os.environ["WRHIP_GRAB_FULL_PUSH"] = mode
            os.environ["WRHIP_GRAB_PUSH_WGS"] = wgs
            w = Window(lib)          # (the two variables are read by a context's first grab)
            for _ in range(10):
                w.grab(0)
            ts = []
            for _ in range(20):
                t0 = time.perf_counter()
                info = w.grab(0)
                ts.append(time.perf_counter() - t0)
            rows.setdefault(name, []).append((float(np.median(ts)), int(info.bytes)))
            w.close()
    os.environ.pop("WRHIP_GRAB_FULL_PUSH", None)
    os.environ.pop("WRHIP_GRAB_PUSH_WGS", None)
    for name, v in rows.items():
        say(f"  {name:30s} " + "  ".join(f"{b / t / 1e9:6.1f} GB/s ({t * 1e6:6.0f} us)" for t, b in v))


def section_stream(lib, frames):
    say(f"## stream: cfg2 {W}x{H} streamed, one native replay call per frame from a Python loop, one Finish at the end; {frames} frames per region, frames/s")
    frame = scenes.make_workload("cfg2", width=W, height=H)
    assert (frame.width, frame.height) == (W, H)
    rec, _ = record_scene(lib, frame)
    # (the changing stream's frames are recorded here too: a recording makes and destroys a context of its own, which must not
    # happen while the player's is the library's current one)
    streams = [record_scene(lib, scenes.make_workload("cfg2", width=W, height=H, seed=sd))[0].stream for sd in (1, 2, 3, 4)]
    p = ScenePlayer(lib, rec)
    sym = lambda name, res, *args: C.CFUNCTYPE(res, *args)(p.symbol(name))
    finish = sym("Finish", None)
    window = sym("WrhipGetFramebufferTexture", C.c_uint32, C.c_uint32)(0)
    tap = sym("WrhipTapTexture", C.c_int32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32)
    grab = sym("WrhipGrabTexture", C.c_int32, C.c_uint32, C.c_void_p, C.c_int32, C.c_uint32)
    grab_get = sym("WrhipGrabResultGet", C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32)
    read_pixels = sym("ReadPixels", None, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p)
    get_stats = sym("WrhipGetStats", None, C.c_void_p)
    reset_stats = sym("WrhipResetStats", None)
    rect = (C.c_int32 * 4)(0, 0, W, H)
    host = np.zeros((H, W, 4), np.uint8)
    info = glapi.WrhipGrabInfo()
    one = rec.stream

    def run(kind, n):
        waiting = []

        def fetch(wait):
            while waiting:
                rc = grab_get(waiting[0], C.byref(info), host.ctypes.data if kind != "full grab, info only" else None, 0, 1 if wait else 0)
                if rc == 1:
                    return
                assert rc == 0, rc
                waiting.pop(0)
                wait = False
        for _ in range(n):
            p.rp.exec(one)
            if kind == "tap":
                assert tap(window, 0, 0, W, H, 0) >= 0
            elif kind.startswith("full grab") or kind == "delta grab":
                if len(waiting) == 8:
                    fetch(True)
                t = grab(window, C.addressof(rect), 1, glapi.GRAB_DELTA if kind == "delta grab" else 0)
                assert t >= 0
                waiting.append(t)
                fetch(False)
            elif kind == "ReadPixels":
                read_pixels(0, 0, W, H, G.GL_BGRA, G.GL_UNSIGNED_BYTE, host.ctypes.data)
        finish()
        while waiting:
            fetch(True)

    kinds = ["no grab", "tap", "full grab", "full grab, info only", "delta grab", "ReadPixels"]
    rows, carried = {}, {}
    for k in kinds:
        run(k, 10)
    for rnd in range(ROUNDS):
        for k in kinds:
            n = frames if k != "ReadPixels" else max(20, frames // 4)
            reset_stats()
            t0 = time.perf_counter()
            run(k, n)
            dt = time.perf_counter() - t0
            st = glapi.WrhipStats()
            get_stats(C.byref(st))
            rows.setdefault(k, []).append(n / dt)
            carried.setdefault(k, []).append((int(st.setup_carried), n))
    for k in kinds:
        say(f"  {k:22s} " + "  ".join(f"{v:9.1f}" for v in rows[k]) + f"   frames/s   (setup_carried {carried[k][0][0]} of {carried[k][0][1]} flushes)")
    say("  (full grab / delta grab / ReadPixels deliver into the caller's 33.2 MB image; ReadPixels as GL_BGRA, no CPU swizzle; 'info only' fetches with dst == NULL)")

    # frames that change: cfg2 of four seeds in turn (recorded one by one above; the window and its tiles are the same objects in each)
    say(f"## changing stream: cfg2 {W}x{H} of seeds 1..4 in turn, one grab per frame, {frames} frames per region")
    modes = {"no grab": None, "delta grab": glapi.GRAB_DELTA, "packed delta grab": glapi.GRAB_DELTA | glapi.GRAB_PACKED}

    def run_changing(flags, n):
        waiting, crossed, blocks = [], [], []

        def fetch(wait):
            while waiting:
                rc = grab_get(waiting[0], C.byref(info), host.ctypes.data, 0, 1 if wait else 0)
                if rc == 1:
                    return
                assert rc == 0 and info.status == 0, (rc, info.status)
                waiting.pop(0)
                crossed.append(int(info.bytes))
                blocks.append(int(info.blocks))
                wait = False
        for k in range(n):
            p.rp.exec(streams[k % len(streams)])
            if flags is not None:
                if len(waiting) == 8:
                    fetch(True)
                t = grab(window, C.addressof(rect), 1, flags)
                assert t >= 0
                waiting.append(t)
                fetch(False)
        finish()
        while waiting:
            fetch(True)
        # (the four recordings must address the same objects for the replay to draw them: every frame then differs from the one before)
        assert flags is None or (len(blocks) == n and min(blocks[1:]) > 0), f"frames that did not change: blocks per frame {blocks}"
        return crossed, blocks

    check = np.zeros((H, W, 4), np.uint8)
    for name, flags in modes.items():
        run_changing(flags, 12)
        if flags is not None:          # (the patched image is the window)
            read_pixels(0, 0, W, H, G.GL_BGRA, G.GL_UNSIGNED_BYTE, check.ctypes.data)
            assert np.array_equal(check, host), f"{name}: the patched image is not the window"
    crows = {}
    for rnd in range(ROUNDS):
        for name, flags in modes.items():
            t0 = time.perf_counter()
            crossed, blocks = run_changing(flags, frames)
            dt = time.perf_counter() - t0
            crows.setdefault(name, []).append((frames / dt, float(np.mean(crossed[1:])) if crossed else 0.0, float(np.mean(blocks[1:])) if blocks else 0.0))
    for name, v in crows.items():
        say(f"  {name:22s} " + "  ".join(f"{fps:9.1f}" for fps, _, _ in v) + "   frames/s   " + (f"({v[0][1] / 1e6:7.3f} MB and {v[0][2]:6.1f} blocks per frame crossed)" if v[0][1] else ""))


def section_scaled(lib, content):
    dw, dh = screenshot_size((W, H), (350, 350))
    L = 0
    while W > 2 * dw * (1 << L):
        L += 1
    say(f"## scaled: {W}x{H} window of {content} -> {dw}x{dh}, L = {L}")
    w = Window(lib, content)
    gl, d = w.gl, w.r.device
    levels = [d.create_texture(dw << k, dh << k, G.GL_RGBA8, render_target=True) for k in range(L + 1)]

    def blit(src_fbo, sw, sh, dst):
        gl.BindFramebuffer(G.GL_READ_FRAMEBUFFER, src_fbo)
        gl.BindFramebuffer(G.GL_DRAW_FRAMEBUFFER, dst.fbo)
        gl.BlitFramebuffer(0, 0, sw, sh, 0, 0, dst.width, dst.height, G.GL_COLOR_BUFFER_BIT, G.GL_LINEAR)

    def chain():
        blit(0, W, H, levels[L])
        for k in range(L - 1, -1, -1):
            blit(levels[k + 1].fbo, levels[k + 1].width, levels[k + 1].height, levels[k])
        gl.BindFramebuffer(G.GL_DRAW_FRAMEBUFFER, 0)
        gl.BindFramebuffer(G.GL_READ_FRAMEBUFFER, 0)
        return gl.grab_texture(levels[0].id)

    def fused():
        return gl.grab_texture_scaled(w.tex, None, (dw, dh))
    # the two agree byte for byte (and both are warm)
    a = gl.grab_result(chain())[1]
    b = gl.grab_result(fused())[1]
    assert np.array_equal(a, b), "the fused pass and the blit chain differ"
    algo = W * H * 4 + dw * dh * 4
    N = 50
    ev, host = [], {"chain": [], "fused": []}
    for rnd in range(ROUNDS):
        gl.WrhipSetProfiling(1)
        gl.WrhipResetStats()
        for _ in range(30):
            t = fused()
        gl.grab_result(t)
        ks = [k for k in kernel_stats(gl, 15) if k.feat == 3]
        assert len(ks) == 1 and ks[0].launches == 30 and ks[0].algo_bytes == 30 * algo, [(k.feat, k.launches, k.algo_bytes) for k in ks]
        ev.append(ks[0].ns / 30 / 1e3)
        gl.WrhipSetProfiling(0)
        for name, fn in (("chain", chain), ("fused", fused)):
            gl.Finish()
            t0 = time.perf_counter()
            for _ in range(N):
                t = fn()
            gl.Finish()
            host[name].append((time.perf_counter() - t0) / N * 1e6)
            gl.grab_result(t)
    say("  wr_grab_scale_kernel, hipEvents     " + "  ".join(f"{us:8.1f}" for us in ev) + f"   us per launch   ({algo / 1e6:.2f} MB algorithmic: " + "  ".join(f"{algo / us / 1e3:6.0f}" for us in ev) + " GB/s)")
    say(f"  {N} enqueued, one Finish, host clock, us per grab:")
    say(f"    {L + 1} x BlitFramebuffer + full grab   " + "  ".join(f"{us:8.1f}" for us in host["chain"]))
    say("    WrhipGrabTextureScaled            " + "  ".join(f"{us:8.1f}" for us in host["fused"]))
    w.close()


def section_scaled_stream(lib, frames):
    dw, dh = screenshot_size((W, H), (350, 350))
    say(f"## scaled stream: cfg2 {W}x{H} streamed as in `stream`, {frames} frames per region, frames/s; the scaled grab delivers {dw}x{dh}")
    rec, _ = record_scene(lib, scenes.make_workload("cfg2", width=W, height=H))
    p = ScenePlayer(lib, rec)
    sym = lambda name, res, *args: C.CFUNCTYPE(res, *args)(p.symbol(name))
    finish = sym("Finish", None)
    window = sym("WrhipGetFramebufferTexture", C.c_uint32, C.c_uint32)(0)
    grab = sym("WrhipGrabTexture", C.c_int32, C.c_uint32, C.c_void_p, C.c_int32, C.c_uint32)
    grab_scaled = sym("WrhipGrabTextureScaled", C.c_int32, C.c_uint32, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32)
    grab_get = sym("WrhipGrabResultGet", C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32)
    get_stats = sym("WrhipGetStats", None, C.c_void_p)
    reset_stats = sym("WrhipResetStats", None)
    rect = (C.c_int32 * 4)(0, 0, W, H)
    host = np.zeros((H, W, 4), np.uint8)
    info = glapi.WrhipGrabInfo()

    def run(kind, n):
        waiting = []

        def fetch(wait):
            while waiting:
                rc = grab_get(waiting[0], C.byref(info), host.ctypes.data, 0, 1 if wait else 0)
                if rc == 1:
                    return
                assert rc == 0, rc
                waiting.pop(0)
                wait = False
        for _ in range(n):
            p.rp.exec(rec.stream)
            if kind != "no grab":
                if len(waiting) == 8:
                    fetch(True)
                t = grab(window, C.addressof(rect), 1, 0) if kind == "full grab" else grab_scaled(window, C.addressof(rect), dw, dh, 0)
                assert t >= 0
                waiting.append(t)
                fetch(False)
        finish()
        while waiting:
            fetch(True)
    kinds = ["no grab", "full grab", "scaled grab"]
    rows, carried = {}, {}
    for k in kinds:
        run(k, 10)
    for rnd in range(ROUNDS):
        for k in kinds:
            reset_stats()
            t0 = time.perf_counter()
            run(k, frames)
            dt = time.perf_counter() - t0
            st = glapi.WrhipStats()
            get_stats(C.byref(st))
            rows.setdefault(k, []).append(frames / dt)
            carried.setdefault(k, []).append(int(st.setup_carried))
    for k in kinds:
        say(f"  {k:22s} " + "  ".join(f"{v:9.1f}" for v in rows[k]) + f"   frames/s   (setup_carried {carried[k][0]} of {frames} flushes)")


# ---- tensor grabs (WrhipGrabTextureTensor) -----------------------------------------------------------------
_MEAN, _STD = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
T_SCALE, T_BIAS = np.float32(1.0) / (np.float32(255.0) * _STD), -_MEAN / _STD
T_SIZES = ((512, 288), (224, 224))              # (w, h): L = 2, one launch; L = 4, two launches


def _levels(dw):
    L = 0
    while W > 2 * dw * (1 << L):
        L += 1
    return L


class ParentPath:
    """What a caller has without tensor grabs: the BlitFramebuffer chain to level 0 (L + 1 wr_blit_kernel launches through HBM),
    WrhipFlush + WrhipGetTextureDevicePtr (the held-back launches are sent), then torch on the draw stream: channel gather,
    permute, cast, scale, bias, cast into a batch slot.  Needs nothing a library without tensor grabs lacks."""

    def __init__(self, gl, size, slots, names=0):
        """names: the first of the texture and framebuffer names to use instead of generated ones (a context a recorded trace is
        replayed in: the trace names objects by the numbers the generator gave when it was recorded, so nothing else may draw from it)"""
        self.names = names
        import torch
        from webrender_amd.dist import DeviceArray
        self.gl, self.torch, self.DeviceArray = gl, torch, DeviceArray
        self.dw, self.dh = size
        self.L = _levels(self.dw)
        self.levels = [self._texture(self.dw << k, self.dh << k) for k in range(self.L + 1)]
        self.stream = torch.cuda.ExternalStream(int(gl.WrhipGetStream()))
        self.batch = torch.empty((slots, 3, self.dh, self.dw), dtype=torch.float16, device="cuda")
        self.scale = torch.from_numpy(T_SCALE).cuda()[:, None, None]
        self.bias = torch.from_numpy(T_BIAS).cuda()[:, None, None]
        self.order = torch.tensor([2, 1, 0], device="cuda")
        torch.cuda.synchronize()

    def _texture(self, w, h):
        gl = self.gl
        if self.names:
            tid = fbo = self.names
            self.names += 1
        else:
            tid, fbo = gl.gen("GenTextures"), gl.gen("GenFramebuffers")
        gl.ActiveTexture(G.GL_TEXTURE0)
        gl.BindTexture(G.GL_TEXTURE_2D, tid)
        gl.TexStorage2D(G.GL_TEXTURE_2D, 1, G.GL_RGBA8, w, h)
        gl.BindFramebuffer(G.GL_DRAW_FRAMEBUFFER, fbo)
        gl.FramebufferTexture2D(G.GL_DRAW_FRAMEBUFFER, G.GL_COLOR_ATTACHMENT0, G.GL_TEXTURE_2D, tid, 0)
        gl.BindFramebuffer(G.GL_DRAW_FRAMEBUFFER, 0)
        return (tid, fbo, w, h)

    def __call__(self, k):
        gl, torch = self.gl, self.torch
        src = (0, 0, W, H)
        for lv in range(self.L, -1, -1):
            tid, fbo, w, h = self.levels[lv]
            gl.BindFramebuffer(G.GL_READ_FRAMEBUFFER, src[1])
            gl.BindFramebuffer(G.GL_DRAW_FRAMEBUFFER, fbo)
            gl.BlitFramebuffer(0, 0, src[2], src[3], 0, 0, w, h, G.GL_COLOR_BUFFER_BIT, G.GL_LINEAR)
            src = self.levels[lv]
        gl.BindFramebuffer(G.GL_DRAW_FRAMEBUFFER, 0)
        gl.BindFramebuffer(G.GL_READ_FRAMEBUFFER, 0)
        gl.WrhipFlush()
        stride = C.c_int32(0)
        ptr = gl.WrhipGetTextureDevicePtr(self.levels[0][0], None, None, C.byref(stride))
        raw = torch.as_tensor(self.DeviceArray(ptr, self.dh * stride.value), device="cuda")
        with torch.cuda.stream(self.stream):
            px = raw.view(self.dh, stride.value)[:, :self.dw * 4].reshape(self.dh, self.dw, 4)
            x = px.index_select(2, self.order).permute(2, 0, 1).float()
            self.batch[k % self.batch.shape[0]].copy_((x * self.scale + self.bias).half())

    def slot_bits(self, k):
        self.stream.synchronize()
        return self.batch[k % self.batch.shape[0]].cpu().numpy().view(np.uint16)


def section_tensor_kernel(lib, content):
    say(f"## tensor, unscaled: wr_grab_tensor_kernel, {W}x{H} RGBA8 window of {content}, hipEvents (WrhipSetProfiling(1)), us per launch")
    w = Window(lib, content)
    gl = w.gl
    cases = (("F32 CHW 3", glapi.TENSOR_F32, glapi.TENSOR_CHW, 3), ("F16 CHW 3", glapi.TENSOR_F16, glapi.TENSOR_CHW, 3),
             ("BF16 CHW 3", glapi.TENSOR_BF16, glapi.TENSOR_CHW, 3), ("F16 HWC 3", glapi.TENSOR_F16, glapi.TENSOR_HWC, 3),
             ("U8  CHW 3", glapi.TENSOR_U8, glapi.TENSOR_CHW, 3), ("F32 HWC 4", glapi.TENSOR_F32, glapi.TENSOR_HWC, 4))
    buf = gl.device_alloc(W * H * 16)
    assert buf, gl.GetError()
    info = glapi.WrhipGrabInfo()

    def grab(dtype, layout, ch):
        t = gl.grab_texture_tensor(w.tex, None, buf, W * H * 16, dtype=dtype, layout=layout, channels=ch, scale=T_SCALE, bias=T_BIAS)
        assert t >= 0, gl.GetError()
        assert gl.WrhipGrabResultGet(t, C.byref(info), None, 0, 1) == 0
    for _, dtype, layout, ch in cases:
        for _ in range(4):
            grab(dtype, layout, ch)
    gl.WrhipSetProfiling(1)
    rows, n = {}, 30
    for rnd in range(ROUNDS):
        for name, dtype, layout, ch in cases:
            gl.WrhipResetStats()
            for _ in range(n):
                grab(dtype, layout, ch)
            ks = [k for k in kernel_stats(gl, 15) if k.feat == 4]
            assert len(ks) == 1 and ks[0].launches == n, [(k.feat, k.launches) for k in ks]
            rows.setdefault(name, []).append((ks[0].ns / n / 1e3, ks[0].algo_bytes // n, ks[0].workgroups // n))
    gl.WrhipSetProfiling(0)
    for name, v in rows.items():
        say(f"  {name:12s} " + "  ".join(f"{us:8.1f}" for us, _, _ in v) + f"   us   ({v[0][1] / 1e6:6.1f} MB read + written: " +
            "  ".join(f"{b / us / 1e3:6.0f}" for us, b, _ in v) + f" GB/s; {v[0][2]} workgroups)")
    say("  (beside: the full-mode pack, 14.2 us for 33.2 MB read + 33.2 MB written, 4.7 TB/s: DESIGN.md section 6.2)")
    gl.device_free(buf)
    w.close()


def section_tensor_scaled(lib, with_tensor=True):
    """50 enqueued, one Finish, host clock per grab: the parent path, and (with_tensor) the tensor grab"""
    say(f"## tensor, scaled: {W}x{H} window of cfg2 -> 3 x h x w F16, 50 enqueued, one Finish, host clock, us per grab" + ("" if with_tensor else "   [THE PARENT'S LIBRARY]"))
    w = Window(lib, "cfg2")
    gl = w.gl
    N = 50
    for size in T_SIZES:
        L = _levels(size[0])
        pp = ParentPath(gl, size, N)
        slot = size[0] * size[1] * 3 * 2
        slot16 = (slot + 15) & ~15
        buf = gl.device_alloc(slot16 * N) if with_tensor else 0

        def tensor(k):
            t = gl.grab_texture_tensor(w.tex, None, buf + (k % N) * slot16, slot, size=size, dtype=glapi.TENSOR_F16, channels=3, scale=T_SCALE, bias=T_BIAS)
            assert t >= 0, gl.GetError()
        kinds = [("parent path", pp)] + ([("tensor grab", tensor)] if with_tensor else [])
        for _, fn in kinds:
            for k in range(4):
                fn(k)
        gl.Finish()
        if with_tensor:
            mine = gl.device_read(buf, slot).view(np.uint16).reshape(3, size[1], size[0])
            say(f"  {size[0]}x{size[1]} (L = {L}, {1 + L // 4} launch(es)): elements in which the parent path's tensor differs from the tensor grab's: {int((pp.slot_bits(0) != mine).sum())} of {mine.size}")
        host = {}
        for rnd in range(ROUNDS):
            for name, fn in kinds:
                gl.Finish()
                pp.torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(N):
                    fn(k)
                gl.Finish()
                pp.stream.synchronize()
                host.setdefault(name, []).append((time.perf_counter() - t0) / N * 1e6)
        for name, v in host.items():
            say(f"    {size[0]}x{size[1]}  {name:12s} " + "  ".join(f"{us:8.1f}" for us in v))
        if with_tensor:
            say(f"    {size[0]}x{size[1]}  ratio parent / tensor, by round: " + "  ".join(f"{a / b:6.2f}" for a, b in zip(host["parent path"], host["tensor grab"])))
            gl.device_free(buf)
    w.close()


def section_tensor_stream(lib, frames, with_tensor=True):
    size = T_SIZES[1]
    say(f"## tensor stream: cfg2 {W}x{H} streamed as in `stream`, {frames} frames per region, frames/s; every frame to 3 x {size[1]} x {size[0]} F16 in a batch slot" + ("" if with_tensor else "   [THE PARENT'S LIBRARY]"))
    rec, _ = record_scene(lib, scenes.make_workload("cfg2", width=W, height=H))
    p = ScenePlayer(lib, rec)
    gl = glapi.GL(lib)                          # (the same loaded library and current context as the player's)
    window = gl.WrhipGetFramebufferTexture(0)
    N = 64
    pp = ParentPath(gl, size, N, names=6000)
    slot = size[0] * size[1] * 3 * 2
    slot16 = (slot + 15) & ~15
    buf = gl.device_alloc(slot16 * N) if with_tensor else 0
    info = glapi.WrhipGrabInfo()

    def run(kind, n):
        t = -1
        for k in range(n):
            p.rp.exec(rec.stream)
            if kind == "tensor grab":
                t = gl.grab_texture_tensor(window, (0, 0, W, H), buf + (k % N) * slot16, slot, size=size, dtype=glapi.TENSOR_F16, channels=3, scale=T_SCALE, bias=T_BIAS)
                assert t >= 0
            elif kind == "parent path":
                pp(k)
        if t >= 0:
            assert gl.WrhipGrabResultGet(t, C.byref(info), None, 0, 1) == 0          # (the last ticket: one stream, in order)
        gl.Finish()
        pp.stream.synchronize()
    kinds = ["no grab", "parent path"] + (["tensor grab"] if with_tensor else [])
    rows, carried = {}, {}
    for k in kinds:
        run(k, 10)
    for rnd in range(ROUNDS):
        for k in kinds:
            gl.WrhipResetStats()
            t0 = time.perf_counter()
            run(k, frames)
            dt = time.perf_counter() - t0
            rows.setdefault(k, []).append(frames / dt)
            carried.setdefault(k, []).append(gl.stats()["setup_carried"])
    for k in kinds:
        say(f"  {k:14s} " + "  ".join(f"{v:9.1f}" for v in rows[k]) + f"   frames/s   (setup_carried {carried[k][0]} of {frames} flushes)")
    if with_tensor:
        gl.device_free(buf)


def section_tensor_parent(other, frames):
    """The parent-path lines again, in a fresh process that loads the parent's library"""
    env = dict(os.environ, WRHIP_LIB_PATH=os.path.abspath(other))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--sections", "tensor_parent", "--frames", str(frames), "--rounds", str(ROUNDS), "--size", f"{W}x{H}"],
                         env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    if out.returncode != 0:
        say(f"  the parent's library: exited with {out.returncode}: {out.stderr[-400:]}")
        return
    for l in out.stdout.splitlines():
        if not l.startswith("# "):
            say(l)


def _put_bytes(el, dtype, hwc, scale):
    """The put's conversion on the host, as the route without it has to do it: elements -> stored B, G, R, A bytes"""
    x = el if hwc else el.transpose(1, 2, 0)
    if dtype != glapi.TENSOR_U8:
        y = x.astype(np.float32) * np.float32(scale)
        x = np.where(y >= 255, 255, np.rint(np.clip(y, 0, 255))).astype(np.uint8)
    out = np.empty(x.shape[:2] + (4,), np.uint8)
    out[..., 0], out[..., 1], out[..., 2] = x[..., 2], x[..., 1], x[..., 0]
    out[..., 3] = x[..., 3] if x.shape[2] == 4 else 255
    return out


def section_put(lib):
    say(f"## put: wr_put_tensor_kernel into the {W}x{H} RGBA8 window, hipEvents (WrhipSetProfiling(1)), us per launch")
    w = Window(lib, "noise")
    gl = w.gl
    rng = np.random.default_rng(2)
    unit = rng.random((3, H, W), dtype=np.float32)
    data = {"F16 CHW 3": (unit.astype(np.float16), glapi.TENSOR_F16, glapi.TENSOR_CHW, 3, 255.0),
            "U8  HWC 4": (rng.integers(0, 256, (H, W, 4), dtype=np.uint8), glapi.TENSOR_U8, glapi.TENSOR_HWC, 4, 1.0),
            "F32 CHW 3": (unit, glapi.TENSOR_F32, glapi.TENSOR_CHW, 3, 255.0)}
    bufs = {}
    for name, (el, *_) in data.items():
        bufs[name] = gl.device_alloc(el.nbytes)
        assert bufs[name], gl.GetError()
        gl.device_write(bufs[name], el)

    def put(name):
        el, dtype, layout, ch, scale = data[name]
        assert gl.put_texture_tensor(w.tex, None, bufs[name], el.nbytes, dtype=dtype, layout=layout, channels=ch, scale=[scale] * 4) == 0, gl.GetError()
    for name in data:
        for _ in range(4):
            put(name)
    # (what the kernel wrote, against the host's conversion: the figures below are of a kernel that is right)
    for name in data:
        put(name)
        got = np.empty((H, W, 4), np.uint8)
        gl.BindFramebuffer(G.GL_READ_FRAMEBUFFER, 0)
        gl.ReadPixels(0, 0, W, H, G.GL_BGRA, G.GL_UNSIGNED_BYTE, got)
        el, dtype, layout, ch, scale = data[name]
        say(f"  {name}: bytes that differ from the numpy conversion: {int((got != _put_bytes(el, dtype, layout == glapi.TENSOR_HWC, scale)).sum())}")
    gl.WrhipSetProfiling(1)
    rows, n = {}, 30
    for rnd in range(ROUNDS):
        for name in data:
            gl.WrhipResetStats()
            for _ in range(n):
                put(name)
            ks = kernel_stats(gl, 16)
            assert len(ks) == 1 and ks[0].launches == n, [(k.feat, k.launches) for k in ks]
            rows.setdefault(name, []).append((ks[0].ns / n / 1e3, ks[0].algo_bytes // n, ks[0].workgroups // n))
    gl.WrhipSetProfiling(0)
    for name, v in rows.items():
        say(f"  {name:12s} " + "  ".join(f"{us:8.1f}" for us, _, _ in v) + f"   us   ({v[0][1] / 1e6:6.1f} MB read + written: " +
            "  ".join(f"{b / us / 1e3:6.0f}" for us, b, _ in v) + f" GB/s; {v[0][2]} workgroups)")
    say(f"## put against the route without it: the same {W}x{H} content, WrhipDeviceRead + numpy + TexSubImage2D; a tap of the texture consumes it; host clock, ms per frame")
    N = 5
    host = {}
    for rnd in range(ROUNDS):
        for name in ("F16 CHW 3", "U8  HWC 4"):
            el, dtype, layout, ch, scale = data[name]
            for kind in ("put", "host route"):
                gl.Finish()
                t0 = time.perf_counter()
                for _ in range(N):
                    if kind == "put":
                        put(name)
                    else:
                        raw = gl.device_read(bufs[name], el.nbytes).view(el.dtype).reshape(el.shape)
                        w.upload(0, 0, _put_bytes(raw, dtype, layout == glapi.TENSOR_HWC, scale))
                    t = gl.tap_texture(w.tex)
                gl.tap_result(t)
                host.setdefault((name, kind), []).append((time.perf_counter() - t0) / N * 1e3)
    for (name, kind), v in host.items():
        say(f"  {name:10s} {kind:11s} " + "  ".join(f"{ms:9.3f}" for ms in v) + "   ms")
    for b in bufs.values():
        gl.device_free(b)
    w.close()


def section_put_stream(lib, frames):
    S = 2048
    say(f"## put stream: image_grid {S}x{S} streamed by native replay, the window fed back into the {S}x{S} atlas every frame, {frames} frames per region, frames/s")
    rec, _ = record_scene(lib, scenes.image_grid(width=S, height=S, atlas=S))
    p = ScenePlayer(lib, rec)
    gl = glapi.GL(lib)
    window, atlas = gl.WrhipGetFramebufferTexture(0), rec.texture_ids["image_atlas"]
    nbytes = 3 * S * S * 2
    buf = gl.device_alloc(nbytes)
    inv = [1.0 / 255.0] * 4

    def run(kind, n):
        for k in range(n):
            p.rp.exec(rec.stream)
            if kind == "no feed":
                continue
            t = gl.grab_texture_tensor(window, (0, 0, S, S), buf, nbytes, dtype=glapi.TENSOR_F16, channels=3, scale=inv)
            assert t >= 0
            if kind == "put":
                assert gl.put_texture_tensor(atlas, (0, 0, S, S), buf, nbytes, dtype=glapi.TENSOR_F16, channels=3, scale=[255.0] * 4) == 0
            else:
                raw = gl.device_read(buf, nbytes).view(np.float16).reshape(3, S, S)
                gl.ActiveTexture(G.GL_TEXTURE0)
                gl.BindTexture(G.GL_TEXTURE_2D, atlas)
                gl.TexSubImage2D(G.GL_TEXTURE_2D, 0, 0, 0, S, S, G.GL_BGRA, G.GL_UNSIGNED_BYTE, _put_bytes(raw, glapi.TENSOR_F16, False, 255.0))
        gl.Finish()
    kinds = ["no feed", "put", "host route"]
    rows = {}
    for k in kinds:
        run(k, 3)
    for rnd in range(ROUNDS):
        for k in kinds:
            n = frames if k != "host route" else max(5, frames // 20)
            t0 = time.perf_counter()
            run(k, n)
            rows.setdefault(k, []).append(n / (time.perf_counter() - t0))
    for k in kinds:
        say(f"  {k:12s} " + "  ".join(f"{v:9.1f}" for v in rows[k]) + "   frames/s")
    gl.device_free(buf)


# ---- YUV grabs (WrhipGrabTextureYuv) ------------------------------------------------------------------------
YUV_NAMES = {glapi.YUV_I420: "I420", glapi.YUV_NV12: "NV12", glapi.YUV_I444: "I444"}
YUV_ROWS = np.array([[11966, 40254, 4064], [-6596, -22188, 28784], [28784, -26145, -2639]], np.int32)      # Rec709Narrow: Y, Cb, Cr over R, G, B


def yuv_numpy_i420(px):
    """The contract's I420 planes of Rec709Narrow restated in numpy on the host -- what a caller does today behind a full grab"""
    rgb = px[..., [2, 1, 0]].astype(np.int32)
    y = ((rgb @ YUV_ROWS[0] + (16 << 16) + 0x8000) >> 16).astype(np.uint8)
    h, w = y.shape
    ys, xs = np.minimum(np.arange(0, 2 * ((h + 1) // 2)), h - 1), np.minimum(np.arange(0, 2 * ((w + 1) // 2)), w - 1)
    v = rgb[ys][:, xs]
    s = v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2]
    c = [np.clip((s @ YUV_ROWS[k] + (128 << 18) + (1 << 17)) >> 18, 0, 255).astype(np.uint8) for k in (1, 2)]
    return np.concatenate([y.reshape(-1), c[0].reshape(-1), c[1].reshape(-1)])


def section_yuv_kernel(lib, content):
    say(f"## yuv: wr_grab_yuv_kernel, {W}x{H} RGBA8 window of {content}, Rec709Narrow, hipEvents (WrhipSetProfiling(1)), us per launch")
    w = Window(lib, content)
    gl = w.gl
    buf = gl.device_alloc(W * H * 3)
    assert buf, gl.GetError()
    info = glapi.WrhipGrabInfo()

    def grab(fmt, device):
        if fmt is None:
            return w.grab(0)
        t = gl.grab_texture_yuv(w.tex, None, fmt, glapi.YUV_REC709_NARROW, dst=buf if device else None, dst_bytes=W * H * 3 if device else 0)
        assert t >= 0, gl.GetError()
        assert gl.WrhipGrabResultGet(t, C.byref(info), None, 0, 1) == 0
    cases = [("full-mode pack", None, False)] + [(f"{YUV_NAMES[f]} {'device' if d else 'host  '}", f, d) for f in YUV_NAMES for d in (True, False)]
    for _, fmt, dev in cases:
        for _ in range(4):
            grab(fmt, dev)
    if content == "noise":
        flat = gl.grab_result(gl.grab_texture_yuv(w.tex, None, glapi.YUV_I420, glapi.YUV_REC709_NARROW))[1]
        px = gl.grab_result(gl.grab_texture(w.tex, None, 0))[1]
        say(f"  bytes in which the I420 grab differs from numpy on the full grab's pixels: {int((flat != yuv_numpy_i420(px)).sum())} of {flat.size}")
    gl.WrhipSetProfiling(1)
    rows, n = {}, 30
    for rnd in range(ROUNDS):
        for name, fmt, dev in cases:
            gl.WrhipResetStats()
            for _ in range(n):
                grab(fmt, dev)
            ks = [k for k in kernel_stats(gl, 15) if k.feat == (0 if fmt is None else 5)]
            assert len(ks) == 1 and ks[0].launches == n, [(k.feat, k.launches) for k in ks]
            rows.setdefault(name, []).append((ks[0].ns / n / 1e3, ks[0].algo_bytes // n, ks[0].workgroups // n))
    gl.WrhipSetProfiling(0)
    for name, v in rows.items():
        say(f"  {name:14s} " + "  ".join(f"{us:8.1f}" for us, _, _ in v) + f"   us   ({v[0][1] / 1e6:6.1f} MB read + written: " +
            "  ".join(f"{b / us / 1e3:6.0f}" for us, b, _ in v) + f" GB/s; {v[0][2]} workgroups)")
    gl.device_free(buf)
    w.close()


def section_yuv_stream(lib, frames):
    say(f"## yuv stream: cfg2 {W}x{H} streamed as in `stream`, {frames} frames per region, frames/s; tickets fetched one frame late")
    rec, _ = record_scene(lib, scenes.make_workload("cfg2", width=W, height=H))
    p = ScenePlayer(lib, rec)
    gl = glapi.GL(lib)                          # (the same loaded library and current context as the player's)
    window = gl.WrhipGetFramebufferTexture(0)
    payload = W * H + 2 * ((W + 1) // 2) * ((H + 1) // 2)
    host = np.empty(W * H * 4, np.uint8)
    info = glapi.WrhipGrabInfo()

    def run(kind, n):
        prev = -1

        def fetch(t):
            assert gl.WrhipGrabResultGet(t, C.byref(info), host.ctypes.data, 0, 1) == 0
            if kind == "full grab + numpy":
                yuv_numpy_i420(host.reshape(H, W, 4))
        for k in range(n):
            p.rp.exec(rec.stream)
            t = -1
            if kind == "I420 host grab":
                t = gl.grab_texture_yuv(window, (0, 0, W, H), glapi.YUV_I420, glapi.YUV_REC709_NARROW)
            elif kind == "full grab + numpy":
                t = gl.grab_texture(window, (0, 0, W, H), 0)
            if prev >= 0:
                fetch(prev)
            prev = t
        if prev >= 0:
            fetch(prev)
        gl.Finish()
    kinds = ["no grab", "I420 host grab", "full grab + numpy"]
    rows, carried, crossed = {}, {}, {}
    for k in kinds:
        run(k, 4)
    for rnd in range(ROUNDS):
        for k in kinds:
            n = frames if k != "full grab + numpy" else max(4, frames // 10)      # (the host conversion: tens of ms per frame)
            gl.WrhipResetStats()
            t0 = time.perf_counter()
            run(k, n)
            dt = time.perf_counter() - t0
            st = gl.stats()
            rows.setdefault(k, []).append(n / dt)
            carried[k] = (st["setup_carried"], n)
            crossed[k] = st["d2h_bytes"] / n
    for k in kinds:
        say(f"  {k:18s} " + "  ".join(f"{v:9.1f}" for v in rows[k]) + f"   frames/s   (setup_carried {carried[k][0]} of {carried[k][1]} flushes; {crossed[k] / 1e6:.2f} MB per frame crossed)")
    say(f"  (an I420 payload is {payload / 1e6:.2f} MB, a full grab's {W * H * 4 / 1e6:.2f} MB)")


# ---- scaled YUV grabs (WrhipGrabTextureYuvScaled) -----------------------------------------------------------
def section_yuv_scaled(lib):
    say(f"## yuv_scaled: {W}x{H} RGBA8 window of cfg2, Rec709Narrow, host sink; 50 enqueued grabs behind one Finish, host clock, us per grab;")
    say("##             launch times: hipEvents (WrhipSetProfiling(1)), all launches of a grab together")
    w = Window(lib, "cfg2")
    gl, d = w.gl, w.r.device
    sp = glapi.YUV_REC709_NARROW
    sizes = [(W // 2, H // 2), (W // 4, H // 4), (W // 8, H // 8)]
    own = {}        # the baseline's textures of its own: one chain per size

    def blit(src_fbo, sw, sh, dst):
        gl.BindFramebuffer(G.GL_READ_FRAMEBUFFER, src_fbo)
        gl.BindFramebuffer(G.GL_DRAW_FRAMEBUFFER, dst.fbo)
        gl.BlitFramebuffer(0, 0, sw, sh, 0, 0, dst.width, dst.height, G.GL_COLOR_BUFFER_BIT, G.GL_LINEAR)

    def chain(size, fmt):
        """What a caller does without the call: L + 1 BlitFramebuffer calls into textures of its own, then a YUV grab of the last"""
        L = _levels(size[0])
        if size not in own:
            own[size] = [d.create_texture(size[0] << k, size[1] << k, G.GL_RGBA8, render_target=True) for k in range(L + 1)]
        lv = own[size]
        blit(0, W, H, lv[L])
        for k in range(L - 1, -1, -1):
            blit(lv[k + 1].fbo, lv[k + 1].width, lv[k + 1].height, lv[k])
        gl.BindFramebuffer(G.GL_DRAW_FRAMEBUFFER, 0)
        gl.BindFramebuffer(G.GL_READ_FRAMEBUFFER, 0)
        return gl.grab_texture_yuv(lv[0].id, None, fmt, sp)

    def fused(size, fmt, n=1, rect=None, flags=0):
        t = gl.grab_texture_yuv_scaled(w.tex, rect, size, fmt, sp, flags, renditions=n)
        assert t >= 0, gl.GetError()
        return t

    def timed(fn, N=50):
        gl.Finish()
        t0 = time.perf_counter()
        for _ in range(N):
            t = fn()
        gl.Finish()
        dt = (time.perf_counter() - t0) / N * 1e6
        gl.grab_result(t)
        return dt

    def events(fn, n=30):
        gl.WrhipSetProfiling(1)
        gl.WrhipResetStats()
        for _ in range(n):
            t = fn()
        gl.grab_result(t)
        ks = [k for k in kernel_stats(gl, 15) if k.feat == 7]
        gl.WrhipSetProfiling(0)
        assert len(ks) == 1 and ks[0].launches == n, [(k.feat, k.launches) for k in ks]
        return ks[0].ns / n / 1e3
    fmts = (glapi.YUV_NV12, glapi.YUV_I420)
    # 1. a single rendition against the chain of blits plus a YUV grab; the two agree byte for byte (and both are warm)
    for size in sizes[:2]:
        for fmt in fmts:
            a, b = gl.grab_result(chain(size, fmt))[1], gl.grab_result(fused(size, fmt))[1]
            assert np.array_equal(a, b), "the fused pass and the blit chain differ"
    rows = {}
    for rnd in range(ROUNDS):
        for size in sizes[:2]:
            for fmt in fmts:
                key = (size, fmt)
                rows.setdefault(key, {"chain": [], "fused": [], "ev": []})
                rows[key]["chain"].append(timed(lambda: chain(size, fmt)))
                rows[key]["fused"].append(timed(lambda: fused(size, fmt)))
                rows[key]["ev"].append(events(lambda: fused(size, fmt)))
    for (size, fmt), v in rows.items():
        L = _levels(size[0])
        say(f"  1. {W}x{H} -> {size[0]}x{size[1]} {YUV_NAMES[fmt]}, L = {L}")
        say(f"     {L + 1} x BlitFramebuffer + WrhipGrabTextureYuv   " + "  ".join(f"{us:8.1f}" for us in v["chain"]))
        say("     WrhipGrabTextureYuvScaled                  " + "  ".join(f"{us:8.1f}" for us in v["fused"]) + "     launches, hipEvents: " + "  ".join(f"{us:7.1f}" for us in v["ev"]))
    # 2. the ladder: one call with three renditions against three calls with one
    lad = {}
    for rnd in range(ROUNDS):
        for fmt in fmts:
            lad.setdefault(fmt, {"one": [], "three": [], "ev1": [], "ev3": []})
            lad[fmt]["one"].append(timed(lambda: fused(sizes[2], fmt, 3)))

            def three():
                fused(sizes[0], fmt)
                fused(sizes[1], fmt)
                return fused(sizes[2], fmt)
            lad[fmt]["three"].append(timed(three))
            lad[fmt]["ev1"].append(events(lambda: fused(sizes[2], fmt, 3)))
            lad[fmt]["ev3"].append(sum(events(lambda: fused(sz, fmt)) for sz in sizes))
    for fmt, v in lad.items():
        say(f"  2. ladder {W}x{H} -> {sizes[2][0]}x{sizes[2][1]}, renditions = 3 ({YUV_NAMES[fmt]}), against three calls of one rendition")
        say("     one call, three renditions      " + "  ".join(f"{us:8.1f}" for us in v["one"]) + "     launches, hipEvents: " + "  ".join(f"{us:7.1f}" for us in v["ev1"]))
        say("     three calls, one rendition each " + "  ".join(f"{us:8.1f}" for us in v["three"]) + "     launches, hipEvents: " + "  ".join(f"{us:7.1f}" for us in v["ev3"]))
        say("     ratio three / one, host clock   " + "  ".join(f"{b / a:8.2f}" for a, b in zip(v["one"], v["three"])) + "     hipEvents: " + "  ".join(f"{b / a:7.2f}" for a, b in zip(v["ev1"], v["ev3"])))
    # 3. the two routes for rendition 0: an odd out_h, without FLIP_ROWS (stored from LDS) and with it (scratch + wr_grab_yuv_kernel)
    odd = {"plain": [], "flipped": [], "ev_plain": [], "ev_flipped": []}
    rect, size = (0, 0, W, H - 2), (W // 2, (H - 2) // 2)
    for rnd in range(ROUNDS):
        for name, flags in (("plain", 0), ("flipped", glapi.GRAB_FLIP_ROWS)):
            odd[name].append(timed(lambda: fused(size, glapi.YUV_I420, 1, rect, flags)))
            odd["ev_" + name].append(events(lambda: fused(size, glapi.YUV_I420, 1, rect, flags)))
    say(f"  3. {rect[2]}x{rect[3]} -> {size[0]}x{size[1]} I420 (odd out_h)")
    say("     stored from LDS (no flip)              " + "  ".join(f"{us:8.1f}" for us in odd["plain"]) + "     launches, hipEvents: " + "  ".join(f"{us:7.1f}" for us in odd["ev_plain"]))
    say("     scratch + wr_grab_yuv_kernel (flipped) " + "  ".join(f"{us:8.1f}" for us in odd["flipped"]) + "     launches, hipEvents: " + "  ".join(f"{us:7.1f}" for us in odd["ev_flipped"]))
    w.close()


def section_yuv_scaled_stream(lib, frames):
    size = (W // 2, H // 2)
    say(f"## yuv_scaled stream: cfg2 {W}x{H} streamed as in `stream`, {frames} frames per region, frames/s; NV12 to the host, tickets fetched one frame late")
    rec, _ = record_scene(lib, scenes.make_workload("cfg2", width=W, height=H))
    p = ScenePlayer(lib, rec)
    gl = glapi.GL(lib)                          # (the same loaded library and current context as the player's)
    window = gl.WrhipGetFramebufferTexture(0)
    host = np.empty(W * H * 2, np.uint8)
    info = glapi.WrhipGrabInfo()

    def run(kind, n):
        prev = -1
        for k in range(n):
            p.rp.exec(rec.stream)
            t = -1
            if kind == "full-size NV12 grab":
                t = gl.grab_texture_yuv(window, (0, 0, W, H), glapi.YUV_NV12, glapi.YUV_REC709_NARROW)
            elif kind != "no grab":
                t = gl.grab_texture_yuv_scaled(window, (0, 0, W, H), size, glapi.YUV_NV12, glapi.YUV_REC709_NARROW)
            if prev >= 0:
                assert gl.WrhipGrabResultGet(prev, C.byref(info), host.ctypes.data, 0, 1) == 0
            prev = t
        if prev >= 0:
            assert gl.WrhipGrabResultGet(prev, C.byref(info), host.ctypes.data, 0, 1) == 0
        gl.Finish()
    kinds = ["no grab", "full-size NV12 grab", f"scaled NV12 grab {size[0]}x{size[1]}"]
    rows, carried, crossed = {}, {}, {}
    for k in kinds:
        run(k, 4)
    for rnd in range(ROUNDS):
        for k in kinds:
            gl.WrhipResetStats()
            t0 = time.perf_counter()
            run(k, frames)
            dt = time.perf_counter() - t0
            st = gl.stats()
            rows.setdefault(k, []).append(frames / dt)
            carried[k] = (st["setup_carried"], frames)
            crossed[k] = st["d2h_bytes"] / frames
    for k in kinds:
        say(f"  {k:28s} " + "  ".join(f"{v:9.1f}" for v in rows[k]) + f"   frames/s   (setup_carried {carried[k][0]} of {carried[k][1]} flushes; {crossed[k] / 1e6:.2f} MB per frame crossed)")


# yuv_delta: what changes between two grabs -- nothing, everything (GRAB_KEY), or a square of noise that moves by a block a frame
YUVD_CONTENTS = [("static", 0), ("keyframe", -1), ("moving 256x256", 256), ("moving 1024x1024", 1024)]


def _yuvd_patches(side):
    rng = np.random.default_rng(side)
    return [rng.integers(0, 256, (side, side, 4), dtype=np.uint8) for _ in range(2)]


def _yuvd_move(upload, patches, side, k):
    """Frame k's change: the square, one of two noises alternately, a block further along a diagonal that wraps"""
    upload((64 * k) % (W - side), (64 * k) % (H - side), patches[k & 1])


def section_yuv_delta_kernel(lib):
    say(f"## yuv_delta: wr_grab_yuv_delta_kernel beside wr_grab_yuv_kernel, {W}x{H} RGBA8 window of cfg2, Rec709Narrow, host sink, hipEvents, us per launch")
    w = Window(lib, "cfg2")
    gl = w.gl
    info = glapi.WrhipGrabInfo()
    n = 30

    def full(fmt):
        t = gl.grab_texture_yuv(w.tex, None, fmt, glapi.YUV_REC709_NARROW)
        assert t >= 0 and gl.WrhipGrabResultGet(t, C.byref(info), None, 0, 1) == 0

    def delta(fmt, key):
        t = gl.grab_texture_yuv_delta(w.tex, None, fmt, glapi.YUV_REC709_NARROW, key=key)
        assert t >= 0 and gl.WrhipGrabResultGet(t, C.byref(info), None, 0, 1) == 0
        return info.blocks, int(info.bytes)
    rows, sent = {}, {}
    gl.WrhipSetProfiling(1)
    for fmt in (glapi.YUV_I420, glapi.YUV_NV12):
        for _ in range(4):
            full(fmt)
            delta(fmt, True)
        for rnd in range(ROUNDS):
            for name, side in [("full grab", None)] + YUVD_CONTENTS:
                patches = _yuvd_patches(side) if side and side > 0 else None
                delta(fmt, True)
                gl.WrhipResetStats()
                blocks = nbytes = 0
                for k in range(n):
                    if patches:
                        _yuvd_move(w.upload, patches, side, k)
                    if side is None:
                        full(fmt)
                    else:
                        b, by = delta(fmt, side == -1)
                        blocks += b
                        nbytes += by
                ks = [k for k in kernel_stats(gl, 15) if k.feat == (5 if side is None else 6)]
                assert len(ks) == 1 and ks[0].launches == n, [(k.feat, k.launches) for k in ks]
                rows.setdefault((fmt, name), []).append(ks[0].ns / n / 1e3)
                sent[(fmt, name)] = (blocks / n, nbytes / n, ks[0].algo_bytes // n)
    gl.WrhipSetProfiling(0)
    for (fmt, name), v in rows.items():
        b, by, algo = sent[(fmt, name)]
        say(f"  {YUV_NAMES[fmt]} {name:18s} " + "  ".join(f"{us:8.1f}" for us in v) + f"   us   ({algo / 1e6:6.1f} MB counted at the launch" +
            (f"; {b:7.1f} blocks, {by / 1e6:6.3f} MB crossed per grab)" if name != "full grab" else ")"))
    for fmt in (glapi.YUV_I420, glapi.YUV_NV12):
        s, f = rows[(fmt, "static")], rows[(fmt, "full grab")]
        say(f"  {YUV_NAMES[fmt]} static / full grab: " + "  ".join(f"{a / b if b else float('nan'):6.2f}" for a, b in zip(s, f)))
    w.close()


def section_yuv_delta_stream(lib, frames):
    say(f"## yuv_delta stream: cfg2 {W}x{H} streamed as in `stream`, {frames} frames per line, frames/s; I420 host sink, tickets fetched one frame late."
        "  The moving square is a TexSubImage2D into the window behind the frame: a write that sends the held-back launches, so each content has its own `no grab`.")
    rec, _ = record_scene(lib, scenes.make_workload("cfg2", width=W, height=H))
    p = ScenePlayer(lib, rec)
    gl = glapi.GL(lib)                          # (the same loaded library and current context as the player's)
    window = gl.WrhipGetFramebufferTexture(0)
    payload = W * H + 2 * ((W + 1) // 2) * ((H + 1) // 2)
    host = np.zeros(payload, np.uint8)
    info = glapi.WrhipGrabInfo()

    def upload(x, y, px):
        gl.ActiveTexture(G.GL_TEXTURE0)
        gl.BindTexture(G.GL_TEXTURE_2D, window)
        gl.TexSubImage2D(G.GL_TEXTURE_2D, 0, x, y, px.shape[1], px.shape[0], G.GL_BGRA, G.GL_UNSIGNED_BYTE, np.ascontiguousarray(px))

    def run(kind, side, n):
        patches = _yuvd_patches(side) if side > 0 else None
        prev = -1
        for k in range(n):
            p.rp.exec(rec.stream)
            if patches:
                _yuvd_move(upload, patches, side, k)
            t = -1
            if kind == "full I420 grab":
                t = gl.grab_texture_yuv(window, (0, 0, W, H), glapi.YUV_I420, glapi.YUV_REC709_NARROW)
            elif kind == "delta I420 grab":
                t = gl.grab_texture_yuv_delta(window, (0, 0, W, H), glapi.YUV_I420, glapi.YUV_REC709_NARROW, key=side == -1)
            if prev >= 0:
                assert gl.WrhipGrabResultGet(prev, C.byref(info), host.ctypes.data, 0, 1) == 0
            prev = t
        if prev >= 0:
            assert gl.WrhipGrabResultGet(prev, C.byref(info), host.ctypes.data, 0, 1) == 0
        gl.Finish()
    kinds = ["no grab", "full I420 grab", "delta I420 grab"]
    cases = [(name, side, k) for name, side in YUVD_CONTENTS for k in kinds if not (name == "keyframe" and k != "delta I420 grab")]
    rows, extra = {}, {}
    for name, side, k in cases:
        run(k, side, 4)
    for rnd in range(ROUNDS):
        for name, side, k in cases:
            gl.WrhipResetStats()
            t0 = time.perf_counter()
            run(k, side, frames)
            dt = time.perf_counter() - t0
            st = gl.stats()
            rows.setdefault((name, k), []).append(frames / dt)
            extra[(name, k)] = (st["setup_carried"], st["d2h_bytes"] / frames)
    for (name, k), v in rows.items():
        say(f"  {name:18s} {k:16s} " + "  ".join(f"{x:9.1f}" for x in v) + f"   frames/s   (setup_carried {extra[(name, k)][0]} of {frames} flushes; {extra[(name, k)][1] / 1e6:.6f} MB per frame crossed)")
    say(f"  (a full I420 payload is {payload / 1e6:.2f} MB; a static delta grab crosses 16 bytes)")


# ---- scroll grabs (WRHIP_GRAB_SCROLL) ----------------------------------------------------------------------
SCROLL_CASES = ("nothing changed", "40 blocks changed", "scroll by 37", "scroll by 37, 40 blocks changed")


def _scroll_frame(w, page, case, k, some, patches):
    """Frame k of a case: the window shows rows [37 * k, 37 * k + H) of the page when the case scrolls; 40 blocks get a 16 x 16 patch"""
    gl = w.gl
    if case.startswith("scroll"):
        w.upload(0, 0, page[37 * k:37 * k + H])
    if case.endswith("40 blocks changed"):
        for b in some:
            w.upload(int(b % (W // 64)) * 64 + 5, int(b // (W // 64)) * 64 + 3, patches[k & 1])
    gl.WrhipFlush()


def section_scroll_kernel(lib, only=None, n=10):
    """(a): every case with DELTA | PACKED | SCROLL and with DELTA | PACKED on the same frames; `only`: that case alone, with the scroll
    grab alone and no event profiling -- for a kernel trace by a profiler, which gives the four launches one by one"""
    say(f"## scroll: {W}x{H} RGBA8 window onto a page of noise, {n} grabs per case, hipEvents (WrhipSetProfiling(1)), us per grab (all its launches)")
    w = Window(lib)
    gl = w.gl
    DP = glapi.GRAB_DELTA | glapi.GRAB_PACKED
    DPS = DP | glapi.GRAB_SCROLL
    rng = np.random.default_rng(3)
    page = rng.integers(0, 256, (H + 37 * n, W, 4), dtype=np.uint8)
    nblocks = ((W + 63) // 64) * ((H + 63) // 64)
    some = rng.choice(nblocks, size=40, replace=False)
    patches = [rng.integers(0, 256, (16, 16, 4), dtype=np.uint8) for _ in range(2)]
    rows = {}
    for rnd in range(1 if only else ROUNDS):
        for case in SCROLL_CASES:
            if only and case != only:
                continue
            for name, flags in (("scroll", DPS), ("packed", DP)):
                if only and name != "scroll":
                    continue
                w.upload(0, 0, page[:H])
                for b in some:          # (the patched places hold a patch from the start: every frame changes exactly these blocks)
                    w.upload(int(b % (W // 64)) * 64 + 5, int(b // (W // 64)) * 64 + 3, patches[1])
                w.grab(flags | glapi.GRAB_KEY)
                w.grab(flags)           # (untimed: code objects, the work memory)
                gl.WrhipSetProfiling(0 if only else 1)
                gl.WrhipResetStats()
                infos = []
                for k in range(1, n + 1):
                    _scroll_frame(w, page, case, k, some, patches)
                    infos.append(w.grab(flags))
                ks = kernel_stats(gl, 15)
                gl.WrhipSetProfiling(0)
                if only:
                    continue
                feat = 8 if flags & glapi.GRAB_SCROLL else 2
                assert len(ks) == 1 and ks[0].launches == n and ks[0].feat == feat, [(k.kind, k.feat, k.launches) for k in ks]
                last = infos[-1]
                rows.setdefault((case, name), []).append((ks[0].ns / n / 1e3, int(last.blocks), int(last.copied), int(last.bytes), int(last.scroll_dy)))
    for (case, name), v in rows.items():
        say(f"  {case:32s} {name:7s} " + "  ".join(f"{us:8.1f}" for us, _, _, _, _ in v) +
            f"   us   (scroll_dy {v[0][4]}; entries {v[0][1]} of {nblocks}, {v[0][2]} of them COPY; {v[0][3]} bytes crossed)")
    w.close()


def section_scroll_stream(lib, frames):
    say(f"## scroll stream: {frames} frames, each the page scrolled by 37 (one TexSubImage2D of the window per frame), one grab per frame patched into the caller's image, frames/s")
    w = Window(lib)
    gl = w.gl
    DP = glapi.GRAB_DELTA | glapi.GRAB_PACKED
    page = np.random.default_rng(4).integers(0, 256, (H + 37 * frames, W, 4), dtype=np.uint8)
    host = np.zeros((H, W, 4), np.uint8)
    info = glapi.WrhipGrabInfo()

    def run(flags, n):
        waiting, crossed = [], []

        def fetch(wait):
            while waiting:
                rc = gl.WrhipGrabResultGet(waiting[0], C.byref(info), host.ctypes.data, 0, 1 if wait else 0)
                if rc == 1:
                    return
                assert rc == 0 and info.status == 0, (rc, info.status)
                waiting.pop(0)
                crossed.append(int(info.bytes))
                wait = False
        w.upload(0, 0, page[:H])
        if flags is not None:
            assert gl.WrhipGrabResultGet(gl.grab_texture(w.tex, None, flags | glapi.GRAB_KEY), C.byref(info), host.ctypes.data, 0, 1) == 0
        gl.Finish()
        t0 = time.perf_counter()
        for k in range(1, n + 1):
            w.upload(0, 0, page[37 * k:37 * k + H])
            if flags is not None:
                if len(waiting) == 8:
                    fetch(True)
                t = gl.grab_texture(w.tex, None, flags)
                assert t >= 0
                waiting.append(t)
                fetch(False)
        gl.Finish()
        while waiting:
            fetch(True)
        dt = time.perf_counter() - t0
        assert flags is None or np.array_equal(host, page[37 * n:37 * n + H]), "the patched image is not the window"
        return n / dt, float(np.mean(crossed)) if crossed else 0.0
    modes = {"no grab": None, "packed delta grab": DP, "scroll grab": DP | glapi.GRAB_SCROLL}
    for flags in modes.values():
        run(flags, 10)
    rows = {}
    for rnd in range(ROUNDS):
        for name, flags in modes.items():
            rows.setdefault(name, []).append(run(flags, frames))
    for name, v in rows.items():
        say(f"  {name:22s} " + "  ".join(f"{fps:9.1f}" for fps, _ in v) + "   frames/s   " + (f"({v[0][1] / 1e6:8.3f} MB per frame crossed)" if v[0][1] else ""))


# ---- scroll-aware delta YUV grabs (WrhipGrabTextureYuvDelta with GRAB_SCROLL) -----------------------------
YUVSCROLL_CASES = ("scroll by 64", "nothing changed", "40 blocks changed")


def _yuv_delta_grab(w, scroll, dst=0, nbytes=0, key=False, wait=True):
    t = w.gl.grab_texture_yuv_delta(w.tex, None, glapi.YUV_I420, glapi.YUV_REC709_NARROW, dst=dst or None, dst_bytes=nbytes if dst else 0, key=key, scroll=scroll)
    assert t >= 0, w.gl.GetError()
    info = glapi.WrhipGrabInfo()
    if wait:
        assert w.gl.WrhipGrabResultGet(t, C.byref(info), None, 0, 1) == 0
        return info
    return t


def section_yuvscroll_kernel(lib, n=10):
    """Every case with and without GRAB_SCROLL on the same frames, host sink, I420: us per grab (all its launches), and what crossed"""
    say(f"## yuvscroll: {W}x{H} window onto a page of noise, I420, host sink, {n} grabs per case, hipEvents (WrhipSetProfiling(1)), us per grab (all its launches)")
    w = Window(lib)
    gl = w.gl
    rng = np.random.default_rng(5)
    page = rng.integers(0, 256, (H + 64 * n, W, 4), dtype=np.uint8)
    nblocks = ((W + 63) // 64) * ((H + 63) // 64)
    some = rng.choice(nblocks, size=40, replace=False)
    patches = [rng.integers(0, 256, (16, 16, 4), dtype=np.uint8) for _ in range(2)]
    rows = {}
    for rnd in range(ROUNDS):
        for case in YUVSCROLL_CASES:
            for name, scroll in (("scroll", True), ("plain", False)):
                w.upload(0, 0, page[:H])
                for b in some:
                    w.upload(int(b % (W // 64)) * 64 + 5, int(b // (W // 64)) * 64 + 3, patches[1])
                _yuv_delta_grab(w, scroll, key=True)
                _yuv_delta_grab(w, scroll)          # (untimed: code objects, the second planes, the work memory)
                gl.WrhipSetProfiling(1)
                gl.WrhipResetStats()
                infos = []
                for k in range(1, n + 1):
                    if case.startswith("scroll"):
                        w.upload(0, 0, page[64 * k:64 * k + H])
                    if case.startswith("40"):
                        for b in some:
                            w.upload(int(b % (W // 64)) * 64 + 5, int(b // (W // 64)) * 64 + 3, patches[k & 1])
                    gl.WrhipFlush()
                    infos.append(_yuv_delta_grab(w, scroll))
                ks = kernel_stats(gl, 15)
                gl.WrhipSetProfiling(0)
                assert len(ks) == 1 and ks[0].launches == n and ks[0].feat == (9 if scroll else 6), [(k.kind, k.feat, k.launches) for k in ks]
                last = infos[-1]
                rows.setdefault((case, name), []).append((ks[0].ns / n / 1e3, int(last.blocks), int(last.copied), int(last.bytes), int(last.scroll_dy)))
    for (case, name), v in rows.items():
        say(f"  {case:20s} {name:7s} " + "  ".join(f"{us:8.1f}" for us, _, _, _, _ in v) +
            f"   us   (scroll_dy {v[0][4]}; entries {v[0][1]} of {nblocks}, {v[0][2]} of them COPY; {v[0][3]} bytes crossed)")
    w.close()


def section_yuvscroll_stream(lib, frames):
    say(f"## yuvscroll stream: {frames} frames, each the page scrolled by 64 (one TexSubImage2D of the window per frame), one I420 delta grab per frame, frames/s")
    w = Window(lib)
    gl = w.gl
    page = np.random.default_rng(6).integers(0, 256, (H + 64 * frames, W, 4), dtype=np.uint8)
    nbytes = W * H * 3 // 2
    host = np.zeros(nbytes, np.uint8)
    dev = gl.device_alloc(nbytes)
    info = glapi.WrhipGrabInfo()

    def run(mode, n):
        waiting, crossed = [], []

        def fetch(wait):
            while waiting:
                rc = gl.WrhipGrabResultGet(waiting[0], C.byref(info), host.ctypes.data, 0, 1 if wait else 0)
                if rc == 1:
                    return
                assert rc == 0 and info.status == 0, (rc, info.status)
                waiting.pop(0)
                crossed.append(int(info.bytes))
                wait = False
        w.upload(0, 0, page[:H])
        if mode is not None:
            scroll, device = mode
            _yuv_delta_grab(w, scroll, dev if device else 0, nbytes, key=True)
        gl.Finish()
        t0 = time.perf_counter()
        for k in range(1, n + 1):
            w.upload(0, 0, page[64 * k:64 * k + H])
            if mode is not None:
                if len(waiting) == 8:
                    fetch(True)
                waiting.append(_yuv_delta_grab(w, scroll, dev if device else 0, nbytes, wait=False))
                fetch(False)
        gl.Finish()
        while waiting:
            fetch(True)
        return n / (time.perf_counter() - t0), float(np.mean(crossed)) if crossed else 0.0
    modes = {"no grab": None, "plain delta, host": (False, False), "scroll delta, host": (True, False), "plain delta, device": (False, True), "scroll delta, device": (True, True)}
    for mode in modes.values():
        run(mode, 10)
    rows = {}
    for rnd in range(ROUNDS):
        for name, mode in modes.items():
            rows.setdefault(name, []).append(run(mode, frames))
    for name, v in rows.items():
        say(f"  {name:22s} " + "  ".join(f"{fps:9.1f}" for fps, _ in v) + "   frames/s   " + (f"({v[0][1] / 1e6:8.3f} MB per frame crossed)" if v[0][1] else ""))
    gl.device_free(dev)
    w.close()


# ---- payload puts (WrhipPutTexturePayload) ----------------------------------------------------------------
class Mirror:
    """A 4K window and a second RGBA8 texture of its size in one context; payloads are fetched into and put from one buffer, and the
    parent path -- WrhipGrabDecode into a host image, TexSubImage2D of the damage rect -- runs on the same payloads"""

    def __init__(self, lib, content="noise"):
        self.w = Window(lib, content)
        gl = self.gl = self.w.gl
        self.tex = self.w.r.device.create_texture(W, H, G.GL_RGBA8, render_target=True)
        self.buf = C.create_string_buffer(16 + ((W + 63) // 64) * ((H + 63) // 64) * (16 + 64 * 64 * 4))
        self.img = np.zeros((H, W, 4), np.uint8)
        self.rect = (C.c_int32 * 4)(0, 0, W, H)
        self.damage, self.blocks, self.n = (C.c_int32 * 4)(), C.c_uint32(0), C.c_uint64(0)
        self.set_both(np.zeros((H, W, 4), np.uint8))

    def set_both(self, px):
        """the mirror texture and the host image hold `px` (a frame a payload is a delta against)"""
        self.img[...] = px
        self.upload_mirror(0, 0, W, H)
        self.gl.Finish()

    def upload_mirror(self, x, y, w, h):
        gl = self.gl
        gl.ActiveTexture(G.GL_TEXTURE0)
        gl.BindTexture(G.GL_TEXTURE_2D, self.tex.id)
        gl.PixelStorei(G.GL_UNPACK_ROW_LENGTH, W)
        gl.TexSubImage2D(G.GL_TEXTURE_2D, 0, x, y, w, h, G.GL_BGRA, G.GL_UNSIGNED_BYTE, self.img.ctypes.data + (y * W + x) * 4)
        gl.PixelStorei(G.GL_UNPACK_ROW_LENGTH, 0)

    def grab_payload(self, flags):
        """A grab of the window, its payload in self.buf: -> bytes"""
        t = self.gl.grab_texture(self.w.tex, None, flags)
        assert t >= 0, self.gl.GetError()
        assert self.gl.WrhipGrabPayloadGet(t, self.buf, len(self.buf), C.byref(self.n), 1) == 0
        return int(self.n.value)

    def put(self, nbytes, flags):
        assert self.gl.WrhipPutTexturePayload(self.tex.id, C.addressof(self.rect), self.buf, nbytes, flags) == 0, self.gl.GetError()

    def parent(self, nbytes, flags):
        """-> the bytes TexSubImage2D carries"""
        assert self.gl.WrhipGrabDecode(self.buf, nbytes, G.GL_RGBA8, flags, W, H, self.img.ctypes.data, 0, self.damage, C.byref(self.blocks)) == 0
        x, y, w, h = self.damage
        if w and h:
            self.upload_mirror(x, y, w, h)
        return w * h * 4

    def mirror_pixels(self):
        return self.w.r.device.read_texture(self.tex)

    def close(self):
        self.w.close()


def section_mirror_put(lib, n=10):
    say(f"## mirror: WrhipPutTexturePayload into a {W}x{H} RGBA8 texture, {n} puts of one payload per line; hipEvents (WrhipSetProfiling(1)) us per put: COPY pass "
        "(wr_put_copy_kernel) + patch pass (wr_put_patch_kernel); host clock us per put, n puts and one Finish, beside the parent path on the same payload "
        "(WrhipGrabDecode into a host image, TexSubImage2D of the damage rect)")
    DP = glapi.GRAB_DELTA | glapi.GRAB_PACKED
    DPS = DP | glapi.GRAB_SCROLL
    rng = np.random.default_rng(3)
    nblocks = ((W + 63) // 64) * ((H + 63) // 64)
    some = rng.choice(nblocks, size=40, replace=False)
    patch = rng.integers(0, 256, (16, 16, 4), dtype=np.uint8)
    page = rng.integers(0, 256, (H + 37, W, 4), dtype=np.uint8)
    cases = ("packed keyframe of cfg2", "40 of %d blocks changed" % nblocks, "noise keyframe (all RAW)", "scroll by 37")
    rows = {}
    for rnd in range(ROUNDS):
        for case in cases:
            m = Mirror(lib, "cfg2" if case.startswith("packed") else "noise")
            gl = m.gl
            flags = DPS if case.startswith("scroll") else DP
            if case.startswith("scroll"):
                m.w.upload(0, 0, page[:H])
            before = np.zeros((H, W, 4), np.uint8)
            if not case.endswith("keyframe of cfg2") and not case.startswith("noise"):
                # (a delta: the mirror and the host image hold the frame the payload is a delta against)
                key = m.grab_payload(flags | glapi.GRAB_KEY)
                m.parent(key, flags)
                before = m.img.copy()
                if case.startswith("scroll"):
                    m.w.upload(0, 0, page[37:37 + H])
                else:
                    for b in some:
                        m.w.upload(int(b % (W // 64)) * 64 + 5, int(b // (W // 64)) * 64 + 3, patch)
            nbytes = m.grab_payload(flags | (glapi.GRAB_KEY if "keyframe" in case else 0))
            entries = gl.grab_decode(m.buf.raw[:nbytes], G.GL_RGBA8, flags, np.zeros((H, W, 4), np.uint8) if "keyframe" in case else before.copy())[1]
            # once each, checked against the other: the put's texture is the parent path's image
            m.set_both(before)
            m.put(nbytes, flags)
            want = before.copy()
            gl.grab_decode(m.buf.raw[:nbytes], G.GL_RGBA8, flags, want)
            assert np.array_equal(m.mirror_pixels(), want), f"{case}: the put's texture is not WrhipGrabDecode's image"
            gl.Finish()
            # the put: events, then the host clock
            gl.WrhipSetProfiling(1)
            gl.WrhipResetStats()
            for _ in range(n):
                m.put(nbytes, flags)
            gl.Finish()
            ks = {k.feat: k.ns / n / 1e3 for k in kernel_stats(gl, 16)}
            staged = gl.stats()["h2d_bytes"] / n
            gl.WrhipSetProfiling(0)
            t0 = time.perf_counter()
            for _ in range(n):
                m.put(nbytes, flags)
            gl.Finish()
            t_put = (time.perf_counter() - t0) / n * 1e6
            t0 = time.perf_counter()
            for _ in range(n):
                up = m.parent(nbytes, flags)
            gl.Finish()
            t_parent = (time.perf_counter() - t0) / n * 1e6
            rows.setdefault(case, []).append((ks.get(2, 0.0), ks.get(1, 0.0), t_put, t_parent, int(staged), up, entries, nbytes))
            m.close()
    for case, v in rows.items():
        say(f"  {case:28s} events: copy " + " ".join(f"{r[0]:7.1f}" for r in v) + "  patch " + " ".join(f"{r[1]:7.1f}" for r in v) +
            "   host clock: put " + " ".join(f"{r[2]:8.1f}" for r in v) + "  parent " + " ".join(f"{r[3]:9.1f}" for r in v) +
            f"   us   ({v[0][6]} entries; payload {v[0][7]} bytes; staged {v[0][4]} bytes per put; the parent path uploads {v[0][5]} bytes)")


def section_mirror_stream(lib, frames):
    say(f"## mirror stream: {frames} frames mirrored into a second {W}x{H} texture, no Finish in the loop: a grab per frame, its payload fetched, then the payload put, "
        "or the parent path (WrhipGrabDecode into a host image, TexSubImage2D of the damage rect); frames/s and bytes per frame to the host / back to the device")
    DP = glapi.GRAB_DELTA | glapi.GRAB_PACKED
    page = np.random.default_rng(4).integers(0, 256, (H + 37 * frames, W, 4), dtype=np.uint8)
    cfg2 = []

    def run(m, case, kind, n):
        gl = m.gl
        flags = DP | glapi.GRAB_SCROLL if case == "scroll by 37" else DP
        if case == "scroll by 37":
            m.w.upload(0, 0, page[:H])
        else:
            m.w.upload(0, 0, cfg2[0])
        key = m.grab_payload(flags | glapi.GRAB_KEY)
        m.parent(key, flags)                   # (both start from the mirror and the host image of frame 0)
        gl.Finish()
        gl.WrhipResetStats()
        down = up = 0
        t0 = time.perf_counter()
        for k in range(1, n + 1):
            m.w.upload(0, 0, page[37 * k:37 * k + H] if case == "scroll by 37" else cfg2[k % len(cfg2)])
            nbytes = m.grab_payload(flags)
            down += nbytes
            if kind == "put":
                m.put(nbytes, flags)
            else:
                up += m.parent(nbytes, flags)
        gl.Finish()
        dt = time.perf_counter() - t0
        if kind == "put":
            up = gl.stats()["h2d_bytes"] - n * W * H * 4      # (without the frames' own uploads of the window)
        want = page[37 * n:37 * n + H] if case == "scroll by 37" else cfg2[n % len(cfg2)]
        assert np.array_equal(m.mirror_pixels(), want), f"{case}, {kind}: the mirror is not the window"
        return n / dt, down / n, up / n
    # the "every block changes" frames: cfg2 of four seeds, rendered once each and read back; the stream uploads them in turn
    w = Window(lib, "cfg2")
    for sd in (1, 2, 3, 4):
        w.r.render(scenes.make_workload("cfg2", width=W, height=H, seed=sd))
        w.r.finish()
        cfg2.append(w.r.device.read_texture(glapi_window_texture(w)).copy())
    w.close()
    rows = {}
    m = Mirror(lib)
    for case in ("scroll by 37", "cfg2 of seeds 1..4 in turn"):
        for kind in ("put", "parent"):
            run(m, case, kind, 5)
    for rnd in range(ROUNDS):
        for case in ("scroll by 37", "cfg2 of seeds 1..4 in turn"):
            for kind in ("put", "parent"):
                rows.setdefault((case, kind), []).append(run(m, case, kind, frames))
    m.close()
    for (case, kind), v in rows.items():
        say(f"  {case:28s} {kind:7s} " + "  ".join(f"{fps:8.1f}" for fps, _, _ in v) + f"   frames/s   ({v[0][1] / 1e6:8.3f} MB per frame to the host, {v[0][2] / 1e6:8.3f} MB back to the device)")
    say(f"  (every frame also uploads the window itself, {W * H * 4 / 1e6:.1f} MB, in both loops: the source of the stream, not part of either path)")


def glapi_window_texture(w):
    from webrender_amd.device import Texture
    return Texture(0, W, H, G.GL_RGBA8, fbo=0)


def section_ab(other, steps, warmup):
    say(f"## ab: bench.py --gpus 1 --steps {steps} --warmup {warmup} (cfg2), this library against {os.path.basename(other)}, alternated, frames/s")
    rows = {"parent": [], "this": []}
    for rnd in range(ROUNDS):
        for name in ("parent", "this"):
            env = dict(os.environ)
            if name == "parent":
                env["WRHIP_LIB_PATH"] = os.path.abspath(other)
            else:
                env.pop("WRHIP_LIB_PATH", None)
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                                 env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
            if out.returncode != 0:
                say(f"  {name}: bench.py exited with {out.returncode}: {out.stderr[-400:]}")
                return
            res = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")][-1]
            rows[name].append(float(res["value"]))
            print(f"  ({name}, round {rnd}: {res['value']})", file=sys.stderr, flush=True)
    for name, v in rows.items():
        say(f"  {name:8s} " + "  ".join(f"{x:10.1f}" for x in v) + f"   {res.get('unit', '')}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="pack,transport,stream")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--ab", default=None, metavar="LIB", help="another build of libwrhip.so to run bench.py against")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", default=None, metavar="WxH", help="another window size (the figures of DESIGN.md are for the default, 3840x2160)")
    ap.add_argument("--scroll-case", default=None, choices=SCROLL_CASES, help="section scroll: this case's scroll grabs alone, unprofiled (for a profiler's kernel trace)")
    args = ap.parse_args()
    global ROUNDS, W, H
    ROUNDS = args.rounds
    if args.size:
        W, H = (int(v) for v in args.size.split("x"))
    lib = glapi.wrhip_path()
    if "tensor" in args.sections:
        import torch                            # (torch brings its own HIP runtime: it has to initialise the device before libwrhip does)
        torch.cuda.init()
    w = Window(lib)
    say(f"# grab_bench: {w.gl.WrhipDeviceName().decode() if w.gl.WrhipDeviceName() else 'no device'}; {ROUNDS} alternated rounds per line")
    w.close()
    try:
        for s in args.sections.split(","):
            if s == "pack":
                section_pack(lib, "noise")
                section_pack(lib, "cfg2")
            elif s == "transport":
                section_transport(lib)
            elif s == "stream":
                section_stream(lib, args.frames)
            elif s == "scaled":
                section_scaled(lib, "noise")
                section_scaled(lib, "cfg2")
                section_scaled_stream(lib, args.frames)
            elif s == "tensor":
                section_tensor_kernel(lib, "noise")
                section_tensor_kernel(lib, "cfg2")
                section_tensor_scaled(lib)
                section_tensor_stream(lib, args.frames)
                if args.ab:
                    section_tensor_parent(args.ab, args.frames)
            elif s == "put":
                section_tensor_kernel(lib, "noise")      # (the rate beside: the same bytes the other way)
                section_put(lib)
                section_put_stream(lib, args.frames)
            elif s == "yuv":
                section_yuv_kernel(lib, "noise")
                section_yuv_kernel(lib, "cfg2")
                section_yuv_stream(lib, args.frames)
            elif s == "yuv_delta":
                section_yuv_delta_kernel(lib)
                section_yuv_delta_stream(lib, args.frames)
            elif s == "yuv_scaled":
                section_yuv_scaled(lib)
                section_yuv_scaled_stream(lib, args.frames)
            elif s == "yuvscroll":
                section_yuvscroll_kernel(lib)
                section_yuvscroll_stream(lib, args.frames)
            elif s == "scroll":
                section_scroll_kernel(lib, only=args.scroll_case)
                if not args.scroll_case:
                    section_scroll_stream(lib, args.frames)
            elif s == "mirror":
                section_mirror_put(lib)
                section_mirror_stream(lib, args.frames)
            elif s == "tensor_parent":        # (run by `tensor` with WRHIP_LIB_PATH set: the parent path alone, on that library)
                section_tensor_scaled(lib, with_tensor=False)
                section_tensor_stream(lib, args.frames, with_tensor=False)
        if args.ab:
            section_ab(args.ab, args.steps, args.warmup)
    finally:
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
