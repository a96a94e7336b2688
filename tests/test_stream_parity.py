"""Frames streamed back to back with nothing that drains libwrhip's held-back raster launches in between (harness.render_streamed):
the path of a frame loop and of bench.py, where every flush's upload scatter and setup stage ride in the first workgroups of a raster
launch the flush before held back (Context::Tail, fuse_at in flush_work).  Host simulation against the oracle, byte for byte; the
same sequences run on the MI355X in tests/test_gpu_parity.py."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest
from conftest import ROOT
from stream_cases import GROWTH, UPLOAD_CARRY, NEW_STATIC, MENU, random_sequences, carriers_expected, check_streamed, W
from webrender_amd import scenes
from webrender_amd.harness import render_direct, render_streamed


@pytest.mark.parametrize("name,make", GROWTH, ids=[g[0] for g in GROWTH])
def test_streamed_growth_behind_held_tail(hostsim, oracle_gcc, name, make):
    """The last flush outgrows one buffer of its scratch set while the flush before has its raster launches held back: the buffer is
    replaced, and the flush's setup stage and upload scatter still go out -- in the held-back launch it planned to use."""
    frames = make()
    st = check_streamed(hostsim, oracle_gcc, frames)
    _, before = render_streamed(hostsim, frames[:-1])
    assert st["scratch_grown_held"] > before["scratch_grown_held"], f"{name}: the last flush grew no scratch buffer behind a held-back launch"


def test_streamed_masks_growth_repro(hostsim, oracle_gcc):
    """The reproduction of the lost setup stage: cfg2 rects, 64, 64 and 129 of them -- the third flush fits its prims (129 of 130) and
    not its coverage masks (384 words of 258).  When the masks were grown after the carrier was chosen, the growth launched the
    held-back launches on their own, the setup stage never ran and the deferred scatter was dropped: every byte of the window differed."""
    frames = [scenes.cfg2_overlapping_rects(n=n, **W) for n in (64, 64, 129)]
    st = check_streamed(hostsim, oracle_gcc, frames)
    assert st["scratch_grown_held"] >= 1 and st["setup_carried"] >= 2, st


def test_streamed_upload_carry(hostsim, oracle_gcc):
    """The data textures (prim headers, GPU cache) grow and are uploaded whole by the last frame, in the scatter its carrier runs."""
    check_streamed(hostsim, oracle_gcc, UPLOAD_CARRY[1]())


def test_streamed_new_static_texture(hostsim, oracle_gcc):
    """The last frame uploads a static texture the backend has not seen (the image atlas) while the frame before is held back: a
    texture no pending draw uses is uploaded without draining the tail, and the atlas frame's setup stage is carried as well."""
    check_streamed(hostsim, oracle_gcc, NEW_STATIC[1]())


def test_streamed_setup_on_its_own_stream(hostsim):
    """WRHIP_SETUP_STREAM=1 (off by default; host simulation only): every flush behind a held-back tail runs its setup stage as a
    launch of its own on the second stream instead of in a held-back launch -- no setup stage is carried, and the window is the one
    the same frames give without the variable.  The variable is read when the context is created: it is in place from before that
    to after the last launch, and is then put back as it was found."""
    _, make = GROWTH[0]          # (the smallest streamed case: 64, 64 and 129 rects)
    want, _ = render_streamed(hostsim, make())
    saved = os.environ.get("WRHIP_SETUP_STREAM")
    os.environ["WRHIP_SETUP_STREAM"] = "1"
    try:
        got, st = render_streamed(hostsim, make())
    finally:
        if saved is None:
            os.environ.pop("WRHIP_SETUP_STREAM", None)
        else:
            os.environ["WRHIP_SETUP_STREAM"] = saved
    assert st["gl_error"] == 0, st
    assert st["setup_carried"] == 0, st
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes of the window differ; {st}"


def stream_driver(lib, mode, **env):
    e = dict(os.environ, **{k: str(v) for k, v in env.items()})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stream_driver.py"), lib, mode], env=e, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1]), p.stderr


def _digest(px):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(px).tobytes()).hexdigest()


@pytest.mark.parametrize("mode", ["readback", "wrap", "realloc"])
def test_recorded_draws_survive_early_batch_close(hostsim, oracle_gcc, mode):
    """Draws recorded while the open upload batch holds their data textures whole may read those in the staging mirror.  Here the
    batch is closed before the draws are flushed -- by a readback of another texture, by the ring wrapping, by the ring being
    reallocated for an upload larger than it -- and the ring is then lapped (1 MB ring): the draws must still see their data."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from stream_driver import frame_for
    want, _ = render_direct(oracle_gcc, frame_for(mode))
    got, _ = stream_driver(hostsim, mode, WRHIP_STAGING_BYTES=1 << 20)
    assert got["gl_error"] == 0, got
    assert got["digest"] == _digest(want), got


def test_pool_word_is_not_read_after_the_ring_reuses_it(hostsim, oracle_gcc):
    """Finish reads the last flush's pool allocation word, which lives in the staging mirror.  A gradient frame is flushed
    (WrhipFlush), then texture uploads with no draws lap a 1 MB ring with bytes that would read as a request for 64 M words: Finish
    must not take them for one (no growth message, no error), and the next frame is the oracle's."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from stream_driver import frame_for
    want, _ = render_direct(oracle_gcc, frame_for("pool"))
    got, err = stream_driver(hostsim, "pool", WRHIP_STAGING_BYTES=1 << 20)
    assert "pool ran out" not in err, err[-2000:]
    assert got["gl_error"] == 0, got
    assert got["digest"] == _digest(want), got


SWEEP = random_sequences(seed=2026, count=20)


@pytest.mark.parametrize("seq", SWEEP, ids=[f"s{i}" for i in range(len(SWEEP))])
def test_streamed_random_sequences(hostsim, oracle_gcc, seq):
    """Sequences of 4-10 frames from the pipelined sweep's menu (tests/sweep_pipelined.py), streamed; the last frame is checked."""
    check_streamed(hostsim, oracle_gcc, [MENU[i]() for i in seq], carried=carriers_expected(seq))
