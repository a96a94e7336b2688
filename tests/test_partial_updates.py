"""Partial tile updates: frames that redraw only the dirty rect of only the invalidated tiles over what the tiles kept from the frame
before, and a clear in the middle of a target -- tests/partial_update_cases.py has the sequences.  Every comparison is byte for byte
against the oracle, which executes each call at once: every frame's window (a tap against the digest of the oracle's window), the
final window and every tile read back after the last frame; GetError() == 0; the raster launches of every frame still held back.

Each sequence shows on the ORACLE's output alone that it is not vacuous: inside every dirty rect consecutive frames differ; outside it
the tile is the previous frame's, is not one colour, and is not what the oracle draws there when it renders the frame from scratch; a
dirty rect equal to the valid rect gives the from-scratch tile, one outside the valid rect leaves the tile as it was.

Which path of libwrhip ran is asserted from its statistics (row_launches, cell_bins, forwarded_targets, flushes), never how it
resolves anything.  Each case runs on the host simulation and, under -m gpu, on the MI355X."""
import numpy as np
import pytest
from conftest import wrhip_lib, oracle_ref
import frame_taps as ft
import hazard_cases as hz
import partial_update_cases as pu

_want = {}


def _words(px):
    return ft.stored_words(px)


def _region(px, r):
    return px[r[1]:r[3], r[0]:r[2]]


def _oracle(ref, name):
    """The oracle's run of a sequence, once per session, checked for what the sequence is meant to show"""
    if (ref, name) in _want:
        return _want[(ref, name)]
    q = pu.seq(name)
    want = pu.run(ref, name)
    assert int(want["gl_error"]) == 0
    n = len(q.frames)
    assert n >= 3
    seen = set()
    for k in range(1, n):
        scratch = pu.run_scratch(ref, name, k)
        assert not np.array_equal(want["frame%d" % (k - 1)], want["frame%d" % k]), f"{name}: the oracle's windows {k - 1} and {k} are alike"
        for ref_t in q.tiles:
            t = ref_t.name
            prev, cur, scr = (_words(want["frame%d/%s" % (k - 1, t)]), _words(want["frame%d/%s" % (k, t)]), _words(scratch[t]))
            rect = q.plan[k].get(t)
            task = q.task_rect(t, rect) if rect is not None else None
            if task is None:
                # left alone, or a dirty rect that misses the valid rect
                assert np.array_equal(cur, prev), f"{name} frame {k} {t}: changed although nothing of it was to be drawn"
                seen.add("untouched" if rect is None else "outside")
                continue
            assert not np.array_equal(_region(cur, task), _region(prev, task)), f"{name} frame {k} {t}: the redraw of {task} changes nothing"
            if rect == pu.FULL or tuple(rect) == q.valid[t]:
                # (not where the tile samples an off-screen target of which the frame redrew only a part)
                assert q.atlases or np.array_equal(cur, scr), f"{name} frame {k} {t}: a redraw of all that is valid is not the frame drawn from scratch"
                seen.add("valid")
                continue
            out = np.ones(cur.shape, bool)
            out[rect[1]:rect[3], rect[0]:rect[2]] = False
            assert np.array_equal(cur[out], prev[out]), f"{name} frame {k} {t}: the oracle changed pixels outside the dirty rect {rect}"
            assert len(np.unique(cur[out])) > 1, f"{name} frame {k} {t}: nothing was kept outside {rect} but one colour"
            assert not np.array_equal(cur[out], scr[out]), f"{name} frame {k} {t}: outside {rect} the kept pixels are what frame {k} draws there anyway"
            seen.add("partial")
    assert np.array_equal(want["window"], want["frame%d" % (n - 1)])
    want["seen"] = seen
    _want[(ref, name)] = want
    return want


def _sequence(lib, ref, name):
    """-> libwrhip's statistics after every frame (what a frame launched shows one frame later: its raster launches are held back) and
    after the Finish"""
    q = pu.seq(name)
    want = _oracle(ref, name)
    n = len(q.frames)
    got = pu.run(lib, name)
    assert int(got["gl_error"]) == 0
    assert got["held"].tolist() == [1] * n, f"{name}: WrhipFlushHeld after each frame returned {got['held'].tolist()}: launches were not held back"
    bad = [k for k in range(n) if tuple(int(v) for v in got["tap%d" % k]) != ft.digest(ft.window_stored(want["frame%d" % k]))]
    assert not bad, f"{name}: frames whose window is not the oracle's: {bad}"
    assert np.array_equal(got["window"], want["window"]), f"{name}: {int((got['window'] != want['window']).sum())} bytes of the final window differ"
    last = {t.name: want["frame%d/%s" % (n - 1, t.name)] for t in q.tiles + [a[0] for a in q.atlases]}
    diff = {t: int((got["tile/" + t] != px).sum()) for t, px in last.items() if not np.array_equal(got["tile/" + t], px)}
    assert not diff, f"{name}: bytes of the tiles that differ after the last frame: {diff}"
    assert all(np.array_equal(want["tile/" + t], px) for t, px in last.items())
    return [got["stats%d" % k] for k in range(n)] + [got["stats_end"]]


def _atlases(ref, name):
    """The off-screen targets that live across the frames, in the oracle's run: a frame changes them inside the task rects it clears
    and redraws, and only there; what it keeps is not one value"""
    q = pu.seq(name)
    want = _oracle(ref, name)
    assert q.atlases
    for tex, per_frame in q.atlases:
        for k in range(1, len(q.frames)):
            prev, cur = _words(want["frame%d/%s" % (k - 1, tex.name)]), _words(want["frame%d/%s" % (k, tex.name)])
            kept = np.ones(cur.shape, bool)
            assert len(per_frame[k]) >= 2
            for r in per_frame[k]:
                kept[r[1]:r[3], r[0]:r[2]] = False
            assert np.array_equal(cur[kept], prev[kept]) and len(np.unique(cur[kept])) > 1, f"{name} frame {k} {tex.name}: the kept tasks"
            assert not np.array_equal(cur[~kept], prev[~kept]), f"{name} frame {k} {tex.name}: the redrawn tasks are as they were"


P1 = [n for n in pu.SEQS if n.startswith("p1_")]
P5 = [n for n in pu.SEQS if n.startswith("p5_")]
ROWS_OFF = ("WRHIP_NO_SPAN_ROWS", "WRHIP_NO_MASK_ROWS", "WRHIP_NO_TILE_ROWS")
P2 = [n for n in pu.SEQS if n.startswith("p2_")]
P3 = [n for n in pu.SEQS if n.startswith("p3_")]


def _p1(lib, ref, name, knob, monkeypatch, device):
    if knob:
        monkeypatch.setenv(knob, "1")
    st = _sequence(lib, ref, name)
    assert _oracle(ref, name)["seen"] == {"partial", "valid", "outside", "untouched"}
    if device:
        # the rect-only kernel variant (the cell raster's) drew the partial frames too
        if knob:
            assert st[-1]["cell_bins"] == 0, st[-1]
        else:
            assert st[-1]["cell_bins"] > st[1]["cell_bins"] > 0, (st[1], st[-1])


def _p2(lib, ref, name):
    _sequence(lib, ref, name)
    assert _oracle(ref, name)["seen"] >= {"partial", "valid", "outside"}


def _p3(lib, ref, name, knob, monkeypatch):
    if knob:
        monkeypatch.setenv(knob, "1")
    st = _sequence(lib, ref, name)
    assert _oracle(ref, name)["seen"] >= {"partial", "valid", "outside"}
    if knob:
        assert st[-1]["row_launches"] == 0, st[-1]
    else:
        # the tile-rows kernel drew every partial frame, not only the first one (st[1]: the launches of frame 0)
        assert st[1]["row_launches"] > 0 and st[-1]["row_launches"] - st[1]["row_launches"] >= len(st) - 3, (st[1], st[-1])


def _p5(lib, ref, name, bins, monkeypatch):
    if bins:
        for knob in ROWS_OFF:
            monkeypatch.setenv(knob, "1")
    st = _sequence(lib, ref, name)
    _atlases(ref, name)
    assert "partial" in _oracle(ref, name)["seen"]
    # libwrhip's atlases after the last frame are in _sequence's comparison of every tile; here: which kernels drew them
    if bins:
        assert st[-1]["row_launches"] == 0, st[-1]
    else:
        assert st[1]["row_launches"] > 0 and st[-1]["row_launches"] - st[1]["row_launches"] >= len(st) - 3, (st[1], st[-1])


def _p4(lib, ref, knob, monkeypatch):
    if knob:
        monkeypatch.setenv(knob, "1")
    st = _sequence(lib, ref, "p4_some_tiles")
    assert _oracle(ref, "p4_some_tiles")["seen"] == {"partial", "valid", "untouched"}
    fw = [s["forwarded_targets"] for s in st[:4]]
    if knob:
        assert fw == [0, 0, 0, 0], fw
    else:
        # the window is a write-through of its tiles only in the frames that redraw every tile
        assert fw[0] > 0 and fw[1] == fw[0] and fw[2] > fw[1] and fw[3] == fw[2], fw


def _p6(lib, ref, family, variant):
    key = (ref, "p6", family)
    if key not in _want:
        _want[key] = pu.run_p6(ref, family, "none")
    control = _want[key]
    if (ref, family, variant) not in _want:
        _want[(ref, family, variant)] = pu.run_p6(ref, family, variant)
    want = _want[(ref, family, variant)]
    assert int(want["gl_error"]) == 0 and int(control["gl_error"]) == 0
    x0, y0, x1, y1 = pu.P6_RECT
    a, b = _words(want["tile"]), _words(control["tile"])
    assert not np.array_equal(a, b), f"p6 {family} {variant}: the oracle draws the same with and without the clear in the middle"
    if variant != "clear_tex":
        # prims behind the cleared writers show: more than the clear's one colour, and not what the writers left
        assert len(np.unique(a[y0:y1, x0:x1])) > 2
    got = pu.run_p6(lib, family, variant)
    assert int(got["gl_error"]) == 0
    assert got["flushes_at_write"].tolist() == [int(got["flushes_first_draw"])], \
        f"p6 {family} {variant}: flushed before the clear ({got['flushes_first_draw']} -> {got['flushes_at_write']}): it met no recorded draws"
    for k in ("mid", "tile"):
        if k in want:
            assert np.array_equal(got[k], want[k]), f"p6 {family} {variant}: {int((got[k] != want[k]).sum())} bytes of '{k}' differ"


# ---------------------------------------------------------------------------- CPU: the host simulation

@pytest.mark.parametrize("knob", [None, "WRHIP_NO_CELLS"], ids=["default", "WRHIP_NO_CELLS"])
@pytest.mark.parametrize("name", P1)
def test_hostsim_rects_over_kept_content(hostsim, oracle_gcc, name, knob, monkeypatch):
    _p1(hostsim, oracle_gcc, name, knob, monkeypatch, False)


@pytest.mark.parametrize("name", P2)
def test_hostsim_images_text_masks_over_kept_content(hostsim, oracle_gcc, name):
    _p2(hostsim, oracle_gcc, name)


@pytest.mark.parametrize("knob", [None, "WRHIP_NO_TILE_ROWS"], ids=["default", "WRHIP_NO_TILE_ROWS"])
@pytest.mark.parametrize("name", P3)
def test_hostsim_tile_rows_over_kept_content(hostsim, oracle_gcc, name, knob, monkeypatch):
    _p3(hostsim, oracle_gcc, name, knob, monkeypatch)


@pytest.mark.parametrize("knob", [None, "WRHIP_NO_FORWARD"], ids=["default", "WRHIP_NO_FORWARD"])
def test_hostsim_some_tiles_only(hostsim, oracle_gcc, knob, monkeypatch):
    _p4(hostsim, oracle_gcc, knob, monkeypatch)


@pytest.mark.parametrize("bins", [False, True], ids=["rows", "bins"])
@pytest.mark.parametrize("name", P5)
def test_hostsim_offscreen_tasks_cleared_and_redrawn(hostsim, oracle_gcc, name, bins, monkeypatch):
    _p5(hostsim, oracle_gcc, name, bins, monkeypatch)


@pytest.mark.parametrize("family,variant", pu.P6_CASES)
def test_hostsim_clear_in_the_middle_of_a_target(hostsim, oracle_gcc, family, variant):
    _p6(hostsim, oracle_gcc, family, variant)


# ---------------------------------------------------------------------------- GPU: libwrhip on the MI355X

def _gpu_ref():
    ref = oracle_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("knob", [None, "WRHIP_NO_CELLS"], ids=["default", "WRHIP_NO_CELLS"])
@pytest.mark.parametrize("name", P1)
def test_gpu_rects_over_kept_content(name, knob, monkeypatch):
    _p1(wrhip_lib(), _gpu_ref(), name, knob, monkeypatch, True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", P2)
def test_gpu_images_text_masks_over_kept_content(name):
    _p2(wrhip_lib(), _gpu_ref(), name)


@pytest.mark.gpu
@pytest.mark.parametrize("knob", [None, "WRHIP_NO_TILE_ROWS"], ids=["default", "WRHIP_NO_TILE_ROWS"])
@pytest.mark.parametrize("name", P3)
def test_gpu_tile_rows_over_kept_content(name, knob, monkeypatch):
    _p3(wrhip_lib(), _gpu_ref(), name, knob, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("knob", [None, "WRHIP_NO_FORWARD"], ids=["default", "WRHIP_NO_FORWARD"])
def test_gpu_some_tiles_only(knob, monkeypatch):
    _p4(wrhip_lib(), _gpu_ref(), knob, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("bins", [False, True], ids=["rows", "bins"])
@pytest.mark.parametrize("name", P5)
def test_gpu_offscreen_tasks_cleared_and_redrawn(name, bins, monkeypatch):
    _p5(wrhip_lib(), _gpu_ref(), name, bins, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("family,variant", pu.P6_CASES)
def test_gpu_clear_in_the_middle_of_a_target(family, variant):
    _p6(wrhip_lib(), _gpu_ref(), family, variant)
