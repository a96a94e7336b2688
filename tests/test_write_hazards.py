"""Writes to textures that recorded or held-back draws still read: the hazard layer of libwrhip (Texture::pending_read / pending_write /
tail_ref, sync_texture_for_write / _read, find_or_add_work, free_texture_storage, set_tex_storage, order_upload, Tail::refs) under the
call orders of a frame loop -- tests/hazard_cases.py has the scripts.  Every comparison is byte for byte against the oracle, which
executes each call at once; nothing about HOW libwrhip resolves a hazard is asserted, only pixels and GetError() == 0.

Each case also shows that it is not vacuous.  In the oracle's run the results on either side of the write differ.  In libwrhip's run
the hazard was there when the write came: in group A no flush happened between the recording of the first draw and the write, in group
B the raster launches of every frame were still held back behind it.

Each case runs on the host simulation and, under -m gpu, on the MI355X."""
import numpy as np
import pytest
from conftest import wrhip_lib, oracle_ref
import frame_taps as ft
import hazard_cases as hz

A_CASES = [n for n, c in hz.CASES.items() if c.group == "A"]
B_CASES = [n for n, c in hz.CASES.items() if c.group == "B"]

_want = {}


def _oracle(ref, name):
    """The oracle's run of a case, once per session"""
    if (ref, name) not in _want:
        _want[(ref, name)] = hz.run(ref, name)
    return _want[(ref, name)]


def _pending(lib, ref, name):
    case = hz.CASES[name]
    want = _oracle(ref, name)
    assert int(want["gl_error"]) == 0
    for before, after in case.differ:
        assert want[before].shape == want[after].shape and not np.array_equal(want[before], want[after]), \
            f"{name}: the oracle draws {before} and {after} alike -- the write changes nothing that is looked at"
    got = hz.run(lib, name)
    assert int(got["gl_error"]) == 0
    writes = got["flushes_at_write"]
    assert len(writes) >= 1 and (writes == got["flushes_first_draw"]).all(), \
        f"{name}: flushed before the write ({got['flushes_first_draw']} -> {writes}): it met no recorded draws"
    names = [k for k in want if k != "gl_error"]
    assert len(names) >= 2
    bad = [f"{k}: {int((got[k] != want[k]).sum())} bytes differ" for k in names if not np.array_equal(got[k], want[k])]
    assert not bad, f"{name}: {bad}"


def _held(lib, ref, name):
    want = _oracle(ref, name)
    assert int(want["gl_error"]) == 0
    n = sum(1 for k in want if k.startswith("frame"))
    assert n >= 3
    for k in range(1, n):
        assert not np.array_equal(want["frame%d" % (k - 1)], want["frame%d" % k]), f"{name}: the oracle's frames {k - 1} and {k} are alike"
    assert np.array_equal(want["window"], want["frame%d" % (n - 1)])
    got = hz.run(lib, name)
    assert int(got["gl_error"]) == 0
    assert got["held"].tolist() == [1] * n, f"{name}: WrhipFlushHeld after each frame returned {got['held'].tolist()}: launches were not held back"
    bad = [k for k in range(n) if tuple(int(v) for v in got["tap%d" % k]) != ft.digest(ft.window_stored(want["frame%d" % k]))]
    assert not bad, f"{name}: frames whose window is not the oracle's: {bad}"
    assert np.array_equal(got["window"], want["window"]), f"{name}: {int((got['window'] != want['window']).sum())} bytes of the final window differ"


# ---------------------------------------------------------------------------- CPU: the host simulation

@pytest.mark.parametrize("name", A_CASES)
def test_hostsim_write_meets_recorded_draws(hostsim, oracle_gcc, name):
    _pending(hostsim, oracle_gcc, name)


@pytest.mark.parametrize("name", B_CASES)
def test_hostsim_write_meets_held_launches(hostsim, oracle_gcc, name):
    _held(hostsim, oracle_gcc, name)


# ---------------------------------------------------------------------------- GPU: libwrhip on the MI355X

def _gpu_ref():
    ref = oracle_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name", A_CASES)
def test_gpu_write_meets_recorded_draws(name):
    _pending(wrhip_lib(), _gpu_ref(), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", B_CASES)
def test_gpu_write_meets_held_launches(name):
    _held(wrhip_lib(), _gpu_ref(), name)
