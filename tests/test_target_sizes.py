"""Parity at target sizes that are no multiple of the raster's 64-px bin (tests/tile_size_cases.py): every shader family
drawn into picture-cache tiles of 61x37 ... 32x1024 under a window that cuts the last tiles, and the off-screen families at
atlas sizes 331 / 512 / 513 / 515 -- the host simulation, and libwrhip.so on the MI355X through the C ABI, against the oracle.

Every tile texture is read back besides the window, so the pixels a composite clips away are compared and a wrong store is
attributed to the tile it happened in.  0 differing bytes and no gl_error; on the GPU the families tests/test_gpu_sweep.py
lists in ONE_LSB keep that file's rule (at most 1 LSB, on at most 1e-3 of the bytes).

What keeps a case from being vacuous is asserted on the oracle's output alone: at least half of the tiles differ from their
clear colour in their last column, in their last row, and at all; an off-screen target differs from its clear colour in its
last column and its last row.  For the rect families at default settings WrhipStats shows that forwarded composites
(forwarded_targets) and, on the GPU, the cell raster's kernel variant (cell_bins) took part: without that the WRHIP_NO_* runs
would compare a path with itself.

Without the oracle (a checkout that cannot build it) the GPU tests hold the bit-exact cases to the oracle's digests in
tests/golden/target_sizes.json (tests/golden/make_target_sizes.py)."""
import hashlib
import json
import os
import numpy as np
import pytest
from conftest import ROOT, wrhip_lib, oracle_ref
from webrender_amd import scenes
from webrender_amd.harness import render_direct
from test_gpu_sweep import ONE_LSB
from tile_size_cases import (tile_cases, build_tile_frame, coverage, offscreen_cases, touches_edges, RECT_FAMILIES)

TILE_CASES = tile_cases()
OFFSCREEN = offscreen_cases()
OFFSCREEN_ENVS = {"rows": {}, "bins": {"WRHIP_NO_SPAN_ROWS": "1", "WRHIP_NO_MASK_ROWS": "1"}}
# the clear colour of the off-screen targets (R8 masks clear to 1.0, everything else to 0)
OFFSCREEN_CLEAR = {"clip_masks": 255, "box_shadow_masks": 255}
_GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "target_sizes.json")
GOLDEN = json.load(open(_GOLDEN_PATH)) if os.path.exists(_GOLDEN_PATH) else {}
_oracle_cache = {}


def flat(out):
    return np.concatenate([out[k].ravel() for k in sorted(out)])


def digest(out):
    return hashlib.sha256(flat(out).tobytes()).hexdigest()


def oracle_tiles(ref, tile, fam):
    """The oracle's output of a (tile size, family) pair, rendered once for all the tests that compare with it, with the
    conditions on it that keep the case from being vacuous."""
    key = (ref, tile, fam)
    if key not in _oracle_cache:
        frame = build_tile_frame(tile, fam)
        want, _ = render_direct(ref, frame)
        for v in want.values():
            v.setflags(write=False)
        col, row, anyw = coverage(frame, want)
        print(f"{tile[0]}x{tile[1]} {fam}: {len(want) - 1} tiles; last column / last row / anything drawn in {col:.2f} / {row:.2f} / {anyw:.2f} of them")
        assert col >= 0.5 and row >= 0.5 and anyw >= 0.5, (col, row, anyw)
        _oracle_cache[key] = want
    return _oracle_cache[key]


def oracle_offscreen(ref, name, make, edge_targets):
    key = (ref, name)
    if key not in _oracle_cache:
        want, _ = render_direct(ref, make())
        for v in want.values():
            v.setflags(write=False)
        for t in edge_targets:
            col, row = touches_edges(want[t], OFFSCREEN_CLEAR.get(t, 0))
            assert col and row, f"{name}: {t} is untouched in its last column / row ({col}, {row})"
        _oracle_cache[key] = want
    return _oracle_cache[key]


def check(got, want, st, tol=0):
    assert st["gl_error"] == 0, hex(st["gl_error"])
    assert set(got) == set(want)
    bad = []
    total = differing = 0
    for k in sorted(want):
        assert got[k].shape == want[k].shape, k
        d = np.abs(got[k].astype(np.int16) - want[k].astype(np.int16))
        total += d.size
        differing += int((d > 0).sum())
        if d.max() > tol:
            ys, xs = np.nonzero(d.reshape(d.shape[0], d.shape[1], -1).max(axis=2) > tol)
            bad.append(f"{k}: max |diff| {int(d.max())}, {int((d > tol).sum())} bytes, first at x {int(xs[0])} y {int(ys[0])}")
    assert not bad, "; ".join(bad[:6])
    assert differing <= (1e-3 * total if tol else 0), (differing, total)


def took_part(fam, knob, st, gpu):
    """default-settings runs of the rect families: the paths the WRHIP_NO_* runs switch off did run"""
    if fam in RECT_FAMILIES and knob is None:
        assert st["forwarded_targets"] > 0, st
        if gpu:
            assert st["cell_bins"] > 0, st


@pytest.mark.parametrize("name,tile,fam,knob", TILE_CASES, ids=[c[0] for c in TILE_CASES])
def test_hostsim_tiles_match_oracle(hostsim, oracle_gcc, name, tile, fam, knob, monkeypatch):
    want = oracle_tiles(oracle_gcc, tile, fam)
    if knob:
        monkeypatch.setenv(knob, "1")
    got, st = render_direct(hostsim, build_tile_frame(tile, fam))
    check(got, want, st)
    took_part(fam, knob, st, gpu=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name,tile,fam,knob", TILE_CASES, ids=[c[0] for c in TILE_CASES])
def test_hip_tiles_match_oracle(name, tile, fam, knob, monkeypatch):
    if knob:
        monkeypatch.setenv(knob, "1")
    got, st = render_direct(wrhip_lib(), build_tile_frame(tile, fam))
    took_part(fam, knob, st, gpu=True)
    ref = oracle_ref()
    if ref:
        check(got, oracle_tiles(ref, tile, fam), st, tol=1 if fam in ONE_LSB else 0)
        return
    if fam in ONE_LSB or (fam == "text" and hashlib.sha256(scenes.build_glyph_atlas()[0].tobytes()).hexdigest() != GOLDEN.get("glyph_atlas")):
        pytest.skip("needs the oracle: no digest holds for this family")
    assert st["gl_error"] == 0
    assert digest(got) == GOLDEN[f"{tile[0]}x{tile[1]}-{fam}"], "differs from the oracle's digest"


@pytest.mark.parametrize("evaluation", list(OFFSCREEN_ENVS))
@pytest.mark.parametrize("name,make,edge_targets", OFFSCREEN, ids=[c[0] for c in OFFSCREEN])
def test_hostsim_offscreen_atlases_match_oracle(hostsim, oracle_gcc, name, make, edge_targets, evaluation, monkeypatch):
    want = oracle_offscreen(oracle_gcc, name, make, edge_targets)
    for k, v in OFFSCREEN_ENVS[evaluation].items():
        monkeypatch.setenv(k, v)
    got, st = render_direct(hostsim, make())
    check(got, want, st)


@pytest.mark.gpu
@pytest.mark.parametrize("evaluation", list(OFFSCREEN_ENVS))
@pytest.mark.parametrize("name,make,edge_targets", OFFSCREEN, ids=[c[0] for c in OFFSCREEN])
def test_hip_offscreen_atlases_match_oracle(name, make, edge_targets, evaluation, monkeypatch):
    for k, v in OFFSCREEN_ENVS[evaluation].items():
        monkeypatch.setenv(k, v)
    got, st = render_direct(wrhip_lib(), make())
    fam = name.rsplit("-", 1)[0]
    ref = oracle_ref()
    if ref:
        check(got, oracle_offscreen(ref, name, make, edge_targets), st, tol=1 if fam in ONE_LSB else 0)
        return
    if fam in ONE_LSB:
        pytest.skip("needs the oracle: no digest holds for this family")
    assert st["gl_error"] == 0
    assert digest(got) == GOLDEN[name], "differs from the oracle's digest"
