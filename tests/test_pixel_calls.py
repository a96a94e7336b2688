"""The immediate pixel calls -- BlitFramebuffer, Composite, CompositeYUV, the texture / rect clears, TexSubImage2D and ReadPixels --
swept over the deterministic case tables of tests/pixel_call_cases.py: every case on the reference's swgl and on libwrhip (the host
simulation here, the HIP build on the GPU), the destination's bytes compared.  These are integer and fixed-point paths whose float
set-up is the same IEEE operations on both sides: 0 differing bytes."""
import json
import os
import time
import numpy as np
import pytest
from conftest import ROOT, wrhip_lib, oracle_ref
import pixel_call_cases as P

GOLDEN = os.path.join(ROOT, "tests", "golden", "pixel_calls.json")
_results = {}          # (library, family, call) -> results: computed once, shared, left unchanged


def results(lib, family, call=True):
    key = (lib, family, call)
    if key not in _results:
        t0 = time.perf_counter()
        _results[key] = P.run_family(lib, family, call)
        print(f"pixel calls: {family}: {len(_results[key])} cases on {os.path.basename(lib)} in {time.perf_counter() - t0:.2f} s")
    return _results[key]


def differing(family, got, want):
    """the cases whose bytes differ: (number of them, lines for the first eight: tag, byte count, largest difference)"""
    lines, n = [], 0
    for c, a, b in zip(P.CASES[family], got, want):
        if a.shape == b.shape and np.array_equal(a, b):
            continue
        n += 1
        if len(lines) < 8:
            if a.shape != b.shape:
                lines.append(f"{c['tag']}: {a.size} bytes against {b.size}")
            else:
                d = np.abs(a.astype(np.int16) - b.astype(np.int16))
                lines.append(f"{c['tag']}: {int((d > 0).sum())} bytes differ, max {int(d.max())}")
    return n, lines


def views_disagree(family, got):
    """Composite / CompositeYUV destinations are read through GetResourceBuffer and through ReadPixels: the tags where the two differ"""
    if family not in P.TWO_VIEWS:
        return []
    return [c["tag"] for c, r in zip(P.CASES[family], got) if not np.array_equal(r[:r.size // 2], r[r.size // 2:])][:8]


def against_digests(family, got):
    gold = json.load(open(GOLDEN))
    assert gold["seed"] == P.SEED and len(gold[family]) == len(P.CASES[family])
    return [c["tag"] for c, r, g in zip(P.CASES[family], got, gold[family]) if P.digest(r) != g]


def check_hostsim(family, hostsim, oracle_gcc):
    want, got = results(oracle_gcc, family), results(hostsim, family)
    n, lines = differing(family, got, want)
    assert n == 0, f"{n} of {len(want)} {family} cases differ from the oracle:\n" + "\n".join(lines)
    assert not views_disagree(family, want) and not views_disagree(family, got)
    # the calls have to DO something: a case the oracle leaves the destination unchanged in shows nothing
    before = results(oracle_gcc, family, call=False)
    noop = sum(int(np.array_equal(a, b)) for a, b in zip(want, before))
    print(f"pixel calls: {family}: {noop} of {len(want)} cases are no-ops on the oracle ({100.0 * noop / len(want):.1f} %)")
    assert noop <= P.NOOP_CAP * len(want), f"{family}: {noop} of {len(want)} cases leave the destination unchanged"
    # the committed digests (what the GPU box compares with when the oracle is absent) are the oracle's
    assert not against_digests(family, want)


def check_hip(family):
    got = results(wrhip_lib(), family)
    ref = oracle_ref()
    if ref:
        n, lines = differing(family, got, results(ref, family))
        assert n == 0, f"{n} of {len(got)} {family} cases differ from the oracle:\n" + "\n".join(lines)
    bad = against_digests(family, got)
    assert not bad, f"{len(bad)} of {len(got)} {family} cases differ from the oracle's digests:\n" + "\n".join(bad[:8])
    assert not views_disagree(family, got)


def test_hostsim_blit_matches_oracle(hostsim, oracle_gcc):
    check_hostsim("blit", hostsim, oracle_gcc)


def test_hostsim_composite_matches_oracle(hostsim, oracle_gcc):
    check_hostsim("composite", hostsim, oracle_gcc)


def test_hostsim_composite_yuv_matches_oracle(hostsim, oracle_gcc):
    check_hostsim("composite_yuv", hostsim, oracle_gcc)


def test_hostsim_clear_matches_oracle(hostsim, oracle_gcc):
    check_hostsim("clear", hostsim, oracle_gcc)


def test_hostsim_upload_matches_oracle(hostsim, oracle_gcc):
    check_hostsim("upload", hostsim, oracle_gcc)


@pytest.mark.gpu
def test_hip_blit_matches_oracle():
    check_hip("blit")


@pytest.mark.gpu
def test_hip_composite_matches_oracle():
    check_hip("composite")


@pytest.mark.gpu
def test_hip_composite_yuv_matches_oracle():
    check_hip("composite_yuv")


@pytest.mark.gpu
def test_hip_clear_matches_oracle():
    check_hip("clear")


@pytest.mark.gpu
def test_hip_upload_matches_oracle():
    check_hip("upload")
