"""Parity under the transforms no scene builder draws (tests/transform_classes.py): the rotated families mirrored, under exact
quarter / half turns and axis flips, scaled, smaller than a pixel, larger than the target, beyond 32-bit integers, singular, and
at device pixel scales 1.5 and 0.77; the projective families mirrored on screen; and, since every builder asks for all four
anti-aliased edges on a transformed prim, the affine and the mirrored classes once more with a subset of the edges per prim
(`reedge`: which screen edge an aa_edges bit lands on under a reversed winding -- with all four set nothing tells).  The host simulation against the reference's
generated program here, libwrhip on the MI355X (-m gpu) against the same oracle: 0 differing bytes and no gl_error -- on the
device the mix-blend family within 1 LSB on at most 1e-4 of the bytes (its sqrt / division come from the device's math library,
tests/test_gpu_parity.py::test_hip_mix_blend_matches_oracle), and only there.

Against vacuity the oracle's image of a rewritten scene has to differ from its image of the unrewritten one, and at least 1000
of its pixels have to differ from the clear colour."""
import hashlib
import numpy as np
import pytest
from conftest import wrhip_lib, oracle_ref
from webrender_amd.harness import render_direct
import transform_classes as X

MIN_DRAWN = 1000
_base = {}      # scene name -> digest of the oracle's image of the unrewritten scene


def _flat(x):
    if isinstance(x, dict):
        return np.concatenate([x[k].ravel() for k in sorted(x)])
    return x.ravel()


def _base_digest(ref, name, make):
    if name not in _base:
        _base[name] = hashlib.sha256(_flat(render_direct(ref, make())[0]).tobytes()).hexdigest()
    return _base[name]


def _rewritten(make, cls):
    frame = make()
    assert X.retransform(frame, cls) > 0
    return frame


def _check(lib, ref, case, name, make, cls, tol):
    frame = _rewritten(make, cls)
    want, _ = render_direct(ref, _rewritten(make, cls))
    got, st = render_direct(lib, frame)
    win = want["window"] if isinstance(want, dict) else want
    clear = (np.asarray(frame.clear_color) * 255.0 + 0.5).astype(np.uint8)
    assert clear[0] == clear[2]      # (so the window's channel order does not matter here: every builder clears to white)
    drawn = int((win != clear).any(axis=-1).sum())
    assert drawn >= MIN_DRAWN, f"{case}: the oracle draws {drawn} pixels"
    assert hashlib.sha256(_flat(want).tobytes()).hexdigest() != _base_digest(ref, name, make), f"{case}: the oracle's image is that of the unrewritten scene"
    d = np.abs(_flat(got).astype(np.int16) - _flat(want).astype(np.int16))
    count, worst = int((d > 0).sum()), int(d.max())
    print(f"{case}: {count} differing bytes, max {worst}, gl_error {st['gl_error']:#x}, {drawn} pixels drawn")
    where = ""
    if count and cls in X.MIXED:
        gw = got["window"] if isinstance(got, dict) else got
        where = f", first at {X.first_member_at(frame, cls, (gw != win).any(axis=-1))}"
    assert st["gl_error"] == 0, f"{case}: gl_error {st['gl_error']:#x}"
    if tol:
        assert worst <= 1 and count <= 1e-4 * d.size, f"{case}: {count} differing bytes of {d.size}, max {worst}{where}"
    else:
        assert np.array_equal(_flat(got), _flat(want)), f"{case}: {count} differing bytes, max {worst}{where}"


@pytest.mark.parametrize("case,name,make,cls", X.ALL, ids=[c[0] for c in X.ALL])
def test_hostsim_transform_classes_match_oracle(hostsim, oracle_gcc, case, name, make, cls):
    _check(hostsim, oracle_gcc, case, name, make, cls, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("case,name,make,cls", X.ALL, ids=[c[0] for c in X.ALL])
def test_gpu_transform_classes_match_oracle(case, name, make, cls):
    ref = oracle_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    _check(wrhip_lib(), ref, case, name, make, cls, 1 if name in X.DEVICE_ONE_LSB else 0)


# ---------------------------------------------------------------------------- the helper itself

def test_retransform_members():
    """every member of both mixed classes is stored as T(c) . L . T(-c) about the builder's centre with its inverse, exact maps are
    exact, singular members carry a zero inverse block, the identity stays"""
    from webrender_amd import scenes
    for cls, cycle in (("affine", 8), ("degenerate", 12)):
        base, frame = scenes.rotated_rects(n=40), scenes.rotated_rects(n=40)
        assert X.retransform(frame, cls) == 40
        d0, d = base.transforms.data, frame.transforms.data
        assert np.array_equal(d[:8], d0[:8])
        seen = set()
        for k in range(1, 41):
            m0, m = d0[8 * k:8 * k + 4].T.astype(np.float64), d[8 * k:8 * k + 4].T.astype(np.float64)
            inv = d[8 * k + 4:8 * k + 8].T.astype(np.float64)
            c = np.linalg.solve(m0[:2, :2] - np.eye(2), -m0[:2, 3])
            lin = m[:2, :2]
            assert np.allclose(lin @ c + m[:2, 3], c, rtol=0, atol=1e-6 * max(1.0, float(np.abs(lin).max())) * 1024), (cls, k)
            seen.add(k % cycle)
            if cls == "affine":
                j = k % 8
                if j == 0:
                    exp = m0[:2, :2] @ np.diag([-1.0, 1.0])
                    assert np.linalg.det(lin) < 0
                elif j <= 6:
                    exp = X.EXACT[j - 1][1]
                    assert np.array_equal(lin, exp)
                else:
                    exp = m0[:2, :2] @ np.diag(X.AFFINE_SCALES[(k // 8) % 4])
            else:
                s = X.DEGENERATE[k % 12][1]
                exp = m0[:2, :2] @ np.diag(s)
                if 0.0 in s:
                    assert not inv.any()
            # (float32 blocks of float64 results: 1e-6 of the largest entry; the centre is 1024 at the most)
            assert np.allclose(lin, exp, rtol=0, atol=1e-6 * float(np.abs(exp).max())), (cls, k)
            if abs(np.linalg.det(exp)) > 1e-20:
                einv = np.linalg.inv(exp)
                assert np.allclose(inv[:2, :2], einv, rtol=0, atol=1e-6 * float(np.abs(einv).max())), (cls, k)
                assert np.allclose(inv[:2, :2] @ c + inv[:2, 3], c, rtol=0, atol=1e-6 * max(1.0, float(np.abs(einv).max())) * 1024), (cls, k)
        assert seen == set(range(cycle))
    frame = scenes.rotated_rects(n=40, perspective=True)
    assert X.retransform(frame, "affine") == 0
    assert X.retransform(frame, "screen_mirror") == 40
    n_tasks = frame.render_tasks.len // 2
    assert X.retransform(frame, "dps1.5") == n_tasks and X.retransform(frame, "dps1.5") == 0
    assert (frame.render_tasks.data[1:2 * n_tasks:2, 0] == 1.5).all()


def test_reedge_subsets():
    """brush and quad instances of transformed prims get the subset of their transform index -- never none, never all four, several per
    member of the affine cycle -- and nothing else in the instance word changes; prims that asked for no anti-aliasing keep that"""
    from webrender_amd import scenes
    assert {X.edge_subset(k) for k in range(1, 41)} <= set(range(1, 15))
    for j in range(8):
        assert len({X.edge_subset(k) for k in range(1, 41) if k % 8 == j}) >= 4
    for enc, shift in (("brush", 28), ("quad", 16)):
        base, frame = scenes.rotated_rects(n=40, encoding=enc), scenes.rotated_rects(n=40, encoding=enc)
        n = X.reedge(frame)
        assert n == sum(len(st.instances) for tg in frame.passes[0] for st in tg.alpha) > 0
        for tg0, tg in zip(base.passes[0], frame.passes[0]):
            for st0, st in zip(tg0.alpha, tg.alpha):
                a, b = st0.instances.astype(np.int64) & 0xFFFFFFFF, st.instances.astype(np.int64) & 0xFFFFFFFF
                assert np.array_equal(a[:, [0, 1, 3]], b[:, [0, 1, 3]])
                assert ((a[:, 2] >> shift) & 15 == 15).all() and np.array_equal(a[:, 2] & ~(15 << shift), b[:, 2] & ~(15 << shift))
                for r in range(len(b)):
                    k = int(frame.gpu_buffer_i.data[b[r, 0], 0] if enc == "quad" else frame.prim_headers_i.data[2 * b[r, 0], 2]) & 0x3FFFFF
                    assert (b[r, 2] >> shift) & 15 == X.edge_subset(k)
    frame = scenes.masked_rects(n=40, seed=12)      # (axis-aligned prims without anti-aliasing)
    assert X.reedge(frame) == 0 and X.retransform(frame, "affine_edges") == 0
