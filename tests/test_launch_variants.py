"""Every raster launch goes out as the kernel variant the recorded fixture names (tests/launch_variant_cases.py): the rows
tests/golden/launch_variants.json holds were recorded on the host simulation before the choice of a launch's kernel was gathered into
one selector, and describe every launch after it -- on the host simulation and on the MI355X."""
import pytest

import launch_variant_cases as lv
from webrender_amd import glapi


@pytest.fixture(scope="module")
def fixture():
    return lv.load_fixture()


def _check(lib, name, make, env, fixture):
    assert fixture[name]["env"] == env, "the fixture was recorded under other switches"
    rows, st = lv.observe(lib, make, env)
    print(name, rows)
    assert st["gl_error"] == 0 and st["carrier_lost"] == 0, st
    assert rows == fixture[name]["rows"]


@pytest.mark.parametrize("name,make,env", lv.CASES, ids=lv.CASE_IDS)
def test_hostsim_launch_variants(hostsim, fixture, name, make, env):
    _check(hostsim, name, make, env, fixture)


@pytest.mark.gpu
@pytest.mark.parametrize("name,make,env", lv.CASES, ids=lv.CASE_IDS)
def test_gpu_launch_variants(fixture, name, make, env):
    _check(glapi.wrhip_path(), name, make, env, fixture)          # (WRHIP_LIB_PATH: another build, e.g. the one the fixture was recorded at)


def test_fixture_reaches_every_instantiated_kernel(fixture):
    """Every kernel a held launch can go out as -- WR_INST_ALL, the chain kernels, the row kernels and their fused forms -- is
    launched by some case, but for the R8 variants without any feature that UNREACHED names."""
    seen = {tuple(r[:4]) for case in fixture.values() for r in case["rows"]}
    inst = lv.instantiated()
    assert set(lv.UNREACHED) <= set(inst)
    assert all(inst[n][1] == lv.R8 and inst[n][3] == 0 and n.startswith(("wr_raster_kernel<", "wr_raster_chain_kernel<")) for n in lv.UNREACHED), \
        "only R8 feature-set-0 variants may be exempt: anything else needs a scene"
    missing = []
    for name, (kind, fmt, depth, feat) in inst.items():
        hit = any(k == kind and ft == feat and fmt in (None, f) and depth in (None, d) for k, f, d, ft in seen)
        if not hit and name not in lv.UNREACHED:
            missing.append(name)
        assert not (hit and name in lv.UNREACHED), f"{name} is reached: take it off UNREACHED"
    assert not missing, missing
