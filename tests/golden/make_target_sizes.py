"""Generates tests/golden/target_sizes.json from the oracle (oracle/_ref/libswgl_ref_gen.so, the hand-header build where that
is absent): one digest per bit-exact case of tests/test_target_sizes.py, over every read-back target and the window in the
order of their names.  `python tests/golden/make_target_sizes.py`; the digests stand in where the oracle cannot be built."""
import hashlib
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import oracle_ref
from webrender_amd import scenes
from webrender_amd.harness import render_direct
from test_gpu_sweep import ONE_LSB
from test_target_sizes import digest
from tile_size_cases import TILES, FAMILIES, build_tile_frame, offscreen_cases


def main():
    lib = oracle_ref()
    out = {"glyph_atlas": hashlib.sha256(scenes.build_glyph_atlas()[0].tobytes()).hexdigest()}
    for tile in TILES:
        for fam in FAMILIES:
            if fam not in ONE_LSB:
                out[f"{tile[0]}x{tile[1]}-{fam}"] = digest(render_direct(lib, build_tile_frame(tile, fam))[0])
    for name, make, _ in offscreen_cases():
        if name.rsplit("-", 1)[0] not in ONE_LSB:
            out[name] = digest(render_direct(lib, make())[0])
    with open(os.path.join(ROOT, "tests", "golden", "target_sizes.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(len(out), "digests")


if __name__ == "__main__":
    main()
