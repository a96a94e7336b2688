"""Generates tests/golden/gradient_sweep.json from the oracle (oracle/_ref/libswgl_ref_gen.so, the hand-header build where that is
absent): per family of tests/gradient_cases.py one digest per case, of the bytes the oracle leaves in the case's cell, in the order
of the table (the tags are the case module's to regenerate), and one per frame, of the whole readback.
`python tests/golden/make_gradient_sweep.py`; the digests stand in where the oracle cannot be built."""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from webrender_amd.harness import render_direct
import gradient_cases as P


def main():
    ref = os.path.join(ROOT, "oracle", "_ref")
    lib = next(p for p in (os.path.join(ref, "libswgl_ref_gen.so"), os.path.join(ref, "libswgl_ref_gcc.so")) if os.path.exists(p))
    out = {"seed": P.SEED}
    for fam in P.FAMILIES:
        out[fam] = {"frames": {}, "cases": [None] * len(P.CASES[fam])}
        for name in P.FRAMES[fam]:
            img = P.image(render_direct(lib, P.make_frame(fam, name))[0], fam, name)
            out[fam]["frames"][name] = P.digest(img)
            for c in P.frame_cases(fam, name):
                out[fam]["cases"][c["index"]] = P.digest(P.cell_of(img, c))
    with open(os.path.join(ROOT, "tests", "golden", "gradient_sweep.json"), "w") as f:
        json.dump(out, f, indent=0)
    print({k: len(v["cases"]) for k, v in out.items() if k != "seed"})


if __name__ == "__main__":
    main()
