"""Generates tests/golden/pixel_calls.json from the oracle (oracle/_ref/libswgl_ref_gen.so, the hand-header build where that is
absent): one SHA-256 per case of tests/pixel_call_cases.py, of the bytes the oracle leaves in the case's destination, keyed by
family and in the order of the tables (the tags are the case module's to regenerate).  `python tests/golden/make_pixel_calls.py`;
the digests stand in where the oracle cannot be built."""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pixel_call_cases as P


def main():
    ref = os.path.join(ROOT, "oracle", "_ref")
    lib = next(p for p in (os.path.join(ref, "libswgl_ref_gen.so"), os.path.join(ref, "libswgl_ref_gcc.so")) if os.path.exists(p))
    out = {"seed": P.SEED}
    for fam in P.FAMILIES:
        out[fam] = [P.digest(r) for r in P.run_family(lib, fam)]
    with open(os.path.join(ROOT, "tests", "golden", "pixel_calls.json"), "w") as f:
        json.dump(out, f, indent=0)
    print({k: len(v) for k, v in out.items() if k != "seed"})


if __name__ == "__main__":
    main()
