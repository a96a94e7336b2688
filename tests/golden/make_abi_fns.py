#!/usr/bin/env python3
"""Extract the reference's C ABI -- the `extern "C"` block of swgl/src/swgl_fns.rs -- as data: every function name in
declaration order with its argument count.

  python3 tests/golden/make_abi_fns.py <reference tree> > tests/golden/swgl_fns.json

tests/test_abi.py holds glapi.SIGNATURES to the committed fixture, and re-derives it where the reference tree is present."""
import json
import os
import re
import sys


def extern_block_functions(src):
    block = src[src.index('extern "C" {'):src.index("#[derive(Clone, Copy)]")]
    out = []
    for m in re.finditer(r"fn (\w+)\((.*?)\)(?: -> [^;]+)?;", block, flags=re.S):
        name, args = m.group(1), m.group(2).strip()
        out.append([name, 0 if not args else len([a for a in args.split(",") if a.strip()])])
    assert len(out) == len(re.findall(r"fn (\w+)\(", block)), "a declaration the pattern does not read"
    return out


if __name__ == "__main__":
    with open(os.path.join(sys.argv[1], "swgl", "src", "swgl_fns.rs")) as f:
        fns = extern_block_functions(f.read())
    print('{"source": "swgl/src/swgl_fns.rs extern \\"C\\" block, extracted by tests/golden/make_abi_fns.py",\n"functions": [\n'
          + ",\n".join(json.dumps(f) for f in fns) + "\n]}")
