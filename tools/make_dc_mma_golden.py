#!/usr/bin/env python3
"""Records tests/golden/dc_mma_reduce_store_v1.json: a SHA-256 of the output bytes of every case of
tests/test_dc_mma_reduce_store.py, from the emulation (tests/emu) of the kernel sources in THIS tree.

Run it on the commit whose bits are to be pinned (the file in the repository was recorded on the parent of the commit that spread
the K-slice reduction and the epilogue over all waves), never to make a failing test pass:

    python tools/make_dc_mma_golden.py out.json            # a file of its own, to compare
    python tools/make_dc_mma_golden.py --overwrite-golden  # replaces the committed fixture
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_dc_mma_reduce_store as t   # noqa: E402
from tests.fp64_env import Env   # noqa: E402

if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    path = t.GOLDEN if sys.argv[1] == "--overwrite-golden" else sys.argv[1]
    if sys.argv[1] != "--overwrite-golden" and os.path.abspath(path) == os.path.abspath(t.GOLDEN):
        sys.exit("the committed fixture is replaced only with --overwrite-golden")
    env = Env(emu=True)
    out = {}
    for cid in sorted(t.CASES):
        got, again, _ = t.run_case(env, cid)
        assert got.tobytes() == again.tobytes(), cid
        out[cid] = t.sha(got)
        print(cid, out[cid][:16], flush=True)
    with open(path, "w") as f:
        json.dump({"what": "sha256 of '<shape>|' + the float32 output bytes, per case of tests/test_dc_mma_reduce_store.py", "sha256": out}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)
