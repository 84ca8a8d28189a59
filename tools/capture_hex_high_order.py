#!/usr/bin/env python3
"""Capture the P6 and P7 hexahedron fixtures (tests/golden/hex_p6_deformed.npz, hex_p7_deformed.npz) -- TEST
INFRASTRUCTURE, container only.

Runs the genuine reference that `build()` compiles into oracle/_ref, through oracle/capture_golden.py's own `case` and
`run_case`, with the settings of hex_p4_n3_deformed (deformed periodic box, amp 0.15, one step) on a 2^3 box.  The P7
file drops the states after the first four RK stages, so that it stays below the 1 MiB a committed file may have; the
operators, the metrics, the first stage's divergence and the state after the step are kept.  Nothing under
oracle/ is written: run_case works in a temporary directory and writes tests/golden, and no bytecode cache is left.

    python tools/capture_hex_high_order.py            # both
    python tools/capture_hex_high_order.py hex_p6_deformed
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True  # (importing capture_golden would otherwise leave oracle/__pycache__)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from capture_golden import case, run_case  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MAX_BYTES = 1 << 20

CASES = [
    (case("hex_p6_deformed", n=2, amp=0.15, level=1, order=6, steps=1), []),
    (case("hex_p7_deformed", n=2, amp=0.15, level=1, order=7, steps=1),
     ["u_step0_stage0", "u_step0_stage1", "u_step0_stage2", "u_step0_stage3"]),
]


def capture(c, drop):
    run_case(c)
    out = os.path.join(GOLDEN, c["name"] + ".npz")
    if drop:
        arrs = {k: v for k, v in np.load(out).items() if k not in drop}
        np.savez_compressed(out, **arrs)
    size = os.path.getsize(out)
    if size > MAX_BYTES:
        raise SystemExit("%s: %d bytes, more than a committed file may have" % (out, size))
    print("%-24s %8.1f kB after dropping %s" % (c["name"], size / 1e3, drop or "nothing"))


if __name__ == "__main__":
    want = sys.argv[1:]
    for c, drop in CASES:
        if not want or c["name"] in want:
            capture(c, drop)
