#!/usr/bin/env python3
"""Triangles at bench size: the 2-D simplex fused stage (hfx_run_steps_blocks(..., fused = 4), csrc/simplex2d.hip) against the
per-method path (fused 0) on the same inputs in one visit, alternating.

The workload is a fixture of the genuine reference (tests/golden/tris/tri_p{1,3,5}_*_deformed.npz: a small periodic box with its
operators, metrics and face tables) tiled to about 10^6 elements: identical, mutually disconnected boxes -- the same per-element and
per-face work as one large mesh, every array at full size in HBM.  Per case one JSON line: ms per RK stage of either path (median
and spread over the repeats, a host clock around a loop that ends in a synchronise), the stage's per-kernel times
(hfx_time_general_kernels, device events), the algorithmic bytes of each kernel (hfx_general_kernel_bytes), their rate, and that
rate relative to the update kernel's.  Both paths' final states are compared (relative to max |u|) before anything is printed.

    python tools/bench_tris.py [--elements 1000000] [--steps 2] [--repeats 5] [--cases tri_p3_n4_deformed ...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hifiles-solver_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hfx  # noqa: E402
import general_util as G  # noqa: E402
import tri_util as T  # noqa: E402

CASES = ["tri_p3_n4_deformed", "tri_p1_n4_deformed", "tri_p5_n2_deformed"]


def build(ctx, d):
    sz = [int(v) for v in d["sizes"]]
    ctx.set_params(hfx.params_from(d))
    e = hfx.Eles(ctx, sz[:5], d, ele_type=sz[6], order=sz[5])
    faces = [hfx.IntInters(ctx, e, e, d["int%d_L" % t], d["int%d_R" % t]) for t in range(3) if "int%d_L" % t in d]
    return e, faces


def timed(ctx, e, faces, steps, fused):
    ctx.synchronize()
    t0 = time.perf_counter()
    hfx.run_steps_blocks([e], faces, steps, fused=fused)
    ctx.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", nargs="*", default=CASES)
    args = ap.parse_args()
    ctx = hfx.Context(0)
    for name in args.cases:
        small = T.load(name)
        ne0, nstage = int(small["sizes"][0]), int(small["sizes"][7])
        d = G.tile(small, max(1, (args.elements + ne0 - 1) // ne0))
        ne = int(d["sizes"][0])
        e, faces = build(ctx, d)
        # both paths from the same state: the results must agree before the times mean anything
        states = {}
        for fused in (0, 4):
            e.upload(hfx.DISU_UPTS0, d["u_init"])
            hfx.run_steps_blocks([e], faces, 1, fused=fused)  # (also the warm-up of every kernel of the path)
            states[fused] = e.download(hfx.DISU_UPTS0)
            assert e.check_nan() == -1
        agree = float(np.abs(states[4] - states[0]).max() / np.abs(states[0]).max())
        assert agree < 1e-11, agree
        ms = {0: [], 4: []}
        for r in range(args.repeats):
            for fused in (0, 4):  # alternating
                ms[fused].append(1e3 * timed(ctx, e, faces, args.steps, fused) / (args.steps * nstage))
        k_ms, k_names = hfx.time_general_kernels([e], faces, 10)
        k_names = k_names.split(",")
        by = hfx.general_kernel_bytes([e])
        rate = [by[i] / (k_ms[i] * 1e-3) / 1e9 if by[i] > 0 else 0.0 for i in range(4)]
        med = {f: float(np.median(v)) for f, v in ms.items()}
        print(json.dumps({
            "case": name, "n_eles": ne, "n_upts": int(d["sizes"][1]), "n_fpts": int(d["sizes"][2]), "plan": e.simplex2d_plan(),
            "states_agree": agree,
            "ms_per_stage_fused0": {"median": round(med[0], 4), "min": round(min(ms[0]), 4), "max": round(max(ms[0]), 4)},
            "ms_per_stage_fused4": {"median": round(med[4], 4), "min": round(min(ms[4]), 4), "max": round(max(ms[4]), 4)},
            "speedup": round(med[0] / med[4], 3),
            "kernel_ms": {n: round(k_ms[i], 4) for i, n in enumerate(k_names)},
            "kernel_MB": {n: round(by[i] / 1e6, 1) for i, n in enumerate(k_names)},
            "kernel_GBps": {n: round(rate[i], 1) for i, n in enumerate(k_names)},
            "GBps_over_update_kernel": {n: round(rate[i] / rate[3], 3) for i, n in enumerate(k_names)},
        }), flush=True)
        for f in faces:
            f.close()
        e.close()
    ctx.close()


if __name__ == "__main__":
    main()
