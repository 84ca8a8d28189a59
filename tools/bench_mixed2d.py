#!/usr/bin/env python3
"""Mixed quadrilateral / triangle meshes at bench size: the 2-D simplex fused stage over several blocks (option blocks_2d 1,
hfx_run_steps_blocks(..., fused = 4), csrc/simplex2d.hip) in one visit, legs alternating.

The workload is a fixture of the genuine reference (tests/golden/mixed2d) tiled to about 10^6 elements (tests/mixed2d_util.py:
tile_mixed -- identical, mutually disconnected boxes: the same per-element and per-face work as one large mesh, every array at full
size in HBM).  P3 runs mx_p3_walls (quadrilateral rows on both walls, triangles between, a third of the elements quadrilaterals),
P1 and P4 the periodic mx_p1_n4 / mx_p4_n4.  Per case one JSON line with, each as median / min / max ms per RK stage over the repeats
(a host clock around a loop that ends in a synchronise):

  mixed      fused 4 with blocks_2d 1 against fused 0 on the same mesh: the ratio is the result
  gather     the same fused 4 with gather_delta 1 against 0: what the delta launches inside the blocks cost
  quads      the quadrilateral class alone (cut out of the tiled fixture, its cut faces boundary faces): the dense stage
             (blocks_2d 1, fused 4) against the sum-factorised split stage (fused 3) -- the price of the dense form
  kernels    hfx_time_general_kernels and hfx_general_kernel_bytes of the mixed stage

The all-triangle comparison against another build is tools/bench_tris.py run from either tree.  Both paths' final states are compared
(relative to max |u|) before anything is printed.

    python tools/bench_mixed2d.py [--elements 1000000] [--steps 2] [--repeats 5] [--orders 1 3 4]
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
import mixed2d_util as X  # noqa: E402
import mixed_util as MU  # noqa: E402

CASES = {1: "mx_p1_n4", 3: "mx_p3_walls", 4: "mx_p4_n4"}


def build_mixed(ctx, d):
    classes, per, faces, bdy = MU.split(d)
    ctx.set_params(hfx.params_from(per[classes[0]]))
    E = {}
    for c in classes:
        sz = [int(v) for v in per[c]["sizes"]]
        E[c] = hfx.Eles(ctx, sz[:5], per[c], ele_type=sz[6], order=sz[5])
    F = [hfx.IntInters(ctx, E[a], E[b], L, R) for a, b, L, R in faces]
    for a, L, ids in bdy:
        F.append(hfx.BdyInters(ctx, E[a], L, ids, hfx.bc_records(d["bc_flags"], d["bc_params"]), float(np.ravel(d["bc_R_ref"])[0]), 0))
    return [E[c] for c in classes], F, [per[c]["u_init"] for c in classes]


def build_single(ctx, d):
    sz = [int(v) for v in d["sizes"]]
    ctx.set_params(hfx.params_from(d))
    e = hfx.Eles(ctx, sz[:5], d, ele_type=sz[6], order=sz[5])
    F = [hfx.IntInters(ctx, e, e, d["int%d_L" % t], d["int%d_R" % t]) for t in range(3) if "int%d_L" % t in d]
    for t in range(3):
        if "bdy%d_L" % t in d:
            F.append(hfx.BdyInters(ctx, e, d["bdy%d_L" % t], d["bdy%d_id" % t], hfx.bc_records(d["bc_flags"], d["bc_params"]),
                                   float(np.ravel(d["bc_R_ref"])[0]), 0))
    return [e], F, [d["u_init"]]


def reset(blocks, F, u0):
    """the initial state, and the pressure ramp of an inlet at its start (the step loops advance it after every step)"""
    for e, u in zip(blocks, u0):
        e.upload(hfx.DISU_UPTS0, u)
    for f in F:
        if isinstance(f, hfx.BdyInters):
            f.set_ramp_counter(0)


def timed(ctx, blocks, F, steps, fused):
    ctx.synchronize()
    t0 = time.perf_counter()
    hfx.run_steps_blocks(blocks, F, steps, fused=fused)
    ctx.synchronize()
    return time.perf_counter() - t0


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def legs(ctx, blocks, F, u0, steps, nstage, repeats, a, b):
    """two legs (name, fused, options) alternating -> {name: ms per stage}, and their states after one step agree"""
    states, ms = {}, {a[0]: [], b[0]: []}
    for name, fused, opts in (a, b):
        for k, v in opts:
            ctx.set_option(k, v)
        reset(blocks, F, u0)
        hfx.run_steps_blocks(blocks, F, 1, fused=fused)  # (also the warm-up of every kernel of the leg)
        states[name] = [e.download(hfx.DISU_UPTS0) for e in blocks]
        assert all(e.check_nan() == -1 for e in blocks)
    agree = max(float(np.abs(x - y).max() / np.abs(y).max()) for x, y in zip(states[a[0]], states[b[0]]))
    assert agree < 1e-11, agree
    for r in range(repeats):
        for name, fused, opts in (a, b):
            for k, v in opts:
                ctx.set_option(k, v)
            ms[name].append(1e3 * timed(ctx, blocks, F, steps, fused) / (steps * nstage))
    return {k: stats(v) for k, v in ms.items()}, agree


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--orders", nargs="*", type=int, default=[1, 3, 4])
    args = ap.parse_args()
    for order in args.orders:
        small = X.load(CASES[order])
        ne0 = X.sizes(small, 0)[0] + X.sizes(small, 1)[0]
        nstage = X.sizes(small, 0)[7]
        d = X.tile_mixed(small, max(1, (args.elements + ne0 - 1) // ne0))
        ctx = hfx.Context(0)
        ctx.set_option("blocks_2d", 1)
        blocks, F, u0 = build_mixed(ctx, d)
        out = {"case": CASES[order], "order": order, "triangles": X.sizes(d, 0)[0], "quadrilaterals": X.sizes(d, 1)[0]}
        out["mixed_ms_per_stage"], out["mixed_states_agree"] = legs(ctx, blocks, F, u0, args.steps, nstage, args.repeats,
                                                                    ("fused0", 0, []), ("fused4", 4, [("gather_delta", 1)]))
        out["mixed_speedup"] = round(out["mixed_ms_per_stage"]["fused0"]["median"] / out["mixed_ms_per_stage"]["fused4"]["median"], 3)
        out["gather_ms_per_stage"], _ = legs(ctx, blocks, F, u0, args.steps, nstage, args.repeats, ("gather0", 4, [("gather_delta", 0)]),
                                             ("gather1", 4, [("gather_delta", 1)]))
        out["stage_plan"] = hfx.simplex2d_stage_plan(blocks)
        out["plans"] = [e.simplex2d_plan() for e in blocks]
        k_ms, k_names = hfx.time_general_kernels(blocks, F, 10)
        by = hfx.general_kernel_bytes(blocks)
        out["kernel_ms"] = {n: round(k_ms[i], 4) for i, n in enumerate(k_names.split(","))}
        out["kernel_GBps"] = {n: round(by[i] / (k_ms[i] * 1e-3) / 1e9, 1) if by[i] > 0 and k_ms[i] > 0 else 0.0 for i, n in enumerate(k_names.split(","))}
        for f in F:
            f.close()
        for e in blocks:
            e.close()
        # the quadrilateral class alone: 12 quadrilaterals of the order's periodic fixture, tiled
        q0 = X.quad_block(order, 12)
        q = G.tile(q0, max(1, (args.elements + 11) // 12))
        blocks, F, u0 = build_single(ctx, q)
        out["quads_ms_per_stage"], out["quads_states_agree"] = legs(ctx, blocks, F, u0, args.steps, nstage, args.repeats, ("fused3", 3, []), ("dense4", 4, []))
        out["quads_dense_over_split"] = round(out["quads_ms_per_stage"]["dense4"]["median"] / out["quads_ms_per_stage"]["fused3"]["median"], 3)
        out["quads_plan"] = blocks[0].simplex2d_plan()
        for f in F:
            f.close()
        blocks[0].close()
        ctx.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
