#!/usr/bin/env python3
"""Partitioned triangles at bench size: the 2-D simplex fused stage on a partitioned block (hfx_run_steps_partitioned_blocks,
interior groups first) against the per-method partitioned call sequence (the reference's calls with send_* / receive_*, the only way
before the stage took partition faces) and against the undivided fused-4 loop on the same mesh, alternating in one visit.

The mesh is a fixture of the genuine reference tiled to about 10^6 elements as tools/bench_tris.py tiles it (identical, mutually
disconnected boxes).  Every --cut-every'th box is cut into three virtual parts (tests/test_tris_partition_oracle.py's seeded
random walk) whose faces become partition faces that the one rank exchanges with itself over libhfx's RCCL transport
(ragged_partition.cut_self); the other boxes stay whole, so that -- as on a real partition, where the cut is a surface -- most groups of
elements are interior groups.  Per case one JSON line: ms per RK stage of the three loops (median and spread over the repeats, a host
clock around a loop that ends in a synchronise), the ratios, and from hfx_simplex2d_partition_plan the share of interior groups.
The new loop's state after a step is compared with the per-method sequence's (relative to max |u|) before anything is printed.

    python tools/bench_tris_partitioned.py [--elements 1000000] [--steps 2] [--repeats 5] [--cut-every 8] [--cases ...]
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
import ragged_partition as RP  # noqa: E402
import tri_util as T  # noqa: E402
from test_tris_partition_oracle import VIRTUAL3, grow_parts  # noqa: E402

CASES = ["tri_p3_n4_deformed", "tri_p1_n4_deformed", "tri_p5_n2_deformed"]


def build(ctx, d):
    sz = [int(v) for v in d["sizes"]]
    ctx.set_params(hfx.params_from(d))
    e = hfx.Eles(ctx, sz[:5], d, ele_type=sz[6], order=sz[5])
    e.upload(hfx.DISU_UPTS0, d["u_init"])
    faces = [hfx.IntInters(ctx, e, e, d["int%d_L" % t], d["int%d_R" % t]) for t in range(3) if "int%d_L" % t in d]
    return e, faces


def per_method_stage(e, ints, M, comm, rk, adv):
    """CalcResidual's order with the partition-face calls (src/solver.cpp:59-221), then AdvanceSolution"""
    e.extrapolate_solution()
    for f in M: f.send_solution(comm)
    e.calculate_gradient()
    e.evaluate_invFlux()
    for f in ints: f.calculate_common_invFlux()
    for f in M: f.receive_solution(comm)
    for f in M: f.calculate_common_invFlux()
    e.correct_gradient()
    for f in M: f.send_corrected_gradient(comm)
    e.evaluate_viscFlux()
    e.extrapolate_totalFlux()
    e.calculate_divergence()
    for f in ints: f.calculate_common_viscFlux()
    for f in M: f.receive_corrected_gradient(comm)
    for f in M: f.calculate_common_viscFlux()
    e.calculate_corrected_divergence()
    e.AdvanceSolution(rk, adv)


def spread(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cut-every", type=int, default=8)
    ap.add_argument("--cases", nargs="*", default=CASES)
    args = ap.parse_args()
    ctx = hfx.Context(0)
    comm = hfx.Comm(ctx.h, hfx.comm_unique_id(), 1, 0)
    for name in args.cases:
        small = T.load(name)
        ne0, nstage, adv = int(small["sizes"][0]), int(small["sizes"][7]), int(np.ravel(small["adv_type"])[0])
        tiles = max(1, (args.elements + ne0 - 1) // ne0)
        d = G.tile(small, tiles)
        ne = int(d["sizes"][0])
        # the virtual parts: the small box's part vector in every cut_every'th box, part 0 elsewhere
        part = np.zeros((tiles, ne0), dtype=np.int64)
        part[::args.cut_every] = grow_parts(small, *VIRTUAL3)
        reg, L, Rlut, seg = RP.cut_self(d, part.reshape(-1))

        whole, whole_faces = build(ctx, d)      # the undivided loop
        e, ints = build(ctx, reg)               # the partitioned block, fused
        m, m_ints = build(ctx, reg)             # the partitioned block, per method
        M = [hfx.MpiInters(ctx, e, L, Rlut)]
        Mm = [hfx.MpiInters(ctx, m, L, Rlut)]
        for f in M + Mm:
            f.set_neighbours(seg)

        def run(which, steps):
            ctx.synchronize()
            t0 = time.perf_counter()
            if which == "partitioned_fused":
                hfx.run_steps_partitioned_blocks([e], ints, M, comm, steps)
            elif which == "undivided_fused":
                hfx.run_steps_blocks([whole], whole_faces, steps, fused=4)
            else:
                for _ in range(steps):
                    for rk in range(nstage):
                        per_method_stage(m, m_ints, Mm, comm, rk, adv)
            ctx.synchronize()
            return 1e3 * (time.perf_counter() - t0) / (steps * nstage)

        loops = ("partitioned_per_method", "partitioned_fused", "undivided_fused")
        for w in loops:  # one step each from the same state: the warm-up, and the results must agree before the times mean anything
            run(w, 1)
        ref = m.download(hfx.DISU_UPTS0)
        agree = float(np.abs(e.download(hfx.DISU_UPTS0) - ref).max() / np.abs(ref).max())
        agree_whole = float(np.abs(whole.download(hfx.DISU_UPTS0) - ref).max() / np.abs(ref).max())
        assert agree < 1e-11 and agree_whole < 1e-11, (agree, agree_whole)
        assert e.check_nan() == -1
        ms = {w: [] for w in loops}
        for r in range(args.repeats):
            for w in loops:  # alternating
                ms[w].append(run(w, args.steps))
        med = {w: float(np.median(v)) for w, v in ms.items()}
        pp = e.simplex2d_partition_plan()
        print(json.dumps({
            "case": name, "n_eles": ne, "n_partition_faces": int(L.shape[1]), "cut_every": args.cut_every, "plan": e.simplex2d_plan(),
            "partition_plan": pp,
            "interior_group_share": round(pp["interior_groups"] / max(1, pp["interior_groups"] + pp["partition_groups"]), 4),
            "states_agree": agree, "states_agree_undivided": agree_whole,
            "ms_per_stage": {w: spread(ms[w]) for w in loops},
            "speedup_over_per_method": round(med["partitioned_per_method"] / med["partitioned_fused"], 3),
            "overhead_over_undivided": round(med["partitioned_fused"] / med["undivided_fused"], 3),
        }), flush=True)
        for f in whole_faces + ints + m_ints + M + Mm:
            f.close()
        for x in (whole, e, m):
            x.close()
    comm.close()
    ctx.close()


if __name__ == "__main__":
    main()
