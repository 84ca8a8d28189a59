#!/usr/bin/env python3
"""Over-integration on triangles at bench size: what forming the de-aliased flux inside the 2-D simplex stage's element kernel buys.

The workload is a fixture of tests/golden/tris_overint (to_p1_o3, to_p3, to_p5: the genuine reference's arrays, 10 / 28 / 36 cubature
points) tiled to about 10^6 elements, as tools/bench_tris.py tiles it.  Loops alternating on the same mesh, every timed loop from the
same initial state; a host clock around a loop that ends in a synchronise; median (min - max) over the repeats, in ms per RK stage:

  a   fused 4, the over-integration folded into the element kernel (the default)
  b   fused 4 with option fold_over_int 0: hfx_eles_evaluate_invFlux_over_int in front of the element kernel, which reads tdisf_upts
  c   fused 0, per method: what ran for this case before the fold, which refused a and b
  d   fused 4 on the same mesh WITHOUT over-integration; with --parent-lib also on that build of libhfx.so (the commit before),
      alternately: the instantiation without over-integration must be the kernel it was

Before anything is timed the legs' states after one step are compared (a against c and a against b at 1e-11; d against the parent
build bit for bit).  One JSON line per case.

    python tools/bench_tris_overint.py [--elements 1000000] [--steps 2] [--repeats 5] [--cases to_p3 ...] [--parent-lib PATH]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hifiles-solver_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hfx  # noqa: E402
import general_util as G  # noqa: E402
import tri_overint_util as TO  # noqa: E402
from bench_tris_shock import other_build, summary, timed  # noqa: E402

CASES = ["to_p1_o3", "to_p3", "to_p5"]


def build(H, ctx, d, over_int):
    sz = [int(v) for v in d["sizes"]]
    ctx.set_params(H.params_from(d))
    e = H.Eles(ctx, sz[:5], d, ele_type=sz[6], order=sz[5])
    faces = [H.IntInters(ctx, e, e, d["int%d_L" % t], d["int%d_R" % t]) for t in range(3) if "int%d_L" % t in d]
    if over_int:
        e.set_over_int(d["opp_over_int_cubpts"], d["over_int_filter"], d["JGinv_over_int_cubpts"])
    return e, faces


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", nargs="*", default=CASES)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    P = other_build(args.parent_lib) if args.parent_lib else None
    ctx = hfx.Context(0)
    pctx = P.Context(0) if P else None
    for name in args.cases:
        small = TO.load(name)
        ne0, nstage = int(small["sizes"][0]), int(small["sizes"][7])
        d = G.tile(small, max(1, (args.elements + ne0 - 1) // ne0))
        ne, u0 = int(d["sizes"][0]), d["u_init"]
        eo, fo = build(hfx, ctx, d, True)
        en, fn = build(hfx, ctx, d, False)
        ep, fp = build(P, pctx, d, False) if P else (None, None)

        def leg(which):
            if which in "abc":
                ctx.set_option("fold_over_int", int(which != "b"))
                return hfx, ctx, eo, fo, 0 if which == "c" else 4
            return (hfx, ctx, en, fn, 4) if which == "d" else (P, pctx, ep, fp, 4)

        legs = ["a", "b", "c", "d"] + (["d_parent"] if P else [])
        states, plans = {}, {}
        for w in legs:  # (also the warm-up of every kernel of the leg)
            H, c, e, f, fused = leg(w)
            timed(H, c, e, f, u0, 1, fused)
            states[w] = e.download(H.DISU_UPTS0)
            assert e.check_nan() == -1
            if w in "ab":
                plans[w] = e.simplex2d_over_int_plan()
        rel = lambda x, y: float(np.abs(states[x] - states[y]).max() / np.abs(states[y]).max())
        agree = {"a_c": rel("a", "c"), "a_b": rel("a", "b"), "a_d": rel("a", "d")}
        assert agree["a_c"] < 1e-11 and agree["a_b"] < 1e-11, agree
        assert plans["a"]["folded"] == 1 and plans["b"]["folded"] == 0, plans
        if P:
            agree["d_parent"] = rel("d", "d_parent")
            assert agree["d_parent"] == 0.0, agree  # (the same kernel: the same bits)
        ms = {w: [] for w in legs}
        for r in range(args.repeats):
            for w in legs:  # alternating
                H, c, e, f, fused = leg(w)
                ms[w].append(1e3 * timed(H, c, e, f, u0, args.steps, fused) / (args.steps * nstage))
        kernels = {}
        for w, (e, f, fold) in {"a": (eo, fo, 1), "b": (eo, fo, 0), "d": (en, fn, 1)}.items():
            ctx.set_option("fold_over_int", fold)
            k, names = hfx.time_general_kernels([e], f, 10)
            kernels[w] = {n: round(k[i if i < 4 else 4], 4) for i, n in enumerate(names.split(","))}
        ctx.set_option("fold_over_int", 1)
        med = {w: float(np.median(v)) for w, v in ms.items()}
        nu, nc = int(d["sizes"][1]), plans["a"]["n_cubpts"]
        out = {"case": name, "n_eles": ne, "n_upts": nu, "n_fpts": int(d["sizes"][2]), "viscous": int(np.ravel(d["viscous"])[0]),
               "over_int_plan": plans["a"], "states_agree": agree, "state_moved_by_over_int_after_one_step": agree["a_d"],
               "ms_per_stage": {w: summary(v) for w, v in ms.items()},
               "b_over_a": round(med["b"] / med["a"], 3), "c_over_a": round(med["c"] / med["a"], 3), "a_over_d": round(med["a"] / med["d"], 3),
               "kernel_ms": kernels, "fold_hbm_bytes_per_element_and_stage": 8 * 4 * nc,
               "fold_lds_multiply_adds_per_element": 12 * nc * nu}
        if P:
            out["d_over_d_parent"] = round(med["d"] / med["d_parent"], 4)
        print(json.dumps(out), flush=True)
        for x, fx in ((eo, fo), (en, fn)) + (((ep, fp),) if P else ()):
            for f in fx:
                f.close()
            x.close()
    ctx.close()
    if pctx:
        pctx.close()


if __name__ == "__main__":
    main()
