#!/usr/bin/env python3
"""The LES closure on triangles at bench size: what evaluating it inside the 2-D simplex stage's element kernel buys.

The workload is a fixture of tests/golden/tris_les (tl_p1_wale, tl_p3_wale, tl_p5_wale: the genuine reference's arrays, the WALE
closure) tiled to about 10^6 elements, as tools/bench_tris.py tiles it.  Loops alternating on the same mesh, every timed loop from the
same initial state; a host clock around a loop that ends in a synchronise; median (min - max) over the repeats, in ms per RK stage:

  a   fused 4 with the closure: the element kernel's LES form
  b   fused 0 with the closure, per method: what ran for this case before, since the stage refused it
  c   fused 4 on the same mesh WITHOUT a closure; with --parent-lib also on that build of libhfx.so (the commit before), alternately:
      the instantiation without a closure must be the kernel it was

Before anything is timed the legs' states after one step are compared (a against b at 1e-11; c against the parent build bit for
bit).  One JSON line per case.

    python tools/bench_tris_les.py [--elements 1000000] [--steps 2] [--repeats 5] [--cases tl_p3_wale ...] [--parent-lib PATH]
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
import tri_les_util as TL  # noqa: E402
from bench_tris_shock import other_build, summary, timed  # noqa: E402

CASES = ["tl_p1_wale", "tl_p3_wale", "tl_p5_wale"]


def build(H, ctx, d, les):
    sz = [int(v) for v in d["sizes"]]
    ctx.set_params(H.params_from(d))
    e = H.Eles(ctx, sz[:5], d, ele_type=sz[6], order=sz[5])
    faces = [H.IntInters(ctx, e, e, d["int%d_L" % t], d["int%d_R" % t]) for t in range(3) if "int%d_L" % t in d]
    if les:
        e.set_les(int(TL.scalar(d, "SGS_model")), TL.scalar(d, "C_s"), TL.scalar(d, "filter_ratio"), TL.scalar(d, "Kappa"),
                  TL.scalar(d, "prandtl_t"), d["Jacobian_fpts"])
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
        small = TL.load(name)
        ne0, nstage = int(small["sizes"][0]), int(small["sizes"][7])
        d = G.tile(small, max(1, (args.elements + ne0 - 1) // ne0))
        ne, u0 = int(d["sizes"][0]), d["u_init"]
        el, fl = build(hfx, ctx, d, True)
        en, fn = build(hfx, ctx, d, False)
        ep, fp = build(P, pctx, d, False) if P else (None, None)

        def leg(which):
            if which in "ab":
                return hfx, ctx, el, fl, 4 if which == "a" else 0
            return (hfx, ctx, en, fn, 4) if which == "c" else (P, pctx, ep, fp, 4)

        legs = ["a", "b", "c"] + (["c_parent"] if P else [])
        states = {}
        for w in legs:  # (also the warm-up of every kernel of the leg)
            H, c, e, f, fused = leg(w)
            timed(H, c, e, f, u0, 1, fused)
            states[w] = e.download(H.DISU_UPTS0)
            assert e.check_nan() == -1
            if w == "a":
                plan = e.simplex2d_les_plan()
        rel = lambda x, y: float(np.abs(states[x] - states[y]).max() / np.abs(states[y]).max())
        agree = {"a_b": rel("a", "b"), "a_c": rel("a", "c")}
        assert agree["a_b"] < 1e-11, agree
        assert plan["les"] == 1, plan
        if P:
            agree["c_parent"] = rel("c", "c_parent")
            assert agree["c_parent"] == 0.0, agree  # (the same kernel: the same bits)
        ms = {w: [] for w in legs}
        for r in range(args.repeats):
            for w in legs:  # alternating
                H, c, e, f, fused = leg(w)
                ms[w].append(1e3 * timed(H, c, e, f, u0, args.steps, fused) / (args.steps * nstage))
        kernels = {}
        for w, (e, f) in {"a": (el, fl), "c": (en, fn)}.items():
            k, names = hfx.time_general_kernels([e], f, 10)
            kernels[w] = {n: round(k[i], 4) for i, n in enumerate(names.split(","))}
        med = {w: float(np.median(v)) for w, v in ms.items()}
        out = {"case": name, "n_eles": ne, "n_upts": int(d["sizes"][1]), "n_fpts": int(d["sizes"][2]), "les_plan": plan,
               "states_agree": agree, "state_moved_by_the_closure_after_one_step": agree["a_c"],
               "ms_per_stage": {w: summary(v) for w, v in ms.items()},
               "b_over_a": round(med["b"] / med["a"], 3), "a_over_c": round(med["a"] / med["c"], 3), "kernel_ms": kernels}
        if P:
            out["c_over_c_parent"] = round(med["c"] / med["c_parent"], 4)
        print(json.dumps(out), flush=True)
        for x, fx in ((el, fl), (en, fn)) + (((ep, fp),) if P else ()):
            for f in fx:
                f.close()
            x.close()
    ctx.close()
    if pctx:
        pctx.close()


if __name__ == "__main__":
    main()
