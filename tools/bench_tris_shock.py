#!/usr/bin/env python3
"""Shock capturing on triangles at bench size: what folding the filter into the 2-D simplex stage's update kernel buys.

The workload is a fixture of tests/golden/tris_shock (ts_p1_n4, ts_p3_n4, ts_p5_n2: the genuine reference's arrays and the numpy
operators of hfx.tri_shock_operators) tiled to about 10^6 elements, as tools/bench_tris.py tiles it.  s0 is found by bisection so
that about a third of the elements is filtered per stage on average over the stages of the timed loop (measured call by call with
the filter at work: it lowers the sensors of the stages behind it): the filtered lanes are the divergent part.  The share of every
stage is reported.  Loops alternating on the same mesh, every timed loop from the same initial state; a host clock around a loop that
ends in a synchronise; median (min - max) over the repeats, in ms per RK stage:

  a   fused 4, the filter folded into the update kernel (the default)
  b   fused 4 with option fold_shock 0: the SHOCK = false update kernel and the per-method filter behind every stage
  c   fused 0 with the per-method filter: what ran for this case before the fold, which refused a and b
  d   fused 4 on a block WITHOUT shock capturing; with --parent-lib also on that build of libhfx.so (the commit before), alternately:
      the SHOCK = false instantiation must be the kernel it was

Before anything is timed the legs' states after one step are compared (a against c at 1e-11, a against b at 1e-12).  One JSON line
per case.

    python tools/bench_tris_shock.py [--elements 1000000] [--steps 2] [--repeats 5] [--cases ts_p3_n4 ...] [--parent-lib PATH]
"""
import argparse
import importlib.util
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
import tri_shock_util as TS  # noqa: E402

CASES = ["ts_p1_n4", "ts_p3_n4", "ts_p5_n2"]


def other_build(path):
    """the Python layer once more, bound to another build of the library"""
    spec = importlib.util.spec_from_file_location("hfx_parent", hfx.__file__.replace(".pyc", ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.LIB_PATH = os.path.abspath(path)
    return m


def build(H, ctx, d, shock_s0=None):
    sz = [int(v) for v in d["sizes"]]
    ctx.set_params(H.params_from(d))
    e = H.Eles(ctx, sz[:5], d, ele_type=sz[6], order=sz[5])
    faces = [H.IntInters(ctx, e, e, d["int%d_L" % t], d["int%d_R" % t]) for t in range(3) if "int%d_L" % t in d]
    if shock_s0 is not None:
        register(e, d, shock_s0)
    return e, faces


def register(e, d, s0):
    e.set_shock_capture(d["inv_vandermonde"], d["exp_filter"], d["norm_basis_persson"], d["persson_high_modes"], s0,
                        int(np.ravel(d["shock_det_field"])[0]))


def stage_sensors(e, faces, d, u_init, s0, steps):
    """the sensors of every stage of `steps` steps with the filter at s0, call by call -> (steps * stages, n_eles)"""
    register(e, d, s0)
    e.upload(hfx.DISU_UPTS0, u_init)
    nstage, adv = int(d["sizes"][7]), int(np.ravel(d["adv_type"])[0])
    out = []
    for st in range(steps):
        for rk in range(nstage):
            hfx.CalcResidual(e, faces)
            e.AdvanceSolution(rk, adv)
            e.shock_capture()
            out.append(e.download(hfx.SENSOR))
    return np.array(out)


def timed(H, ctx, e, faces, u_init, steps, fused):
    e.upload(H.DISU_UPTS0, u_init)
    ctx.synchronize()
    t0 = time.perf_counter()
    H.run_steps_blocks([e], faces, steps, fused=fused)
    ctx.synchronize()
    return time.perf_counter() - t0


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


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
        small = TS.load(name)
        ne0, nstage = int(small["sizes"][0]), int(small["sizes"][7])
        d = G.tile(small, max(1, (args.elements + ne0 - 1) // ne0))
        ne, u0 = int(d["sizes"][0]), d["u_init"]
        es, fs = build(hfx, ctx, d, shock_s0=float("inf"))
        # s0: about a third of the elements filtered per stage, on average over the stages of the timed loop.  The filter lowers
        # the sensors of the stages behind it, so the share is measured with the filter at work
        free = stage_sensors(es, fs, d, u0, float("inf"), args.steps)
        lo, hi, best = float(np.log(free.min())), float(np.log(free.max())), None
        for _ in range(12):  # bisection on log s0 (a lower threshold filters more, up to the feedback)
            s0 = float(np.exp(0.5 * (lo + hi)))
            mean = float((stage_sensors(es, fs, d, u0, s0, args.steps) >= s0).mean())
            if best is None or abs(mean - 1.0 / 3.0) < abs(best[1] - 1.0 / 3.0):
                best = (s0, mean)
            lo, hi = (lo, np.log(s0)) if mean < 1.0 / 3.0 else (np.log(s0), hi)
        s0 = best[0]
        per_stage = (stage_sensors(es, fs, d, u0, s0, args.steps) >= s0).mean(axis=1)
        en, fn = build(hfx, ctx, d)
        ep, fp = build(P, pctx, d) if P else (None, None)

        def leg(which):
            if which in "abc":
                ctx.set_option("fold_shock", int(which != "b"))
                return hfx, ctx, es, fs, 0 if which == "c" else 4
            return (hfx, ctx, en, fn, 4) if which == "d" else (P, pctx, ep, fp, 4)

        legs = ["a", "b", "c", "d"] + (["d_parent"] if P else [])
        states, share = {}, {}
        for w in legs:  # (also the warm-up of every kernel of the leg)
            H, c, e, f, fused = leg(w)
            timed(H, c, e, f, u0, 1, fused)
            states[w] = e.download(H.DISU_UPTS0)
            assert e.check_nan() == -1
            if w in "abc":
                share[w] = float((e.download(hfx.SENSOR) >= s0).mean())
        rel = lambda x, y: float(np.abs(states[x] - states[y]).max() / np.abs(states[y]).max())
        agree = {"a_c": rel("a", "c"), "a_b": rel("a", "b")}
        assert agree["a_c"] < 1e-11 and agree["a_b"] < 1e-12, agree
        if P:
            agree["d_parent"] = rel("d", "d_parent")
            assert agree["d_parent"] == 0.0, agree  # (the same kernel: the same bits)
        ctx.set_option("fold_shock", 1)
        plan = es.simplex2d_shock_plan()
        ms = {w: [] for w in legs}
        for r in range(args.repeats):
            for w in legs:  # alternating
                H, c, e, f, fused = leg(w)
                ms[w].append(1e3 * timed(H, c, e, f, u0, args.steps, fused) / (args.steps * nstage))
        ctx.set_option("fold_shock", 1)
        k_a, names = hfx.time_general_kernels([es], fs, 10)
        k_d, _ = hfx.time_general_kernels([en], fn, 10)
        names = names.split(",")
        med = {w: float(np.median(v)) for w, v in ms.items()}
        nu = int(d["sizes"][1])
        out = {"case": name, "n_eles": ne, "n_upts": nu, "n_fpts": int(d["sizes"][2]), "s0": s0, "filtered_share_per_stage": [round(float(x), 3) for x in per_stage],
               "filtered_share_mean": round(float(per_stage.mean()), 3), "filtered_share_after_one_step": share,
               "shock_plan": plan, "update_lds_without": en.simplex2d_plan()["update_lds"], "states_agree": agree,
               "ms_per_stage": {w: summary(v) for w, v in ms.items()},
               "b_over_a": round(med["b"] / med["a"], 3), "c_over_a": round(med["c"] / med["a"], 3), "a_over_d": round(med["a"] / med["d"], 3),
               "kernel_ms_a": {n: round(k_a[i], 4) for i, n in enumerate(names)},
               "kernel_ms_d": {n: round(k_d[i], 4) for i, n in enumerate(names)},
               "filter_hbm_bytes_per_element_and_stage": 8,
               "filter_lds_multiply_adds_per_element": {"modal": nu * nu, "filtered_elements": 4 * nu * nu}}
        if P:
            out["d_over_d_parent"] = round(med["d"] / med["d_parent"], 4)
        print(json.dumps(out), flush=True)
        for x, fx in ((es, fs), (en, fn)) + (((ep, fp),) if P else ()):
            for f in fx:
                f.close()
            x.close()
    ctx.close()
    if pctx:
        pctx.close()


if __name__ == "__main__":
    main()
