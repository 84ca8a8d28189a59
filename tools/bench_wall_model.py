#!/usr/bin/env python3
"""What the wall model costs: the 32 x 32 x 8 channel of P4 hexahedra of tools/bench_wall_force.py (2 048 wall faces of 25 flux
points between an isothermal and an adiabatic wall), once with `use_wm 0` on both walls -- the yardstick: the LDG wall flux from
the gradient -- and once with `use_wm 1` and Werner-Wengle (`--model 2`: Breuer-Rodi).  Timed on the same build, the two cases
alternating round by round in one process:
  - the viscous boundary sweep (hfx_bdy_inters_evaluate_boundaryConditions_viscFlux), `--sweeps` calls back to back between two
    synchronisations, per call; with the model that is two launches (the faces without a model, then the compacted model faces);
  - one time step of hfx_run_steps(..., 3).
Medians over the rounds after one warm-up round.  The numbers the state takes mean nothing here (the sweep accumulates into
norm_tconf_fpts over and over), only the time does.  No pass mark: the yardstick is the use_wm 0 row.

    python tools/bench_wall_model.py [--cells 32 32 8] [--order 4] [--model 1] [--rounds 9] [--sweeps 50] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hifiles-solver_amd"))

import hfx  # noqa: E402
import hfx_host as H  # noqa: E402


def make(cells, order, model, use_wm):
    bcs = [{"type": "isotherm_wall", "T_static": 310.0, "u": 3.0, "use_wm": use_wm}, {"type": "adiabat_wall", "v": -2.0, "use_wm": use_wm}]
    case = H.Case(cells, order=order, amp=0.05, mu_gas=4e-4, wall_model=model, bcs=bcs, sides={"z-": 0, "z+": 1})
    case.set_deferred(False)
    case.to_device(0)
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs=3, default=[32, 32, 8])
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--model", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--sweeps", type=int, default=50)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib = hfx.lib()
    cases = {0: make(args.cells, args.order, args.model, 0), 1: make(args.cells, args.order, args.model, 1)}
    rows = {k: dict(sweep_ms=[], step_ms=[]) for k in cases}
    n_model = {}
    for k, case in cases.items():
        ctx, e, f, nb = case.handles()
        hfx.check(lib.hfx_CalcResidual(e, f, C.c_int(nb)))  # every array the sweep reads holds a residual's values
        n_model[k] = case.wall_model_points()[3]
    for r in range(args.rounds + 1):
        for k, case in cases.items():
            ctx, e, f, nb = case.handles()
            bdy = f[nb - 1]  # (the mirror lists the interior block first, the boundary block last)
            hfx.check(lib.hfx_ctx_synchronize(ctx))
            t0 = time.perf_counter()
            for _ in range(args.sweeps):
                hfx.check(lib.hfx_bdy_inters_evaluate_boundaryConditions_viscFlux(C.c_void_p(bdy), C.c_double(0.0)))
            hfx.check(lib.hfx_ctx_synchronize(ctx))
            t1 = time.perf_counter()
            hfx.check(lib.hfx_run_steps(e, f, C.c_int(nb), C.c_int(1), C.c_int(3)))
            hfx.check(lib.hfx_ctx_synchronize(ctx))
            t2 = time.perf_counter()
            if r > 0:
                rows[k]["sweep_ms"].append(1e3 * (t1 - t0) / args.sweeps)
                rows[k]["step_ms"].append(1e3 * (t2 - t1))
    out = []
    for k in (0, 1):
        s, t = rows[k]["sweep_ms"], rows[k]["step_ms"]
        res = dict(use_wm=k, wall_model=args.model, cells=args.cells, order=args.order, model_faces=n_model[k], rounds=args.rounds,
                   sweep_ms=statistics.median(s), sweep_min_ms=min(s), sweep_max_ms=max(s),
                   step_ms=statistics.median(t), step_min_ms=min(t), step_max_ms=max(t))
        out.append(res)
        print("use_wm %d (%4d model faces): viscous boundary sweep %.4f ms (min %.4f, max %.4f); one step of hfx_run_steps(.., 3) %.3f ms "
              "(min %.3f, max %.3f)" % (k, n_model[k], res["sweep_ms"], res["sweep_min_ms"], res["sweep_max_ms"], res["step_ms"],
                                        res["step_min_ms"], res["step_max_ms"]))
    for case in cases.values():
        case.close()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
