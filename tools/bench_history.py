#!/usr/bin/env python3
"""What the history monitor costs, one device: the flagship box (32^3 hexahedra, P4, periodic Taylor-Green) for the residual
columns, the 32 x 32 x 8 channel of tools/bench_wall_force.py (P4, an isothermal and an adiabatic wall) for residuals with forces.

  --mode monitor   (this tree's library)
      - the sample on its own (hfx_time_history: the residual kernel, with forces the wall-force kernel, the finishing launch;
        HIP events around back-to-back samples), beside the bytes the residual must move, (n_fields + 1) x 8 x n_upts x n_eles, at
        the HBM rate the update kernel of the fused stage reaches in the same process (hfx_time_fused_kernels slot 3 over
        hfx_fused_kernel_bytes slot 3);
      - ms per step of hfx_run_steps(..., fused 3) without a monitor and with the rows taken inside the loop at monitor_res_freq
        1, 10 and 100 (with viscous forces a sampled step ends with one RK stage call by call).
  --mode by_hand   (any library that has the per-call entry points: run it on the PARENT commit's library through HFX_LIB_DIR)
      what a caller does without the monitor: leave the loop at every sampled step, n_fields calls of hfx_eles_compute_res_upts
      and, on the channel, one hfx_eles_compute_wall_forces -- which after a fused 3 loop is REFUSED on a viscous case (the
      gradient is on chip), so hfx_CalcResidual runs first, as a caller has to, and pairs the forces with the gradient of the
      wrong state.

Each figure is the median of `regions` regions of `steps` steps after a warm-up.

    python tools/bench_history.py --mode monitor [--case tgv|channel] [--steps 100] [--regions 3] [--json out.json]
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

WALLS = dict(bcs=[{"type": "isotherm_wall", "T_static": 310.0, "u": 3.0}, {"type": "adiabat_wall", "v": -2.0}])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["monitor", "by_hand"], required=True)
    ap.add_argument("--case", choices=["tgv", "channel"], default="tgv")
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--freqs", type=int, nargs="*", default=[1, 10, 100])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib = hfx.lib()
    forces = args.case == "channel"
    if forces:
        case = H.Case([32, 32, 8], order=args.order, calc_force=1, area_ref=1.0, nx_c_ic=0.8, ny_c_ic=0.5, nz_c_ic=0.33,
                      sides={"z-": 0, "z+": 1}, **WALLS)
    else:
        case = H.Case(32, order=args.order)
    case.set_deferred(False)
    case.to_device(0)
    ctx, e, f, nb = case.handles()
    n_fields, n_pts = case.n_fields, case.n_upts * case.n_eles
    out = dict(mode=args.mode, case=args.case, order=args.order, n_eles=case.n_eles, steps_per_region=args.steps, regions=args.regions,
               library=os.environ.get("HFX_LIB_DIR", "this tree"), cases=[])

    def run(n):
        hfx.check(lib.hfx_run_steps(e, f, C.c_int(nb), C.c_int(n), C.c_int(3)))

    def region(n):
        hfx.check(lib.hfx_ctx_set_clock(ctx, C.c_double(0.0), C.c_int(0)))
        hfx.check(lib.hfx_ctx_synchronize(ctx))
        t0 = time.perf_counter()
        run(n)
        hfx.check(lib.hfx_ctx_synchronize(ctx))
        return 1e3 * (time.perf_counter() - t0) / n

    v = C.c_double(0)
    fi, fv, cl, cd = (C.c_double * 3)(), (C.c_double * 3)(), C.c_double(0), C.c_double(0)

    def by_hand():
        if forces:  # (the gradient of a fused 3 loop is on chip: the call is refused until a residual has run)
            hfx.check(lib.hfx_CalcResidual(e, f, C.c_int(nb)))
            hfx.check(lib.hfx_eles_compute_wall_forces(e, fi, fv, C.byref(cl), C.byref(cd), None, None))
        for fld in range(n_fields):
            hfx.check(lib.hfx_eles_compute_res_upts(e, C.c_int(2), C.c_int(fld), C.byref(v)))

    def region_by_hand(n, freq):
        hfx.check(lib.hfx_ctx_set_clock(ctx, C.c_double(0.0), C.c_int(0)))
        hfx.check(lib.hfx_ctx_synchronize(ctx))
        t0 = time.perf_counter()
        done = 0
        while done < n:
            nxt = 1 if done == 0 else min(n, (done // freq + 1) * freq)
            run(nxt - done)
            done = nxt
            if done == 1 or done % freq == 0:
                by_hand()
        hfx.check(lib.hfx_ctx_synchronize(ctx))
        return 1e3 * (time.perf_counter() - t0) / n

    def monitor(freq, capacity):
        hfx.check(lib.hfx_ctx_set_history_monitor(ctx, C.c_int(2), C.c_int(1 if forces else 0), C.c_int(freq), C.c_int(capacity)))

    region(2)  # warm-up: the fused tables, the first launches
    if args.mode == "by_hand":
        by_hand()
        hfx.check(lib.hfx_ctx_synchronize(ctx))
        t0 = time.perf_counter()
        for _ in range(10):
            by_hand()
        out["by_hand_ms"] = 1e3 * (time.perf_counter() - t0) / 10
    else:
        run(1)
        monitor(1, 1)
        ms = C.c_double(0)
        if forces:  # (the timing entry point reads the gradient: one residual leaves it)
            hfx.check(lib.hfx_CalcResidual(e, f, C.c_int(nb)))
        hfx.check(lib.hfx_time_history(e, C.c_int(20), C.byref(ms)))
        out["sample_ms"] = ms.value
        if forces:
            hfx.check(lib.hfx_ctx_set_history_monitor(ctx, C.c_int(2), C.c_int(0), C.c_int(1), C.c_int(1)))
            hfx.check(lib.hfx_time_history(e, C.c_int(20), C.byref(ms)))
            out["sample_ms_residuals_alone"] = ms.value
        groups, ppp = C.c_int(0), C.c_int(0)
        hfx.check(lib.hfx_eles_history_launch(e, C.byref(groups), C.byref(ppp)))
        out["workgroups"] = groups.value
        out["residual_bytes"] = (n_fields + 1) * 8 * n_pts
        kms, kbytes, names = (C.c_double * 8)(), (C.c_double * 8)(), C.create_string_buffer(256)
        monitor(1, 0)
        hfx.check(lib.hfx_time_fused_kernels(e, f, C.c_int(nb), C.c_int(10), kms, names))
        hfx.check(lib.hfx_fused_kernel_bytes(e, kbytes))
        out["update_kernel_ms"], out["update_kernel_bytes"] = kms[3], kbytes[3]
        if kms[3] > 0:
            rate = kbytes[3] / (1e-3 * kms[3])
            out["update_kernel_GBps"] = rate / 1e9
            out["residual_bound_ms"] = 1e3 * out["residual_bytes"] / rate
    print(json.dumps({k: v for k, v in out.items() if k != "cases"}), flush=True)

    for freq in args.freqs:
        n_rows = len([s for s in range(1, args.steps + 1) if s == 1 or s % freq == 0])
        ms = {"without": [], "sampled": []}
        for _ in range(args.regions):
            if args.mode == "monitor":
                monitor(1, 0)
            ms["without"].append(region(args.steps))
            if args.mode == "monitor":
                monitor(freq, n_rows)
                ms["sampled"].append(region(args.steps))
                assert len(hfx.read_history_of(e, n_fields, 2 * case.n_dims + 2)[1]) == n_rows
            else:
                ms["sampled"].append(region_by_hand(args.steps, freq))
        med = {k: statistics.median(x) for k, x in ms.items()}
        out["cases"].append(dict(monitor_res_freq=freq, rows=n_rows, ms_per_step=med, all_regions=ms,
                                 cost_ms_per_row=(med["sampled"] - med["without"]) * args.steps / n_rows,
                                 overhead=med["sampled"] / med["without"] - 1.0))
        print(json.dumps(out["cases"][-1]), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    case.close()


if __name__ == "__main__":
    main()
