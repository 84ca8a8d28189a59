#!/usr/bin/env python3
"""Per-method path against the split fused stage on hexahedra of orders 4, 6 and 7 at about 4.1 M solution points each
(32^3 P4, 23^3 P6, 20^3 P7 periodic Taylor-Green boxes).  For every order and path: ms per RK stage of hfx_run_steps
(fused 0 and 3; fused 3 runs variant 2 at P6 and P7), G DOF-updates/s, and for the fused stage the fraction of the HBM roof
that the stage's algorithmic bytes (hfx_fused_kernel_bytes, summed over the launches of a stage) reach, and the same per launch.

    python tools/bench_hex_orders.py [--orders 4,6,7] [--steps 4] [--warmup 1] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hifiles-solver_amd"))

import hfx  # noqa: E402
import hfx_host as H  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E, 8.0 TB/s
CELLS = {4: 32, 6: 23, 7: 20}


def time_steps(case, fused, steps, warmup):
    ctx, e, f, nb = case.handles()
    lib = hfx.lib()
    hfx.check(lib.hfx_run_steps(e, f, C.c_int(nb), C.c_int(warmup), C.c_int(fused)))
    hfx.check(lib.hfx_ctx_synchronize(ctx))
    t0 = time.perf_counter()
    hfx.check(lib.hfx_run_steps(e, f, C.c_int(nb), C.c_int(steps), C.c_int(fused)))
    hfx.check(lib.hfx_ctx_synchronize(ctx))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--orders", default="4,6,7")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    rows = []
    for order in [int(o) for o in args.orders.split(",")]:
        n = CELLS[order]
        case = H.Case(n, order=order)
        case.to_device(0)
        ctx, e = case.handles()[0], case.handles()[1]
        dof = case.n_eles * case.n_upts * case.n_fields
        row = dict(order=order, cells=n, n_upts_total=case.n_eles * case.n_upts)
        for label, fused in (("per_method", 0), ("fused3", 3)):
            steps = max(1, args.steps // 2) if fused == 0 else args.steps
            el = time_steps(case, fused, steps, args.warmup)
            ms = 1e3 * el / (steps * case.n_stages)
            row[label] = dict(ms_per_rk_stage=ms, gdof_updates_per_s=dof / (ms * 1e-3) / 1e9, steps=steps)
            if fused:
                hfx.check(hfx.lib().hfx_ctx_set_fused_mode(ctx, C.c_int(fused)))
                b = (C.c_double * 8)()
                hfx.check(hfx.lib().hfx_fused_kernel_bytes(e, b))
                stage_bytes = sum(b[:5])
                row[label]["algorithmic_bytes_per_stage"] = stage_bytes
                row[label]["hbm_roof_fraction"] = stage_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS
                # the launches of a stage on their own (HIP events around each, hfx_time_fused_kernels)
                kt, names = (C.c_double * 8)(), (C.c_char * 256)()
                hfx.check(hfx.lib().hfx_time_fused_kernels(e, case.handles()[2], C.c_int(case.handles()[3]), C.c_int(10), kt, names))
                kn = names.value.decode().split(",")
                row[label]["kernels"] = {k: dict(ms=kt[i], algorithmic_bytes=b[i], hbm_roof_fraction=b[i] / (kt[i] * 1e-3) / 1e9 / HBM_PEAK_GBS)
                                         for i, k in enumerate(kn[:4]) if kt[i] > 0}
        row["speedup_fused_vs_per_method"] = row["per_method"]["ms_per_rk_stage"] / row["fused3"]["ms_per_rk_stage"]
        rows.append(row)
        print("P%d %d^3 (%.2f M upts): per-method %.3f ms/stage (%.2f GDOF/s) | fused %.3f ms/stage (%.2f GDOF/s, %.1f %% of HBM roof) "
              "| %.2fx" % (order, n, row["n_upts_total"] / 1e6, row["per_method"]["ms_per_rk_stage"], row["per_method"]["gdof_updates_per_s"],
                           row["fused3"]["ms_per_rk_stage"], row["fused3"]["gdof_updates_per_s"], 100 * row["fused3"]["hbm_roof_fraction"],
                           row["speedup_fused_vs_per_method"]), flush=True)
        for k, v in row["fused3"]["kernels"].items():
            print("    %-24s %.3f ms  %.1f %% of HBM roof" % (k, v["ms"], 100 * v["hbm_roof_fraction"]), flush=True)
        case.close()
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
