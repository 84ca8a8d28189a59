#!/usr/bin/env python3
"""What the time averages cost on the flagship box (32^3 hexahedra, P4, periodic Taylor-Green): hfx_run_steps(..., 3 steps,
fused 3) with the clock set, alternately without and with the reference's five average fields on the same device block, in
one process; the median of 5 regions each after one warm-up step.  Then the update kernel of the averages on its own
(hfx_eles_CalcTimeAverageQuantities back to back) with the GB/s of its 15 doubles per solution point, and beside it the split
stage's update kernel with its algorithmic bytes (hfx_time_fused_kernels, hfx_fused_kernel_bytes).

    python tools/bench_time_average.py [--cells 32] [--order 4] [--steps 3] [--regions 5] [--json out.json]
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

FIVE = ["rho_average", "u_average", "v_average", "w_average", "e_average"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=32)
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib = hfx.lib()
    case = H.Case(args.cells, order=args.order)
    case.to_device(0)
    ctx, e, f, nb = case.handles()
    hfx.check(lib.hfx_ctx_set_clock(ctx, C.c_double(0.0), C.c_int(0)))

    def region(n):
        hfx.check(lib.hfx_ctx_synchronize(ctx))
        t0 = time.perf_counter()
        hfx.check(lib.hfx_run_steps(e, f, C.c_int(nb), C.c_int(n), C.c_int(3)))
        hfx.check(lib.hfx_ctx_synchronize(ctx))
        return 1e3 * (time.perf_counter() - t0) / n

    region(1)  # warm-up: the fused tables, the first launches
    ms = {"without": [], "with": []}
    for _ in range(args.regions):
        for label, fields in (("without", []), ("with", FIVE)):
            case.set_average_fields(fields)
            if fields:
                region(1)  # (the first launch of the averaging kernel)
            ms[label].append(region(args.steps))
    P = case.n_eles * case.n_upts
    # the kernel alone: back-to-back updates, one synchronisation
    case.set_average_fields(FIVE)
    reps = 50
    hfx.check(lib.hfx_eles_CalcTimeAverageQuantities(e, C.c_double(2.0), C.c_double(1.0)))
    hfx.check(lib.hfx_ctx_synchronize(ctx))
    t0 = time.perf_counter()
    for _ in range(reps):
        hfx.check(lib.hfx_eles_CalcTimeAverageQuantities(e, C.c_double(2.0), C.c_double(1.0)))
    hfx.check(lib.hfx_ctx_synchronize(ctx))
    k_ms = 1e3 * (time.perf_counter() - t0) / reps
    k_bytes = 15 * 8 * P
    case.set_average_fields([])
    # the split stage's update kernel, for comparison
    b, kt, names = (C.c_double * 8)(), (C.c_double * 8)(), (C.c_char * 256)()
    hfx.check(lib.hfx_fused_kernel_bytes(e, b))
    hfx.check(lib.hfx_time_fused_kernels(e, f, C.c_int(nb), C.c_int(10), kt, names))
    kn = names.value.decode().split(",")
    upd = [i for i, k in enumerate(kn[:4]) if "update" in k]
    out = dict(cells=args.cells, order=args.order, n_upts_total=P,
               ms_per_step_without=statistics.median(ms["without"]), ms_per_step_with=statistics.median(ms["with"]),
               regions=ms, average_kernel_ms=k_ms, average_kernel_gbs=k_bytes / (k_ms * 1e-3) / 1e9)
    if upd:
        i = upd[0]
        out.update(update_kernel=kn[i], update_kernel_ms=kt[i], update_kernel_gbs=b[i] / (kt[i] * 1e-3) / 1e9)
    out["cost_fraction_of_a_step"] = out["ms_per_step_with"] / out["ms_per_step_without"] - 1.0
    print(json.dumps(out), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    case.close()


if __name__ == "__main__":
    main()
