#!/usr/bin/env python3
"""What the mass-flux body force costs on the flagship box (32^3 hexahedra, P4, periodic Taylor-Green): hfx_run_steps(..., 3 steps,
fused 3) alternately without and with the body force registered on the same device block, in one process; the median of 5
regions each after one warm-up step.  With the force every update kernel also reads src_upts (5 doubles per solution point and
stage) and every step starts with the three kernels of one evaluation.  Then those three kernels on their own, each between
two HIP events (hfx_time_body_force_kernels), with the GB/s of the streaming one (4 doubles per solution point), and beside
them the split stage's update kernel without and with the source term (hfx_time_fused_kernels).

The inflow plane is the x-min plane of the periodic box (32 x 32 faces), area its true area, mdot0 = 0: the Taylor-Green state
carries no mass through it, so the controller's force stays at rounding level and the flow is the benchmark's own.

    python tools/bench_forcing.py [--cells 32] [--order 4] [--steps 3] [--regions 5] [--json out.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=32)
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib = hfx.lib()
    case = H.Case(args.cells, order=args.order, body_forcing=1)
    area = case.cfg["length"] ** 2
    assert len(case.inflow_faces()[0]) == args.cells ** 2
    case.to_device(0)
    ctx, e, f, nb = case.handles()

    def region(n):
        hfx.check(lib.hfx_ctx_synchronize(ctx))
        t0 = time.perf_counter()
        hfx.check(lib.hfx_run_steps(e, f, C.c_int(nb), C.c_int(n), C.c_int(3)))
        hfx.check(lib.hfx_ctx_synchronize(ctx))
        return 1e3 * (time.perf_counter() - t0) / n

    def update_kernel():
        kt, names = (C.c_double * 8)(), (C.c_char * 256)()
        hfx.check(lib.hfx_time_fused_kernels(e, f, C.c_int(nb), C.c_int(10), kt, names))
        kn = names.value.decode().split(",")
        i = [i for i, k in enumerate(kn[:4]) if "update" in k]
        return (kn[i[0]], kt[i[0]]) if i else (None, 0.0)

    hfx.check(lib.hfx_eles_clear_body_force(e))
    region(1)  # warm-up: the fused tables, the first launches
    ms = {"without": [], "with": []}
    for _ in range(args.regions):
        for label in ("without", "with"):
            if label == "with":
                case.set_forcing(area, 0.0)  # registers (again): a fresh controller
                region(1)                    # (the first launches of the three kernels, the allocation of src_upts)
            else:
                hfx.check(lib.hfx_eles_clear_body_force(e))  # src_upts goes with it: the update kernel reads none
            ms[label].append(region(args.steps))
    P = case.n_eles * case.n_upts
    hfx.check(lib.hfx_eles_clear_body_force(e))
    name, upd_without = update_kernel()
    case.set_forcing(area, 0.0)
    k = (C.c_double * 3)()
    hfx.check(lib.hfx_time_body_force_kernels(e, C.c_int(5), k))   # (first launches)
    hfx.check(lib.hfx_time_body_force_kernels(e, C.c_int(50), k))
    _, upd_with = update_kernel()
    s = case.body_force_state()
    out = dict(cells=args.cells, order=args.order, n_upts_total=P, inflow_faces=args.cells ** 2,
               ms_per_step_without=statistics.median(ms["without"]), ms_per_step_with=statistics.median(ms["with"]), regions=ms,
               mass_flux_kernel_ms=k[0], body_force_kernel_ms=k[1], add_body_force_kernel_ms=k[2],
               add_body_force_kernel_gbs=4 * 8 * P / (k[2] * 1e-3) / 1e9,
               update_kernel=name, update_kernel_ms_without=upd_without, update_kernel_ms_with=upd_with,
               last_body_force_x=s["body_force_x"])
    out["cost_fraction_of_a_step"] = out["ms_per_step_with"] / out["ms_per_step_without"] - 1.0
    print(json.dumps(out), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    case.close()


if __name__ == "__main__":
    main()
