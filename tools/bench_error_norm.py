#!/usr/bin/env python3
"""What one call of the exact-solution error monitor costs on the flagship box (32^3 hexahedra, P4, periodic Taylor-Green):
hfx_eles_compute_error (csrc/error_norm.hip) timed from the host around the whole call -- the fused kernel, the copy of one
partial per workgroup and quantity, the synchronisation -- as the median of `reps` calls after one warm-up call, for
  - test case 1 (the state alone) after two steps of the split fused stage, and
  - test case 5 (state and gradient, made-up walls) after one per-method residual,
beside the bytes the kernel must move: the state (and the gradient), the positions and the determinants once from HBM, and the
operator, which every pass of every workgroup reads again (from L2).  The state is the Taylor-Green one: the errors mean nothing
here, only the time does.

    python tools/bench_error_norm.py [--cells 32] [--order 4] [--reps 20] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hifiles-solver_amd"))

import hfx  # noqa: E402
import hfx_host as H  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=32)
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib = hfx.lib()
    case = H.Case(args.cells, order=args.order)
    case.set_test_case(1, 2)
    case.set_deferred(False)
    case.to_device(0)
    ctx, e, f, nb = case.handles()
    n_upts, n_eles, n_fields, n_dims = case.n_upts, case.n_eles, case.n_fields, case.n_dims
    n_cub = case.array("weight_volume_cubpts").shape[0]
    groups, epp = C.c_int(0), C.c_int(0)
    hfx.check(lib.hfx_eles_error_launch(e, C.byref(groups), C.byref(epp)))
    out = np.zeros((2, n_fields), order="F")

    def timed(test_case):
        x = hfx.Exact(test_case, 0, 0.3, 1.1, 1.0, 1.0, 2.0)
        hfx.check(lib.hfx_ctx_set_exact_solution(ctx, C.byref(x)))
        ms = []
        for r in range(args.reps + 1):
            hfx.check(lib.hfx_ctx_synchronize(ctx))
            t0 = time.perf_counter()
            hfx.check(lib.hfx_eles_compute_error(e, C.c_int(2), C.c_double(0.0), out.ctypes.data_as(hfx.dp)))
            ms.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ms[1:]), ms[1:]

    hfx.check(lib.hfx_run_steps(e, f, C.c_int(nb), C.c_int(2), C.c_int(3)))
    ms1, all1 = timed(1)
    hfx.check(lib.hfx_CalcResidual(e, f, C.c_int(nb)))
    ms5, all5 = timed(5)

    point = 8 * n_cub * n_eles
    state = 8 * n_upts * n_eles * n_fields
    hbm1 = state + point * (n_dims + 1)
    hbm5 = hbm1 + state * n_dims
    opp = 8 * n_cub * n_upts
    passes = -(-n_eles // epp.value)
    res = dict(cells=args.cells, order=args.order, n_eles=n_eles, n_upts=n_upts, n_cubpts=n_cub, groups=groups.value,
               eles_per_pass=epp.value, reps=args.reps,
               test_case_1=dict(ms=ms1, all_ms=all1, hbm_bytes=hbm1, operator_bytes_from_l2=opp * passes,
                                hbm_gb_per_s=hbm1 / ms1 * 1e-6),
               test_case_5=dict(ms=ms5, all_ms=all5, hbm_bytes=hbm5, operator_bytes_from_l2=opp * passes * (1 + n_dims),
                                hbm_gb_per_s=hbm5 / ms5 * 1e-6),
               scratch_the_integral_monitor_would_take=8 * n_cub * n_eles * n_fields * (1 + n_dims))
    print("error monitor, %d^3 P%d: %d workgroups, %d element(s) per pass, %d cubature points per element" %
          (args.cells, args.order, groups.value, epp.value, n_cub))
    for k in ("test_case_1", "test_case_5"):
        r = res[k]
        print("  %s: %.3f ms per call (min %.3f, max %.3f); %.1f MB from HBM (%.0f GB/s), %.1f MB of operator reads from L2" %
              (k, r["ms"], min(r["all_ms"]), max(r["all_ms"]), r["hbm_bytes"] / 1e6, r["hbm_gb_per_s"],
               r["operator_bytes_from_l2"] / 1e6))
    print("  (interpolating all fields to scratch first, as the integral monitor does, would take %.0f MB)" %
          (res["scratch_the_integral_monitor_would_take"] / 1e6))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)
    case.close()


if __name__ == "__main__":
    main()
