#!/usr/bin/env python3
"""What the integral monitor costs on the flagship box (32^3 hexahedra, P4, periodic Taylor-Green), one device:
  - the sample on its own (hfx_time_integral_quantities: the fused kernel and the finishing launch, HIP events around back-to-back
    samples) for the kinetic energy alone and for all five quantities;
  - ms per step of hfx_run_steps(..., fused 3) without a monitor and with all five quantities sampled inside the loop at
    monitor_res_freq 1, 10 and 100 (a sampled step ends with one RK stage call by call);
  - against that, what a caller did before per sample: leave the loop, hfx_CalcResidual (which leaves the gradient of the state
    itself, not the reference's pairing), hfx_eles_CalcIntegralQuantities (two scratch arrays, a host synchronisation);
alternately on the same device block in one process, the median of `regions` regions of `steps` steps each after a warm-up.

    python tools/bench_integrals.py [--cells 32] [--order 4] [--steps 100] [--regions 3] [--json out.json]
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

FIVE = [0, 1, 2, 3, 4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=32)
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--freqs", type=int, nargs="*", default=[1, 10, 100])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib = hfx.lib()
    case = H.Case(args.cells, order=args.order)
    case.set_integral_quantities(hfx.INTEGRAL_NAMES)  # (the cubature; the monitor itself is registered below, on the context)
    case.to_device(0)
    ctx, e, f, nb = case.handles()

    def monitor(ids, freq, capacity):
        a = (C.c_int * max(1, len(ids)))(*ids)
        hfx.check(lib.hfx_ctx_set_integral_monitor(ctx, C.c_int(len(ids)), a, C.c_int(freq), C.c_int(capacity)))

    def run(n):
        hfx.check(lib.hfx_run_steps(e, f, C.c_int(nb), C.c_int(n), C.c_int(3)))

    def region(n):
        hfx.check(lib.hfx_ctx_set_clock(ctx, C.c_double(0.0), C.c_int(0)))
        hfx.check(lib.hfx_ctx_synchronize(ctx))
        t0 = time.perf_counter()
        run(n)
        hfx.check(lib.hfx_ctx_synchronize(ctx))
        return 1e3 * (time.perf_counter() - t0) / n

    ids5 = (C.c_int * 5)(*FIVE)
    q = np.zeros(5)

    def by_hand():
        hfx.check(lib.hfx_CalcResidual(e, f, C.c_int(nb)))
        q[:] = 0.0
        hfx.check(lib.hfx_eles_CalcIntegralQuantities(e, C.c_int(5), ids5, q.ctypes.data_as(hfx.dp)))

    def region_by_hand(n, freq):
        """the loop left at every step the reference samples; residual, then the old entry point"""
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

    monitor([], 1, 1)
    region(2)  # warm-up: the fused tables, the first launches
    by_hand()  # (and the gradient arrays, the scratch arrays of the old entry point)
    n_groups, epp = C.c_int(0), C.c_int(0)
    hfx.check(lib.hfx_eles_integral_launch(e, C.byref(n_groups), C.byref(epp)))
    out = dict(cells=args.cells, order=args.order, steps_per_region=args.steps, regions=args.regions, workgroups=n_groups.value,
               eles_per_pass=epp.value, cases=[])

    # the sample on its own
    for name, ids in (("kinetic_energy", [0]), ("all_five", FIVE)):
        monitor(ids, 1, 1)
        ms = C.c_double(0)
        hfx.check(lib.hfx_time_integral_quantities(e, C.c_int(20), C.byref(ms)))
        out["sample_ms_" + name] = ms.value
    # the old entry point on its own (with its host synchronisation), and the residual that precedes it
    hfx.check(lib.hfx_ctx_synchronize(ctx))
    t0 = time.perf_counter()
    for _ in range(10):
        q[:] = 0.0
        hfx.check(lib.hfx_eles_CalcIntegralQuantities(e, C.c_int(5), ids5, q.ctypes.data_as(hfx.dp)))
    out["old_entry_point_ms"] = 1e3 * (time.perf_counter() - t0) / 10
    t0 = time.perf_counter()
    for _ in range(10):
        hfx.check(lib.hfx_CalcResidual(e, f, C.c_int(nb)))
    hfx.check(lib.hfx_ctx_synchronize(ctx))
    out["calc_residual_ms"] = 1e3 * (time.perf_counter() - t0) / 10
    print(json.dumps({k: v for k, v in out.items() if k != "cases"}), flush=True)

    for freq in args.freqs:
        n_samples = len([s for s in range(1, args.steps + 1) if s == 1 or s % freq == 0])
        ms = {"without": [], "in_loop": [], "by_hand": []}
        for _ in range(args.regions):
            monitor([], 1, 1)
            ms["without"].append(region(args.steps))
            monitor(FIVE, freq, n_samples)
            ms["in_loop"].append(region(args.steps))
            t, s, v = hfx.read_integral_history_of(e, 5)
            assert len(s) == n_samples, (len(s), n_samples)
            monitor([], 1, 1)
            ms["by_hand"].append(region_by_hand(args.steps, freq))
        med = {k: statistics.median(v) for k, v in ms.items()}
        out["cases"].append(dict(monitor_res_freq=freq, samples=n_samples, ms_per_step=med, all_regions=ms,
                                 in_loop_cost_ms_per_sample=(med["in_loop"] - med["without"]) * args.steps / n_samples,
                                 by_hand_cost_ms_per_sample=(med["by_hand"] - med["without"]) * args.steps / n_samples,
                                 in_loop_overhead=med["in_loop"] / med["without"] - 1.0,
                                 by_hand_overhead=med["by_hand"] / med["without"] - 1.0))
        print(json.dumps(out["cases"][-1]), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    case.close()


if __name__ == "__main__":
    main()
