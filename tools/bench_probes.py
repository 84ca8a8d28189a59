#!/usr/bin/env python3
"""What point probes cost on the flagship box (32^3 hexahedra, P4, periodic Taylor-Green): hfx_run_steps(..., fused 3) with
the clock set, alternately
  - without probes,
  - with probes sampled inside the loop (hfx_ctx_set_probes / hfx_eles_set_probes), and
  - the way a caller had to do it before: leave the loop every probe_freq steps, hfx_eles_download of disu_upts(0), and the
    contraction on the host (numpy),
on the same device block in one process, for 4 096 and 65 536 probes spread over the elements and probe_freq 1 and 10; the
median of `regions` regions of `steps` steps each after a warm-up.  Then the sampling kernel on its own (hfx_time_probes,
device events around back-to-back launches) and the read of one region's history.

    python tools/bench_probes.py [--cells 32] [--order 4] [--steps 10] [--regions 5] [--json out.json]
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

SIX = ["rho", "u", "v", "w", "specific_total_energy", "pressure"]


def host_fields(state, gamma):
    rho, E = state[:, 0], state[:, 4]
    v_sq = (state[:, 1] ** 2 + state[:, 2] ** 2 + state[:, 3] ** 2) / (rho * rho)
    return np.array([rho, state[:, 1] / rho, state[:, 2] / rho, state[:, 3] / rho, E / rho, (gamma - 1.0) * (E - 0.5 * rho * v_sq)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=32)
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--probes", type=int, nargs="*", default=[4096, 65536])
    ap.add_argument("--freqs", type=int, nargs="*", default=[1, 10])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib = hfx.lib()
    case = H.Case(args.cells, order=args.order)
    case.to_device(0)
    ctx, e, f, nb = case.handles()
    gamma = case.params().gamma
    n_upts, n_eles, n_fields = case.n_upts, case.n_eles, case.n_fields
    u = np.zeros((n_upts, n_eles, n_fields), order="F")

    def set_clock():
        hfx.check(lib.hfx_ctx_set_clock(ctx, C.c_double(0.0), C.c_int(0)))

    def set_fields(names, freq, capacity):
        codes = (C.c_int * max(1, len(names)))(*[hfx.PROBE_NAMES.index(n) for n in names])
        hfx.check(lib.hfx_ctx_set_probes(ctx, C.c_int(len(names)), codes, C.c_int(freq), C.c_int(capacity)))

    def run(n):
        hfx.check(lib.hfx_run_steps(e, f, C.c_int(nb), C.c_int(n), C.c_int(3)))

    def region(n):
        set_clock()
        hfx.check(lib.hfx_ctx_synchronize(ctx))
        t0 = time.perf_counter()
        run(n)
        hfx.check(lib.hfx_ctx_synchronize(ctx))
        return 1e3 * (time.perf_counter() - t0) / n

    def region_by_download(n, freq, ele, opp):
        """the loop left every freq steps, the state downloaded, the probes contracted on the host"""
        set_clock()
        hfx.check(lib.hfx_ctx_synchronize(ctx))
        t0 = time.perf_counter()
        done = 0
        while done < n:
            k = min(freq, n - done)
            run(k)
            done += k
            if done % freq == 0:
                hfx.check(lib.hfx_eles_download(e, C.c_int(hfx.DISU_UPTS0), u.ctypes.data_as(hfx.dp)))
                state = np.einsum("kp,kpf->pf", opp, u[:, ele, :])
                host_fields(state, gamma)
        hfx.check(lib.hfx_ctx_synchronize(ctx))
        return 1e3 * (time.perf_counter() - t0) / n

    region(1)  # warm-up: the fused tables, the first launches
    out = dict(cells=args.cells, order=args.order, steps_per_region=args.steps, regions=args.regions, cases=[])
    rng = np.random.default_rng(0)
    for n_probes in args.probes:
        ele = (np.arange(n_probes, dtype=np.int64) * n_eles // n_probes).astype(np.int32)  # spread over the elements
        rng.shuffle(ele)
        opp = rng.uniform(-0.2, 1.0, (n_upts, n_probes))
        for freq in args.freqs:
            samples = args.steps // freq + 1
            ms = {"without": [], "in_loop": [], "download": []}
            for _ in range(args.regions):
                set_fields([], 1, 1)
                ms["without"].append(region(args.steps))
                set_fields(SIX, freq, samples)
                hfx.set_probes_of(e, n_upts, ele, opp)
                ms["in_loop"].append(region(args.steps))
                t0 = time.perf_counter()
                t, s, v = hfx.read_probes_of(e, len(SIX))
                read_ms = 1e3 * (time.perf_counter() - t0)
                assert len(s) == args.steps // freq, (len(s), args.steps, freq)
                set_fields([], 1, 1)
                ms["download"].append(region_by_download(args.steps, freq, ele, opp))
            set_fields(SIX, freq, samples)
            hfx.set_probes_of(e, n_upts, ele, opp)
            k_ms = C.c_double(0)
            hfx.check(lib.hfx_time_probes(e, C.c_int(50), C.byref(k_ms)))
            bytes_read = n_probes * n_upts * 8 * (1 + n_fields)  # one operator row and one element's state per probe
            med = {k: statistics.median(v) for k, v in ms.items()}
            out["cases"].append(dict(n_probes=n_probes, probe_freq=freq, ms_per_step=med, all_regions=ms,
                                     in_loop_cost_ms_per_step=med["in_loop"] - med["without"],
                                     download_cost_ms_per_step=med["download"] - med["without"],
                                     sampling_kernel_ms=k_ms.value, sampling_kernel_gbs=bytes_read / (k_ms.value * 1e-3) / 1e9,
                                     read_history_ms=read_ms, samples_read=len(s)))
            print(json.dumps(out["cases"][-1]), flush=True)
    # one RK stage, for scale: a step of this scheme has n_stages of them
    set_fields([], 1, 1)
    out["ms_per_step_plain"] = region(args.steps)
    out["rk_stages_per_step"] = case.n_stages
    print(json.dumps({k: v for k, v in out.items() if k != "cases"}), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    case.close()


if __name__ == "__main__":
    main()
