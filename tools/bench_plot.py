#!/usr/bin/env python3
"""What the plot monitor costs, one device: the flagship box (32^3 hexahedra, P4, periodic Taylor-Green), p_res 5 (125 plot points
per element).

  --mode monitor   (this tree's library)
      (a) one snapshot with every three-dimensional field but the sensor (hfx_time_plot_fields: HIP events around back-to-back
          launches into a scratch snapshot), beside the bytes it must move -- (n_fields + n_fields n_dims) n_upts read (the energy's
          gradient is skipped: that much less), (n_fields + n_diag) n_ppts written, per element -- at the HBM rate the update kernel of
          the fused stage reaches in the same process (hfx_time_fused_kernels slot 3 over hfx_fused_kernel_bytes slot 3);
      (b) one snapshot with gradient-free fields (u v w energy mach pressure);
      (c) ms per step of hfx_run_steps(..., fused 3) without a monitor and with the snapshots taken inside the loop at plot_freq 1,
          10 and 100 (a sampled step ends with one RK stage call by call), alternating.
  --mode by_hand   (any library that has the per-call entry points: run it on the PARENT commit's library through HFX_LIB_DIR)
      (d) what a caller does without the monitor: leave the loop, hfx_CalcResidual (which also pairs the fields with the gradient of
          the wrong state), download grad_disu_upts, hfx_eles_calc_disu_ppts, and the fields in numpy (BLAS for the interpolation).

Each loop figure is the median of `regions` regions after a warm-up.

    python tools/bench_plot.py --mode monitor [--regions 3] [--json out.json]
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

ALL = ["u", "v", "w", "energy", "mach", "pressure", "vorticity", "q_criterion", "scaled_q_criterion"]
FREE = ALL[:6]
STEPS = {1: 10, 10: 20, 100: 100}  # steps of a region per plot_freq: a snapshot of this box is 0.46 GB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["monitor", "by_hand"], required=True)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--p_res", type=int, default=5)
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--freqs", type=int, nargs="*", default=[1, 10, 100])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib = hfx.lib()
    case = H.Case(args.n, order=args.order, p_res=args.p_res)
    case.set_deferred(False)
    case.to_device(0)
    ctx, e, f, nb = case.handles()
    nf, nd, nu, ne = case.n_fields, case.n_dims, case.n_upts, case.n_eles
    opp_p = case.array("opp_p")
    npp = opp_p.shape[0]
    out = dict(mode=args.mode, n_eles=ne, n_upts=nu, n_ppts=npp, regions=args.regions, library=os.environ.get("HFX_LIB_DIR", "this tree"),
               cases=[])

    def run(n):
        hfx.check(lib.hfx_run_steps(e, f, C.c_int(nb), C.c_int(n), C.c_int(3)))

    def region(n):
        hfx.check(lib.hfx_ctx_set_clock(ctx, C.c_double(0.0), C.c_int(0)))
        hfx.check(lib.hfx_ctx_synchronize(ctx))
        t0 = time.perf_counter()
        run(n)
        hfx.check(lib.hfx_ctx_synchronize(ctx))
        return 1e3 * (time.perf_counter() - t0) / n

    def monitor(names, freq, capacity):
        codes = [hfx.PLOT_NAMES.index(n) for n in names]
        a = (C.c_int * max(1, len(codes)))(*codes)
        hfx.check(lib.hfx_ctx_set_plot_monitor(ctx, C.c_int(len(codes)), a, C.c_int(freq), C.c_int(capacity)))

    region(2)  # warm-up: the fused tables, the first launches
    if args.mode == "by_hand":
        gamma = case.params().gamma
        grad = np.zeros((nu, ne, nf, nd), order="F")
        disu = np.zeros((npp, ne, nf), order="F")

        def by_hand():
            t = [time.perf_counter()]
            hfx.check(lib.hfx_CalcResidual(e, f, C.c_int(nb)))
            hfx.check(lib.hfx_ctx_synchronize(ctx))
            t.append(time.perf_counter())
            hfx.check(lib.hfx_eles_download(e, C.c_int(hfx.GRAD_DISU_UPTS), grad.ctypes.data_as(hfx.dp)))
            t.append(time.perf_counter())
            hfx.check(lib.hfx_eles_calc_disu_ppts(e, disu.ctypes.data_as(hfx.dp)))
            t.append(time.perf_counter())
            gp = (opp_p @ grad.reshape((nu, -1), order="F")).reshape((npp, ne, nf, nd), order="F")
            irho = 1.0 / disu[..., 0]
            vel = [disu[..., i + 1] * irho for i in range(nd)]
            dv = [[irho * (gp[..., i + 1, j] - vel[i] * gp[..., 0, j]) for j in range(nd)] for i in range(nd)]
            wx, wy, wz = dv[2][1] - dv[1][2], dv[0][2] - dv[2][0], dv[1][0] - dv[0][1]
            v_sq = sum(v * v for v in vel)
            pressure = (gamma - 1.0) * (disu[..., nd + 1] - 0.5 * disu[..., 0] * v_sq)
            mach = np.sqrt(v_sq / (gamma * pressure / disu[..., 0]))
            vort = np.sqrt(wx * wx + wy * wy + wz * wz)
            SS = dv[0][0] ** 2 + dv[1][1] ** 2 + dv[2][2] ** 2 + 0.5 * ((dv[0][1] + dv[1][0]) ** 2 + (dv[0][2] + dv[2][0]) ** 2 +
                                                                     (dv[1][2] + dv[2][1]) ** 2)
            OO = 0.5 * (wx * wx + wy * wy + wz * wz)
            q = 0.5 * (OO - SS)
            qs = q / (SS + 1e-24)
            t.append(time.perf_counter())
            return [1e3 * (b - a) for a, b in zip(t[:-1], t[1:])], float(mach.max() + vort.max() + q.max() + qs.max())

        by_hand()
        parts, _ = by_hand()
        out["by_hand_ms"] = dict(zip(("CalcResidual", "download_grad_disu_upts", "calc_disu_ppts", "numpy"), parts))
        out["by_hand_total_ms"] = sum(parts)
        out["grad_bytes"] = grad.nbytes
        print(json.dumps({k: v for k, v in out.items() if k != "cases"}), flush=True)
    else:
        hfx.check(lib.hfx_CalcResidual(e, f, C.c_int(nb)))  # (the timing entry point reads the gradient: one residual leaves it)
        ms = C.c_double(0)
        for tag, names in (("all", ALL), ("gradient_free", FREE), ("all_again", ALL), ("gradient_free_again", FREE)):
            monitor(names, 1, 1)
            hfx.check(lib.hfx_time_plot_fields(e, C.c_int(10), C.byref(ms)))
            out["snapshot_ms_" + tag] = ms.value
        g, epp, ppp = C.c_int(0), C.c_int(0), C.c_int(0)
        hfx.check(lib.hfx_eles_plot_launch(e, C.byref(g), C.byref(epp), C.byref(ppp)))
        out["workgroups"], out["eles_per_pass"], out["ppts_per_pass"] = g.value, epp.value, ppp.value
        out["bytes_all"] = 8 * ne * ((nf + (nf - 1) * nd) * nu + (nf + len(ALL)) * npp)
        out["bytes_gradient_free"] = 8 * ne * (nf * nu + (nf + len(FREE)) * npp)
        # FP64 work of the interpolation: one FMA per (plot point, solution point, interpolated plane)
        out["fma_all"] = ne * npp * nu * (nf + (nf - 1) * nd)
        monitor([], 1, 0)
        kms, kbytes, names = (C.c_double * 8)(), (C.c_double * 8)(), C.create_string_buffer(256)
        hfx.check(lib.hfx_time_fused_kernels(e, f, C.c_int(nb), C.c_int(10), kms, names))
        hfx.check(lib.hfx_fused_kernel_bytes(e, kbytes))
        out["update_kernel_ms"], out["update_kernel_bytes"] = kms[3], kbytes[3]
        if kms[3] > 0:
            rate = kbytes[3] / (1e-3 * kms[3])
            out["update_kernel_GBps"] = rate / 1e9
            out["bound_ms_all"] = 1e3 * out["bytes_all"] / rate
            out["bound_ms_gradient_free"] = 1e3 * out["bytes_gradient_free"] / rate
        print(json.dumps({k: v for k, v in out.items() if k != "cases"}), flush=True)
        for freq in args.freqs:
            steps = STEPS.get(freq, max(10, freq))
            n_snap = steps // freq
            ms = {"without": [], "all": [], "gradient_free": []}
            for _ in range(args.regions):
                monitor([], 1, 0)
                ms["without"].append(region(steps))
                for tag, names in (("all", ALL), ("gradient_free", FREE)):
                    monitor(names, freq, n_snap)
                    got, none = C.c_int(0), C.c_int(0)  # (the history of this registration is made here, outside the region)
                    hfx.check(lib.hfx_eles_read_plot_snapshots(e, C.c_int(0), None, None, None, C.byref(got)))
                    ms[tag].append(region(steps))
                    n = C.c_int(0)
                    hfx.check(lib.hfx_eles_plot_count(e, C.byref(n)))
                    assert n.value == n_snap, (n.value, n_snap)
            med = {k: statistics.median(x) for k, x in ms.items()}
            out["cases"].append(dict(plot_freq=freq, steps=steps, snapshots=n_snap, ms_per_step=med, all_regions=ms,
                                     cost_ms_per_snapshot={k: (med[k] - med["without"]) * steps / n_snap for k in ("all", "gradient_free")}))
            print(json.dumps(out["cases"][-1]), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    case.close()


if __name__ == "__main__":
    main()
