#!/usr/bin/env python3
"""What one call of the wall-force monitor costs: a 32 x 32 x 8 box of P4 hexahedra between two walls (2 048 wall faces of 5 x 5
cubature points), hfx_eles_compute_wall_forces (csrc/wall_force.hip) timed from the host around the whole call -- the fused
kernel, the copy of one partial per workgroup and quantity and of Cp and Cf, the synchronisation -- as the median of `reps`
calls after one warm-up call, for
  - a viscous case (state and gradient: an isothermal and an adiabatic wall) after one per-method residual, and
  - an inviscid case (the state alone: two slip walls),
beside the kernel alone (hfx_time_wall_forces) and, for comparison, what the monitor costs without it: downloading the state
and the gradient and evaluating the formulas of tests/wall_force_util.py in float64 on the host.  The forces mean nothing
here, only the time does.

    python tools/bench_wall_force.py [--cells 32 32 8] [--order 4] [--reps 20] [--json out.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hfx  # noqa: E402
import hfx_host as H  # noqa: E402
import wall_force_util as W  # noqa: E402

VISCOUS = dict(bcs=[{"type": "isotherm_wall", "T_static": 310.0, "u": 3.0}, {"type": "adiabat_wall", "v": -2.0}])
INVISCID = dict(viscous=0, ic_form=1, riemann_solve_type=0, rho_c_ic=1.2, u_c_ic=30.0, v_c_ic=10.0, w_c_ic=5.0, p_c_ic=101325.0,
                bcs=[{"type": "slip_wall"}, {"type": "slip_wall_dual"}])


def run(name, cells, order, reps, keys):
    lib = hfx.lib()
    case = H.Case(cells, order=order, calc_force=1, area_ref=1.0, monitor_cp_freq=1, nx_c_ic=0.8, ny_c_ic=0.5, nz_c_ic=0.33,
                  sides={"z-": 0, "z+": 1}, **keys)
    case.set_deferred(False)
    case.to_device(0)
    ctx, e, f, nb = case.handles()
    wp = case.wall_points()
    n_faces, n_points = len(wp["ele"]), int(wp["n_points"].sum())
    groups, fpp = C.c_int(0), C.c_int(0)
    hfx.check(lib.hfx_eles_wall_force_launch(e, C.byref(groups), C.byref(fpp)))
    viscous = bool(case.params().viscous)
    if viscous:
        hfx.check(lib.hfx_CalcResidual(e, f, C.c_int(nb)))
    fi, fv, cl, cd = (C.c_double * 3)(), (C.c_double * 3)(), C.c_double(0), C.c_double(0)
    cp, cf = np.zeros(n_points), np.zeros(n_points)
    ms = []
    for r in range(reps + 1):
        hfx.check(lib.hfx_ctx_synchronize(ctx))
        t0 = time.perf_counter()
        hfx.check(lib.hfx_eles_compute_wall_forces(e, fi, fv, C.byref(cl), C.byref(cd), cp.ctypes.data_as(hfx.dp), cf.ctypes.data_as(hfx.dp)))
        ms.append(1e3 * (time.perf_counter() - t0))
    kernel = C.c_double(0)
    hfx.check(lib.hfx_time_wall_forces(e, C.c_int(reps), C.byref(kernel)))

    # without the kernel: the arrays to the host, the same formulas there in float64
    from test_wall_force_host import device_arrays, phys_of, ref_of
    A, phys, ref = device_arrays(case), phys_of(case), ref_of(case)
    shape_u = (case.n_upts, case.n_eles, case.n_fields)
    t0 = time.perf_counter()
    u = np.zeros(shape_u, order="F")
    hfx.check(lib.hfx_eles_download(e, C.c_int(hfx.DISU_UPTS0), u.ctypes.data_as(hfx.dp)))
    grad = None
    if viscous:
        grad = np.zeros(shape_u + (case.n_dims,), order="F")
        hfx.check(lib.hfx_eles_download(e, C.c_int(hfx.GRAD_DISU_UPTS), grad.ctypes.data_as(hfx.dp)))
    t_copy = 1e3 * (time.perf_counter() - t0)
    W.LD = np.float64
    t0 = time.perf_counter()
    host = W.wall_forces(A["face_ele"], A["face_inter"], A["face_flag"], A["opp"], A["weight"], A["detjac"], A["norm"], u, grad, phys, ref)
    t_host = 1e3 * (time.perf_counter() - t0)
    dev = np.array(list(fi[:3]) + list(fv[:3]) + [cl.value, cd.value])
    ref_v = np.array(list(host["inv_force"]) + list(host["vis_force"]) + [host["cl"], host["cd"]], dtype=np.float64)
    slabs = 1 + (case.n_dims if viscous else 0)
    res = dict(name=name, cells=list(cells), order=order, n_faces=n_faces, n_points=n_points, groups=groups.value, faces_per_pass=fpp.value,
               reps=reps, call_ms=statistics.median(ms[1:]), call_all_ms=ms[1:], kernel_ms=kernel.value,
               slab_bytes=8 * case.n_upts * case.n_fields * n_faces * slabs,
               operator_bytes_from_l2=8 * 25 * case.n_upts * (-(-n_faces // fpp.value)) * slabs,
               host_download_ms=t_copy, host_float64_ms=t_host, device_minus_host=float(np.abs(dev - ref_v).max()))
    print("wall forces, %s, %s P%d: %d faces, %d workgroups, %d faces per pass" % (name, "x".join(map(str, cells)), order, n_faces,
                                                                                   groups.value, fpp.value))
    print("  whole call %.3f ms (min %.3f, max %.3f); kernel alone %.3f ms; %.1f MB staged through LDS, %.1f MB of operator reads from L2" %
          (res["call_ms"], min(ms[1:]), max(ms[1:]), kernel.value, res["slab_bytes"] / 1e6, res["operator_bytes_from_l2"] / 1e6))
    print("  on the host instead: %.1f ms to download state%s, %.1f ms for the formulas in float64 (numpy, face by face)" %
          (t_copy, " and gradient" if viscous else "", t_host))
    case.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs=3, default=[32, 32, 8])
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    out = [run("viscous", args.cells, args.order, args.reps, VISCOUS), run("inviscid", args.cells, args.order, args.reps, INVISCID)]
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
