#!/usr/bin/env python3
"""Capture the full-loop fixtures (tests/golden/full_loop/fl_*.npz) -- TEST INFRASTRUCTURE, container only.

Small cases of the genuine driver doing what its main loop (src/HiFiLES.cpp:194-300) always does, all at once: the mass-flux
body force at the top of a step, the time averages, history.plt (residual norms, wall forces, integral quantities) at
monitor_res_freq and the plot files at a DIFFERENT plot_freq.  Per case the genuine reference that `build()` compiles into
oracle/_ref runs twice on one mesh.neu and input, as in tools/capture_history_rows.py and tools/capture_plot_rows.py, whose parsers
and case tables this tool imports: the DRIVER (oracle/_ref/HiFiLES_ref, write_type 1) writes history.plt and the Tecplot files, the
HARNESS (oracle/_ref/ref_harness, level 2, with HFX_DUMP_PPTS) the arrays a device block is built from.

A file holds the harness's arrays without the intermediates of its first residual and without its per-step states but the last,
every column of every history row, every row of every plot file (average columns included, in the layout of the pr_* files), on the
forced case the controller lines the driver prints before every step, and the input keys in meta_json.

Conditions enforced before a file is written, on the CPU, through tests/full_loop_util.py (walk):
  1. the two runs are one: the oracle stepped from the harness's initial state meets the harness's state after the LAST step within
     1e-11 of its largest value.  On the forced case the harness, whose first residual is hand-unrolled without the forcing branch,
     runs with forcing off: the oracle WITHOUT the force is tied to it that way, and the oracle WITH the controller in lockstep to
     the mass flux and force the driver prints before every step, at 1e-7 of the printed 8 digits;
  2. every row the driver wrote is met by the oracle in lockstep at the bars of tests/history_rows_util.py and
     tests/plot_rows_util.py, with the reference's pairing: the state after the step, the corrected gradient of the last stage's input;
  3. the fixture can tell right from subtly wrong: the sensitivity numbers of tests/full_loop_util.py, each stored in the file, each
     more than 1e-6 in every row or file it is formed for.  dt is the neighbouring hr_* case's; no case needed a larger one.
The triangle cases (see TRI_MESH below) also hold what the host mirror cannot give: the surface cubature of every local face as the
reference formed it (HFX_DUMP_INTERS_CUBPTS: opp_, weight_, inter_detjac_ and norm_inters_cubpts_l in the mirror's shapes, and the
reference state of the wall forces); the wall list is derived from the boundary tables in tests/full_loop_util.py.  On the triangle
case with shock capturing the harness runs without the filter, as on the forced case it runs without the force: condition 1 ties the
oracle WITHOUT the filter to it, condition 2 the oracle WITH it to every row of the driver, the sensor column among them, and the
file holds how many elements the filter took per stage and per step -- in every step at least one and not all.

Nothing under oracle/ is written: everything runs in a temporary directory, and no bytecode cache is left.  The archive is written
with fixed member times, so that a second capture gives the same bytes.

    python tools/capture_full_loop.py            # all
    python tools/capture_full_loop.py fl_quad_p3_walls
"""
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

sys.dont_write_bytecode = True  # (importing capture_golden would otherwise leave oracle/__pycache__)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import capture_history_rows as CH  # noqa: E402  (puts oracle/, tests/ and the package on the path)
import capture_plot_rows as CP  # noqa: E402
import capture_tris_shock as CTS  # noqa: E402
from capture_golden import read_dump, write_neu, write_neu_tets  # noqa: E402
from gen_neu_mesh import box_vertices  # noqa: E402
import full_loop_util as FU  # noqa: E402
import hfx  # noqa: E402
import integral_history_util as IU  # noqa: E402
import plot_rows_util as PU  # noqa: E402
import tri_shock_util as TS  # noqa: E402
import tri_util as T  # noqa: E402

GOLDEN = FU.FL_DIR
MAX_BYTES = CH.MAX_BYTES
CTS_SHOCK = CTS.SHOCK  # (shock_cap 1, expf_fac 36, expf_order 4, expf_cutoff 1, shock_det_field 0: the keys of ts_p3_n4)


def derive(base, name, steps, forced=False, mesh=None, **over):
    """the case `base` of tools/capture_history_rows.py with other steps and input keys; forced: the driver runs with body_forcing 1;
    mesh: other entries of the case itself (n, tris, orient_seed, shock)"""
    b = next(c for c in CH.CASES if c["name"] == base)
    c = dict(b, name=name, steps=steps, forced=forced, keys=dict(b["keys"]), **(mesh or {}))
    c["keys"].pop("pairing", None)
    c["keys"].pop("forced", None)
    c["keys"].update(over)
    return c


CHANNEL = dict(integral_quantities=CH.ALL_FIVE, p_res=2, diagnostic_fields="4 u pressure vorticity q_criterion",
               average_fields="3 rho_average u_average e_average")

CASES = [
    # the channel of hr_hex_p2_forced (4 x 3 x 3 undeformed P2 hexahedra, x and z cyclic, isothermal walls in y), 7 steps: history
    # rows after 1, 3, 6, plot files after 2, 4, 6 -- step 6 sampled by both, 5 and 7 by neither.
    # WITHOUT the body force: the genuine driver does not survive three forced steps on this box.  Its controller's hard-coded inflow
    # area of 9.162 (src/eles.cpp:5393) is a quarter of the box's (2 pi)^2, so every step over-corrects the mass flux by a factor of
    # about -6 (the driver prints 79, -483, ...) and the third step's residual is NaN, whatever dt.  The force runs in
    # fl_hex_p2_forced below, a case of its own of the two steps the driver does take
    derive("hr_hex_p2_forced", "fl_hex_p2_channel", steps=7, monitor_res_freq=3, plot_freq=2, **CHANNEL),
    # the same channel DRIVEN (body_forcing 1 for the driver only), the two steps the driver survives: a history row after step 1, a
    # plot file after step 2, the averages and the controller in every step
    derive("hr_hex_p2_forced", "fl_hex_p2_forced", steps=2, forced=True, monitor_res_freq=3, plot_freq=2, **CHANNEL),
    # hr_quad_p3_walls (4 x 4 deformed P3 quadrilaterals between an isothermal and an adiabatic wall, its dt), 5 steps: history rows
    # after 1, 2, 4, plot file after 3
    derive("hr_quad_p3_walls", "fl_quad_p3_walls", steps=5, monitor_res_freq=2, integral_quantities="2 kineticenergy enstropy",
           plot_freq=3, p_res=2, diagnostic_fields="2 mach vorticity"),
    # hr_tet_p2_rk45's mesh with forward Euler: the only stage of a step is both its first and its last.  6 steps: history rows
    # after 1, 4, plot files after 3, 6
    derive("hr_tet_p2_rk45", "fl_tet_p2_euler", steps=6, adv_type=0, monitor_res_freq=4, res_norm_type=1,
           integral_quantities=CH.ALL_FIVE, plot_freq=3, p_res=3, diagnostic_fields="2 vorticity pressure",
           average_fields="1 rho_average"),
]

# TRIANGLES.  The box of fl_quad_p3_walls with 4 x 5 squares, each cut into two deformed P3 triangles (tests/tri_util.py:
# write_neu_tris): 40 elements, at G = 32 one whole group of the fused 2-D simplex stage and a ragged one of 8; node lists rotated,
# cyclic in x, an isothermal wall on y-, an adiabatic one on y+.  The keys of fl_quad_p3_walls (viscous, RK45, dt_type 0,
# calc_force 1, its dt) and the time averages; p_res 5, the smallest with more than one plot point strictly inside a triangle: the
# probes of tests/full_loop_util.py sit there.  The host mirror builds no triangles: the harness dumps the surface cubature of the
# wall forces itself (HFX_DUMP_INTERS_CUBPTS)
TRI_MESH = dict(n=[4, 5], tris=True, orient_seed=5)
TRI_KEYS = dict(upts_type_tri=0, fpts_type_tri=0, vcjh_scheme_tri=1, c_tri=0.0, monitor_res_freq=2,
                integral_quantities="2 kineticenergy enstropy", plot_freq=3, p_res=5, average_fields="3 rho_average u_average e_average")
CASES += [
    derive("hr_quad_p3_walls", "fl_tri_p3_walls", steps=5, mesh=TRI_MESH, diagnostic_fields="2 mach vorticity", **TRI_KEYS),
    # the same with shock_cap 1 for the DRIVER and the sensor among the plotted fields.  The harness does not dump a triangle run
    # with the filter (tools/capture_tris_shock.py): it runs with shock_cap 0 and gives the arrays; the filter's operators are rebuilt
    # in numpy (hfx.tri_shock_operators).  Condition 1 is split as on a forced case: the oracle WITHOUT the filter is tied to the
    # harness's last state, the oracle WITH it to every row the driver wrote, the sensor column among them.  s0: the first of
    # tri_shock_util.choose_s0's gaps of the first stage's sensors for which no sensor value of any stage of the run lies within
    # tri_shock_util.MARGIN of it and in EVERY step at least one element and not all are filtered; the mesh amplitude is the base's
    derive("hr_quad_p3_walls", "fl_tri_p3_shock", steps=5, mesh=dict(TRI_MESH, shock=dict(CTS_SHOCK)),
           diagnostic_fields="3 mach vorticity sensor", **TRI_KEYS),
    # NO fl_tri_p3_forced: the reference's body force exists in three dimensions only.  Its CalcResidual evaluates the mass-flux
    # controller under `FlowSol->n_dims == 3` (src/solver.cpp:97), so the genuine driver with body_forcing 1 on this box IS the run
    # of fl_tri_p3_walls -- it prints no controller line and adds no source -- and there is nothing of the driver's to compare a
    # forced triangle block with; hfx_eles_set_body_force refuses a two-dimensional block for the same reason
]


def save_npz(path, arrays):
    """np.savez_compressed with the members' times fixed: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)


def run(cmd, td, env, name):
    r = subprocess.run(cmd, cwd=td, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
        raise SystemExit("%s failed for %s" % (os.path.basename(cmd[0]), name))
    return r.stdout


def shock_arrays(c, arrs):
    """the filter of a triangle case: the operators of eles_tris rebuilt from the harness's loc_upts, and s0 (see the case)"""
    sh = c["shock"]
    n_eles, order = int(arrs["sizes"][0]), int(arrs["sizes"][5])
    iv, ef, norm, high = hfx.tri_shock_operators(arrs["loc_upts"], order, sh["expf_fac"], sh["expf_order"], sh["expf_cutoff"])
    out = dict(shock_cap=np.array([1], dtype=np.int32), inv_vandermonde=iv, exp_filter=ef, norm_basis_persson=norm,
               persson_high_modes=high, shock_det_field=np.array([sh["shock_det_field"]], dtype=np.int32),
               expf_fac=np.array([sh["expf_fac"]]), expf_order=np.array([sh["expf_order"]], dtype=np.int32),
               expf_cutoff=np.array([sh["expf_cutoff"]], dtype=np.int32), s0=np.array([np.inf]))
    block = dict(arrs, **out)
    first = TS.lockstep(block, 1, shock=False)["stage_sensors"][0]
    n_stages = int(arrs["sizes"][7])
    for skip in range(12):
        s0 = TS.choose_s0(first, skip)
        sens = TS.lockstep(block, c["steps"], s0=s0)["stage_sensors"]
        per_step = [int((sens[s * n_stages:(s + 1) * n_stages] >= s0).any(axis=0).sum()) for s in range(c["steps"])]
        if TS.closest(sens, s0) > TS.MARGIN and all(0 < k < n_eles for k in per_step):
            out["s0"] = np.array([s0])
            return out
        print("%s: s0 %.4e of gap %d: closest %.1e, filtered per step %s of %d -- the next-widest gap"
              % (c["name"], s0, skip, TS.closest(sens, s0), per_step, n_eles))
    raise SystemExit("%s: no s0 filters at least one element and not all in every step: raise the amplitude" % c["name"])


def capture(c):
    forced, shock = c["forced"], c.get("shock")
    with tempfile.TemporaryDirectory() as td:
        mesh = os.path.join(td, "mesh.neu")
        if c.get("tets"):
            xv = write_neu_tets(mesh, c["n"], amp=c["amp"])
        elif c.get("tris"):
            xv = box_vertices(c["n"], 2, amp=c["amp"])
            T.write_neu_tris(mesh, c["n"], xv, bcs=c.get("bcs"), orient_seed=c.get("orient_seed"))
        else:
            xv = write_neu(mesh, c["n"], c["dims"], amp=c["amp"], bcs=c.get("bcs"))
        keys = dict(c["keys"])
        keys["n_steps"] = c["steps"]
        keys["write_type"] = 1
        if c["dims"] == 2:
            keys.pop("dz_cyclic")
        with open(os.path.join(td, "input"), "w") as f:
            for k, v in keys.items():
                f.write("%s %s\n" % (k, repr(v) if isinstance(v, float) else v))
        env = dict(os.environ, HIFILES_HOME=CH.REF_HOME, HFX_DUMP_PPTS="1")
        if c.get("tris"):
            env["HFX_DUMP_INTERS_CUBPTS"] = "1"
        # the harness, in a directory of its own beside the driver's
        hd = os.path.join(td, "harness")
        os.mkdir(hd)
        for f in ("mesh.neu", "input"):
            shutil.copyfile(os.path.join(td, f), os.path.join(hd, f))
        run([CH.HARNESS, "input", "dump.bin", str(c["steps"]), str(c["level"])], hd, env, c["name"])
        arrs = read_dump(os.path.join(hd, "dump.bin"))
        # the driver's input alone: the body force; the shock filter with the s0 the harness's arrays give
        more = {}
        if forced:
            more["body_forcing"] = 1
        if shock:
            filt = shock_arrays(c, arrs)
            arrs.update(filt)
            more.update(shock, s0=float(filt["s0"][0]))
        with open(os.path.join(td, "input_driver"), "w") as f:
            f.write(open(os.path.join(td, "input")).read())
            for k, v in more.items():
                f.write("%s %s\n" % (k, repr(v) if isinstance(v, float) else v))
        driver_out = run([CH.DRIVER, "input_driver"], td, env, c["name"])
        sz = [int(v) for v in arrs["sizes"]]
        n_eles, n_fields, n_dims, n_stages = sz[0], sz[3], sz[4], sz[7]
        calc_force = int(keys.get("calc_force", 0))
        ids = np.ravel(arrs["integral_quantity_ids"])
        it, res, frc, hdiag, time = CH.parse_history(os.path.join(td, "history.plt"), n_fields, n_dims, calc_force, len(ids))
        diag = keys["diagnostic_fields"].split()[1:]
        avg = keys.get("average_fields", "0").split()[1:]
        n_ppts = arrs["opp_p"].shape[0]
        files = {}
        for path in glob.glob(os.path.join(td, "Mesh_*_p0000.plt")):
            files[int(os.path.basename(path).split("_")[1])] = CP.parse_plt(path, n_dims + n_fields + len(avg) + len(diag))

    steps, freq, plot_freq = c["steps"], int(keys["monitor_res_freq"]), int(keys["plot_freq"])
    want_rows, want_files = IU.sample_steps(0, steps, freq), PU.sample_steps(0, steps, plot_freq)
    files.pop(0, None)  # (the file of step 0: the gradient in it is one nothing has written)
    if list(it) != want_rows or sorted(files) != want_files:
        raise SystemExit("%s: history rows at %s and plot files at %s, the sampling rules give %s and %s"
                         % (c["name"], list(it), sorted(files), want_rows, want_files))
    rows = np.stack([files[s] for s in want_files])
    if rows.shape[1] != n_eles * n_ppts:
        raise SystemExit("%s: %d rows per file, %d elements of %d plot points" % (c["name"], rows.shape[1], n_eles, n_ppts))

    last = "u_step%d_stage%d" % (steps - 1, n_stages - 1)
    out = {k: v for k, v in arrs.items() if not (k.startswith("s0_") or k.startswith("u_step") or k == "disu_ppts")}
    out["u_last_harness"] = arrs[last]  # (on the forced case: of the run WITHOUT the force)
    if int(keys["adv_type"]) == 0:
        # forward Euler reads no RK coefficients and the reference sets none: what the harness dumps is whatever the memory held,
        # other bytes in every run
        out["RK_a"], out["RK_b"] = np.zeros_like(arrs["RK_a"]), np.zeros_like(arrs["RK_b"])
    time_ref = float(keys["L_free_stream"]) / IU.scalar(arrs, "uvw_ref")
    t_rows = np.array([s * IU.scalar(arrs, "dt") * time_ref for s in want_rows])
    if not np.all(np.abs(time - t_rows) <= 1e-13 * np.abs(time)):
        raise SystemExit("%s: the driver's times %s are not step x dt x time_ref %s" % (c["name"], time, t_rows))
    out["hist_iter"], out["hist_res"], out["hist_force"], out["hist_diag"], out["hist_time"] = it, res, frc, hdiag, time
    out["time_ref"] = np.array([time_ref])
    out["monitor_res_freq"] = np.array([freq], dtype=np.int32)
    out["res_norm_type"] = np.array([int(keys["res_norm_type"])], dtype=np.int32)
    out["calc_force"] = np.array([calc_force], dtype=np.int32)
    out["body_forcing"] = np.array([int(forced)], dtype=np.int32)
    out["plot_iter"] = np.array(want_files, dtype=np.int32)
    out["plot_rows"] = rows  # (n_files, n_eles * n_ppts, n_dims + n_fields + n_average + n_diag): per element and plot point
    out["plot_freq"] = np.array([plot_freq], dtype=np.int32)
    out["p_res"] = np.array([int(keys["p_res"])], dtype=np.int32)
    out["diagnostic_fields"] = np.frombuffer(" ".join(diag).encode(), dtype=np.uint8)
    out["average_fields"] = np.frombuffer(" ".join(avg).encode(), dtype=np.uint8)
    out["xv"] = xv
    if forced:
        lines = [l for l in driver_out.splitlines() if l.startswith("iter, mdot0")]
        if len(lines) != steps:
            raise SystemExit("%s: the driver printed %d controller lines for %d steps" % (c["name"], len(lines), steps))
        out["driver_controller"] = np.array([[float(x) for x in l.split(":")[1].split(",")] for l in lines])
    meta = dict(name=c["name"], n=c["n"], dims=c["dims"], amp=c["amp"], steps=steps, level=c["level"], keys=c["keys"],
                bcs=c.get("bcs"), orient_seed=c.get("orient_seed"),
                generator="tools/capture_full_loop.py via oracle/_ref/HiFiLES_ref and oracle/_ref/ref_harness (genuine reference)")
    if c.get("tris"):
        meta.update(mesh="tests/tri_util.py: write_neu_tris", driver_keys=more)
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)

    # the conditions, through the oracle
    w = FU.walk(out)
    free = FU.harness_state(out, w)
    tie = float(np.abs(free - arrs[last]).max() / np.abs(arrs[last]).max())
    if not tie <= 1e-11:
        raise SystemExit("%s: driver and harness are not one run: the oracle's last state misses the harness's by %.2e" % (c["name"], tie))
    ctl = None
    if forced:
        ctl = FU.controller_tie(out, w)
        drv = out["driver_controller"]
        if not (ctl <= 1e-7 and np.all(drv[:, 1] == CH.FM) and np.all(drv[:, 4] != 0)):
            raise SystemExit("%s: the controller in lockstep misses the driver's printed mass flux and force by %.2e" % (c["name"], ctl))
    worst = FU.worst_bars(w)
    if not worst <= 1.0:
        raise SystemExit("%s: the oracle in lockstep misses the driver's rows by %.2f bars: history %s, plot %s"
                         % (c["name"], worst, [{k: v for k, v in r.items() if k.endswith("bars")} for r in w["hist"]],
                            [s["bars"] for s in w["plot"]]))
    for k in FU.SENSITIVITY:
        v = w["sens"][k]
        if v and not min(v) > FU.MARGIN:
            raise SystemExit("%s: %s is %s: raise dt or the amplitude" % (c["name"], k, v))
        out["sens_" + k] = np.array(v)
    out["state_tie"] = np.array([tie])
    if shock:
        per_stage, per_step, gap = FU.filtered_counts(out)
        if not (gap > TS.MARGIN and np.all((per_step >= 1) & (per_step <= sz[0] - 1))):
            raise SystemExit("%s: filtered per step %s of %d, closest sensor value %.1e from s0" % (c["name"], per_step, sz[0], gap))
        out["filtered_per_stage"], out["filtered_per_step"], out["closest_sensor_to_s0"] = per_stage, per_step, np.array([gap])
    out["rows_paired_bars"] = np.array([s["bars"] for s in w["plot"]]).max(axis=0)  # per column behind the position, as the pr_* files
    out["hist_paired_bars"] = np.array([max(r[k] for k in ("res_bars", "force_bars", "diag_bars") if k in r) for r in w["hist"]])

    os.makedirs(GOLDEN, exist_ok=True)
    path = os.path.join(GOLDEN, c["name"] + ".npz")
    save_npz(path, out)
    size = os.path.getsize(path)
    if size > MAX_BYTES:
        raise SystemExit("%s: %d bytes, more than a committed file may have" % (path, size))
    fmt = lambda v: ("%.1e" % min(v)) if len(v) else "-"
    print("%-18s %6.1f kB  history rows at %s, plot files at %s, state tie %.1e, controller tie %s, worst %.2f bars; own gradient: force "
          "%s vorticity %s, previous state %s, unforced %s, spinup 0 %s"
          % (c["name"], size / 1e3, want_rows, want_files, tie, "-" if ctl is None else "%.1e" % ctl, worst,
             *[fmt(w["sens"][k]) for k in FU.SENSITIVITY]))


if __name__ == "__main__":
    want = sys.argv[1:]
    for c in CASES:
        if not want or c["name"] in want:
            capture(c)
