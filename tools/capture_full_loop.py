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

Nothing under oracle/ is written: everything runs in a temporary directory, and no bytecode cache is left.  The archive is written
with fixed member times, so that a second capture gives the same bytes.

    python tools/capture_full_loop.py            # all
    python tools/capture_full_loop.py fl_quad_p3_walls
"""
import glob
import json
import os
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
from capture_golden import read_dump, write_neu, write_neu_tets  # noqa: E402
import full_loop_util as FU  # noqa: E402
import integral_history_util as IU  # noqa: E402
import plot_rows_util as PU  # noqa: E402

GOLDEN = FU.FL_DIR
MAX_BYTES = CH.MAX_BYTES


def derive(base, name, steps, forced=False, **over):
    """the case `base` of tools/capture_history_rows.py with other steps and input keys; forced: the driver runs with body_forcing 1"""
    b = next(c for c in CH.CASES if c["name"] == base)
    c = dict(b, name=name, steps=steps, forced=forced, keys=dict(b["keys"]))
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


def save_npz(path, arrays):
    """np.savez_compressed with the members' times fixed: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)


def capture(c):
    forced = c["forced"]
    with tempfile.TemporaryDirectory() as td:
        mesh = os.path.join(td, "mesh.neu")
        if c.get("tets"):
            xv = write_neu_tets(mesh, c["n"], amp=c["amp"])
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
        if forced:  # (the driver's input alone)
            with open(os.path.join(td, "input_forced"), "w") as f:
                f.write(open(os.path.join(td, "input")).read() + "body_forcing 1\n")
        env = dict(os.environ, HIFILES_HOME=CH.REF_HOME, HFX_DUMP_PPTS="1")
        driver_out = ""
        for cmd in ([CH.DRIVER, "input_forced" if forced else "input"], [CH.HARNESS, "input", "dump.bin", str(c["steps"]), str(c["level"])]):
            r = subprocess.run(cmd, cwd=td, env=env, capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
                raise SystemExit("%s failed for %s" % (os.path.basename(cmd[0]), c["name"]))
            if cmd[0] == CH.DRIVER:
                driver_out = r.stdout
        arrs = read_dump(os.path.join(td, "dump.bin"))
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
                bcs=c.get("bcs"), orient_seed=None,
                generator="tools/capture_full_loop.py via oracle/_ref/HiFiLES_ref and oracle/_ref/ref_harness (genuine reference)")
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)

    # the conditions, through the oracle
    w = FU.walk(out)
    free = w["unforced"] if forced else w["states"][-1]
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
