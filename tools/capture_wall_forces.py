#!/usr/bin/env python3
"""Capture the wall-force fixtures (tests/golden/wall_force/wf_*.npz) -- TEST INFRASTRUCTURE, container only.

Per case the genuine reference that `build()` compiles into oracle/_ref runs twice on the same mesh.neu and input: the DRIVER
(oracle/_ref/HiFiLES_ref), whose output::CalcForces at step 1 writes the force columns of history.plt and
force_files_000000001/cp_000000001_p0000.dat, and the HARNESS (oracle/_ref/ref_harness, level 2), which records the arrays
that CalcForces read.  adv_type 0: with one RK stage per step the harness's s0_grad_disu_upts is the gradient the driver's
CalcForces reads at step 1 and u_step0_stage0 is its state.

The meshes are one cell thick between their two walls and cyclic elsewhere, so that every local face of every element belongs to
a boundary group: the reference's loop reads bc_list(bcid) also where bcid is -1 (src/eles.cpp:5755), and on such meshes there is
no such face.  Two conditions are enforced before a file is written: the labelled faces of the cp file number exactly the
mesh's wall faces, and the driver's residual columns equal log10(s0_res_sums[:, 0] / (n_upts n_eles)) of the harness within
1e-13, which ties the two runs together.

Nothing under oracle/ is written: everything runs in a temporary directory, and no bytecode cache is left.

    python tools/capture_wall_forces.py            # all five
    python tools/capture_wall_forces.py wf_quad_p3_a
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True  # (importing capture_golden would otherwise leave oracle/__pycache__)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from capture_golden import BC_KEYS, case, read_dump, write_neu  # noqa: E402

REF_HOME = os.environ.get("HIFILES_HOME", "/root/reference")
DRIVER = os.path.join(ROOT, "oracle", "_ref", "HiFiLES_ref")
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
# a directory of their own: the suites that run every tests/golden/*.npz as a whole case (operators, metrics, every stage)
# do not take these, which hold the monitor's inputs and outputs alone
GOLDEN = os.path.join(ROOT, "tests", "golden", "wall_force")
MAX_BYTES = 1 << 20
LABELS = ("SLIP_WALL", "ISOTHERM_WALL", "ADIABAT_WALL", "SLIP_WALL_DUAL")

# every case: one Euler stage per step, forces and the cp file at step 1, a free stream off every axis (aoa and aos matter)
COMMON = dict(BC_KEYS, adv_type=0, monitor_res_freq=1, monitor_cp_freq=1, calc_force=1, area_ref=1.0,
              nx_c_ic=0.8, ny_c_ic=0.5, nz_c_ic=0.33)
INVISCID = dict(viscous=0, ic_form=1, riemann_solve_type=2, rho_c_ic=1.2, u_c_ic=30.0, v_c_ic=10.0, w_c_ic=0.0, p_c_ic=101325.0)

CASES = [
    case("wf_hex_p2_a", n=[3, 3, 1], amp=0.1, steps=1, level=2, order=2, bcs={"z-": "WallT", "z+": "Dual"}, **COMMON),
    case("wf_hex_p2_b", n=[3, 3, 1], amp=0.1, steps=1, level=2, order=2, bcs={"z-": "WallQ", "z+": "Slip"}, **COMMON),
    case("wf_quad_p3_a", dims=2, n=[4, 1], amp=0.1, steps=1, level=2, order=3, bcs={"y-": "WallQ", "y+": "Slip"}, **COMMON),
    case("wf_quad_p3_b", dims=2, n=[4, 1], amp=0.1, steps=1, level=2, order=3, bcs={"y-": "WallT", "y+": "Dual"}, **COMMON),
    case("wf_quad_p3_inviscid", dims=2, n=[4, 1], amp=0.1, steps=1, level=2, order=3, bcs={"y-": "Dual", "y+": "Slip"},
         **dict(COMMON, **INVISCID)),
]

# of the harness's level-2 dump: the state and the gradient CalcForces read, the residual sums that tie the runs together, and
# the small arrays (sizes, parameters, solution points, boundary records)
KEEP = ("u_step0_stage0", "s0_grad_disu_upts", "s0_res_sums", "u_init", "loc_upts", "sizes", "bc_flags", "bc_params")
SMALL = 64


def parse_history(path, n_fields, n_dims):
    """the last line of history.plt: iteration, log10 residuals, F totals, CL, CD, ..."""
    rows = [l for l in open(path).read().splitlines() if l and (l[0].isdigit() or l[0] == " ")]
    v = [float(x) for x in rows[-1].split(",")]
    res = np.array(v[1:1 + n_fields])
    F = np.array(v[1 + n_fields:1 + n_fields + n_dims])
    cl, cd = v[1 + n_fields + n_dims], v[2 + n_fields + n_dims]
    return int(v[0]), res, F, cl, cd


def parse_cp(path):
    """cp_*.dat -> (rows (n_rows, n_cols), labels (n_faces), first (n_faces): the row at which each labelled face begins)"""
    rows, labels, first = [], [], []
    for line in open(path).read().splitlines()[1:]:
        t = line.split()
        if not t:
            continue
        if t[0] in LABELS:
            labels.append(t[0])
            first.append(len(rows))
        else:
            rows.append([float(x) for x in t])
    return np.array(rows), labels, np.array(first, dtype=np.int64)


def capture(c):
    with tempfile.TemporaryDirectory() as td:
        xv = write_neu(os.path.join(td, "mesh.neu"), c["n"], c["dims"], amp=c["amp"], bcs=c.get("bcs"))
        keys = dict(c["keys"])
        keys["n_steps"] = c["steps"]
        if c["dims"] == 2:
            keys.pop("dz_cyclic")
        with open(os.path.join(td, "input"), "w") as f:
            for k, v in keys.items():
                f.write("%s %s\n" % (k, repr(v) if isinstance(v, float) else v))
        env = dict(os.environ, HIFILES_HOME=REF_HOME)
        for cmd in ([DRIVER, "input"], [HARNESS, "input", "dump.bin", str(c["steps"]), str(c["level"])]):
            r = subprocess.run(cmd, cwd=td, env=env, capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
                raise SystemExit("%s failed for %s" % (os.path.basename(cmd[0]), c["name"]))
        arrs = read_dump(os.path.join(td, "dump.bin"))
        sz = [int(v) for v in arrs["sizes"]]
        n_eles, n_upts, n_fields, n_dims = sz[0], sz[1], sz[3], sz[4]
        it, res, F, cl, cd = parse_history(os.path.join(td, "history.plt"), n_fields, n_dims)
        rows, labels, first = parse_cp(os.path.join(td, "force_files_%09d" % 1, "cp_%09d_p%04d.dat" % (1, 0)))

    # the two conditions
    n_wall = 2 * int(np.prod(c["n"])) // c["n"][-1]  # one cell between the two walls: two wall faces per element
    if len(labels) != n_wall:
        raise SystemExit("%s: the cp file labels %d faces, the mesh has %d wall faces" % (c["name"], len(labels), n_wall))
    want = np.log10(arrs["s0_res_sums"][:, 0] / (n_upts * n_eles))
    tie = float(np.abs(res - want).max())
    if it != 1 or not tie <= 1e-13:
        raise SystemExit("%s: driver and harness disagree: iteration %d, residual columns differ by %.2e" % (c["name"], it, tie))

    out = {k: v for k, v in arrs.items() if k in KEEP or v.size <= SMALL}
    if not c["keys"]["viscous"]:
        out.pop("s0_grad_disu_upts", None)
    out["xv"] = xv
    out["hist_res"], out["hist_F"], out["hist_CL"], out["hist_CD"] = res, F, np.array([cl]), np.array([cd])
    out["cp_rows"], out["cp_first"] = rows, first
    out["cp_labels"] = np.array(labels, dtype="U16")
    meta = dict(name=c["name"], n=c["n"], dims=c["dims"], amp=c["amp"], steps=c["steps"], level=c["level"], keys=c["keys"],
                bcs=c.get("bcs"), orient_seed=None, residual_tie=tie,
                generator="tools/capture_wall_forces.py via oracle/_ref/HiFiLES_ref and oracle/_ref/ref_harness (genuine reference)")
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    os.makedirs(GOLDEN, exist_ok=True)
    path = os.path.join(GOLDEN, c["name"] + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    if size > MAX_BYTES:
        raise SystemExit("%s: %d bytes, more than a committed file may have" % (path, size))
    print("%-22s %7.1f kB  %d faces, %d rows, residual tie %.1e" % (c["name"], size / 1e3, len(labels), len(rows), tie))


if __name__ == "__main__":
    want = sys.argv[1:]
    for c in CASES:
        if not want or c["name"] in want:
            capture(c)
