#!/usr/bin/env python3
"""Capture the integral-history fixtures (tests/golden/integral_history/ih_*.npz) -- TEST INFRASTRUCTURE, container only.

Per case the genuine reference that `build()` compiles into oracle/_ref runs twice on the same mesh.neu and input: the DRIVER
(oracle/_ref/HiFiLES_ref), whose main loop fills the Diagnostics[...] columns of history.plt at step 1 and every
monitor_res_freq steps (src/HiFiLES.cpp:247-266), and the HARNESS (oracle/_ref/ref_harness, level 2), which records the arrays
a device block is built from, the cubature of the monitor and the state after every step.  A fixture holds the harness's arrays
without the intermediates of its first residual and the driver's rows: iteration, diagnostics, time.

What the rows pin: the reference integrates the state AFTER the step against grad_disu_upts as the step's last RK stage left it,
the corrected gradient of that stage's INPUT state.  Two conditions are enforced before a file is written, on the CPU:
  1. the two runs are one: numpy on the harness's state after step 1 with the fixture's cubature gives the driver's row-1 kinetic
     energy within the 15 digits history.plt prints;
  2. the pairing is visible: through the oracle (tests/oracle_py.py) the enstrophy of every sampled row formed with the gradient of
     the sampled state ITSELF differs from the driver's by more than 1e-6 relative, while formed with the last stage's gradient it
     agrees within 1e-11 (of the row's largest value).
Amplitude and dt are those of the neighbouring *_integrals cases of oracle/capture_golden.py, except where condition 2 asked for a
larger dt: the value and the reason stand beside the case.

Nothing under oracle/ is written: everything runs in a temporary directory, and no bytecode cache is left.

    python tools/capture_integral_history.py            # all five
    python tools/capture_integral_history.py ih_quad_p3_rk45
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from capture_golden import BC_KEYS, TET_KEYS, case, read_dump, write_neu, write_neu_tets  # noqa: E402
import integral_history_util as IU  # noqa: E402

REF_HOME = os.environ.get("HIFILES_HOME", "/root/reference")
DRIVER = os.path.join(ROOT, "oracle", "_ref", "HiFiLES_ref")
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
# a directory of their own: the suites that run every tests/golden/*.npz as a whole case do not take these
GOLDEN = IU.IH_DIR
MAX_BYTES = 1 << 20

ALL_FIVE = "5 kineticenergy enstropy pressuredilatation straincolonproduct devstraincolonproduct"
THREE = "3 enstropy kineticenergy devstraincolonproduct"

CASES = [
    # (dt: twenty times hex_p2_integrals' 1.440389e-05, with which the own-gradient enstrophy differs by 3.8e-07 only, and by
    # 1.7e-07 with five times that; at a hundred times the reference aborts)
    case("ih_hex_p2_rk45", amp=0.15, steps=5, level=2, order=2, adv_type=3, monitor_res_freq=2, integral_quantities=ALL_FIVE,
         dt=2.880778e-04),
    case("ih_hex_p2_euler", amp=0.15, steps=2, level=2, order=2, adv_type=0, monitor_res_freq=1, integral_quantities=ALL_FIVE),
    # (dt: thirty times quad_p3_integrals' 1.440389e-05, with which the own-gradient enstrophy differs by 6.8e-08 only)
    case("ih_quad_p3_rk45", dims=2, n=4, amp=0.1, steps=4, level=2, order=3, adv_type=3, monitor_res_freq=3,
         integral_quantities=THREE, dt=4.321167e-04),
    # the gradient goes through the boundary LDG path: one cell between an isothermal wall and a slip wall, as wf_hex_p2_a
    case("ih_hex_p2_walls", n=[3, 3, 1], amp=0.1, steps=2, level=2, order=2, adv_type=3, integral_quantities=ALL_FIVE,
         bcs={"z-": "WallT", "z+": "Dual"}, **dict(BC_KEYS, monitor_res_freq=2)),
    case("ih_tet_p2_rk45", n=2, amp=0.1, steps=2, level=2, order=2, adv_type=3, monitor_res_freq=2, tets=True,
         integral_quantities=ALL_FIVE, **TET_KEYS),
]


def parse_history(path, n_fields, n_dims, calc_force, n_diags):
    """history.plt -> (iterations, diagnostics (n_rows, n_diags), times): src/output.cpp:2375-2402"""
    rows = [l for l in open(path).read().splitlines() if l and (l[0].isdigit() or l[0] == " ")]
    it, diag, time = [], [], []
    first = 1 + n_fields + ((n_dims + 2) if calc_force else 0)
    for l in rows:
        v = [float(x) for x in l.split(",")]
        assert len(v) == first + n_diags + 2, l
        it.append(int(v[0]))
        diag.append(v[first:first + n_diags])
        time.append(v[first + n_diags])
    return np.array(it, dtype=np.int32), np.array(diag), np.array(time)


def capture(c):
    with tempfile.TemporaryDirectory() as td:
        mesh = os.path.join(td, "mesh.neu")
        if c.get("tets"):
            xv = write_neu_tets(mesh, c["n"], amp=c["amp"])
        else:
            xv = write_neu(mesh, c["n"], c["dims"], amp=c["amp"], bcs=c.get("bcs"))
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
        n_fields, n_dims, n_stages = sz[3], sz[4], sz[7]
        ids = np.ravel(arrs["integral_quantity_ids"])
        it, diag, time = parse_history(os.path.join(td, "history.plt"), n_fields, n_dims, int(keys.get("calc_force", 0)), len(ids))

    freq, steps = int(keys["monitor_res_freq"]), c["steps"]
    want_rows = IU.sample_steps(0, steps, freq)
    if list(it) != want_rows:
        raise SystemExit("%s: history.plt has rows at %s, the sampling rule gives %s" % (c["name"], list(it), want_rows))
    last = n_stages - 1
    out = {k: v for k, v in arrs.items() if not (k.startswith("s0_") or k.startswith("u_step"))}
    out["s0_grad_disu_upts"] = arrs["s0_grad_disu_upts"]
    out["s0_integral_quantities"] = arrs["s0_integral_quantities"]
    for s in range(steps):
        out["u_step%d_stage%d" % (s, last)] = arrs["u_step%d_stage%d" % (s, last)]
    # the time of a row: the driver prints time x time_ref on a viscous case (src/output.cpp:2394-2402), time_ref = L_ref / uvw_ref
    time_ref = float(keys["L_free_stream"]) / IU.scalar(arrs, "uvw_ref")
    dt = IU.scalar(arrs, "dt")
    t, t_rows = 0.0, []
    for s in range(1, steps + 1):
        t += dt
        if s in want_rows:
            t_rows.append(t * time_ref)
    if not np.all(np.abs(time - np.array(t_rows)) <= 1e-14 * np.abs(time)):
        raise SystemExit("%s: the driver's times %s are not step x dt x time_ref %s" % (c["name"], time, t_rows))
    out["hist_iter"], out["hist_diag"], out["hist_time"], out["time_ref"] = it, diag, time, np.array([time_ref])
    out["monitor_res_freq"] = np.array([freq], dtype=np.int32)

    # condition 1: the two runs are one
    ke_col = int(np.where(ids == 0)[0][0])
    ke = IU.fixture_quantities(out, arrs["u_step0_stage%d" % last], None, ids=[0])[0]
    tie = abs(ke - diag[0, ke_col]) / abs(diag[0, ke_col])
    if not tie <= 1e-14:  # (15 printed digits)
        raise SystemExit("%s: driver and harness disagree: kinetic energy of row 1 differs by %.2e" % (c["name"], tie))
    # condition 2: the pairing is visible (and the oracle, paired as the reference pairs, gives the rows)
    ens_col = int(np.where(ids == 1)[0][0])
    run = IU.OracleRun(out)
    paired, own = [], []
    for s in range(1, steps + 1):
        run.step()
        if s not in want_rows:
            continue
        row = diag[want_rows.index(s)]
        got = IU.fixture_quantities(out, run.u, run.grad)
        paired.append(float(np.abs(got - row).max() / np.abs(row).max()))
        ens = IU.fixture_quantities(out, run.u, run.own_gradient(), ids=[1])[0]
        own.append(abs(ens - row[ens_col]) / abs(row[ens_col]))
    if not max(paired) <= 1e-11:
        raise SystemExit("%s: the oracle with the last stage's gradient misses the driver's rows by %.2e" % (c["name"], max(paired)))
    if not min(own) > 1e-6:
        raise SystemExit("%s: the enstrophy with the sampled state's own gradient differs by %.2e only: raise dt or the amplitude"
                         % (c["name"], min(own)))

    out["xv"] = xv
    meta = dict(name=c["name"], n=c["n"], dims=c["dims"], amp=c["amp"], steps=steps, level=c["level"], keys=c["keys"],
                bcs=c.get("bcs"), orient_seed=None, kinetic_energy_tie=tie, rows_paired=paired, enstrophy_own_gradient=own,
                generator="tools/capture_integral_history.py via oracle/_ref/HiFiLES_ref and oracle/_ref/ref_harness (genuine reference)")
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    os.makedirs(GOLDEN, exist_ok=True)
    path = os.path.join(GOLDEN, c["name"] + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    if size > MAX_BYTES:
        raise SystemExit("%s: %d bytes, more than a committed file may have" % (path, size))
    print("%-18s %7.1f kB  rows at %s, tie %.1e, paired %.1e, own gradient misses the enstrophy by %.1e"
          % (c["name"], size / 1e3, [int(i) for i in it], tie, max(paired), min(own)))


if __name__ == "__main__":
    want = sys.argv[1:]
    for c in CASES:
        if not want or c["name"] in want:
            capture(c)
