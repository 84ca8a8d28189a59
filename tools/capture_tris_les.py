#!/usr/bin/env python3
"""Capture the fixtures of the LES closure on triangles (tests/golden/tris_les/tl_*.npz) -- TEST INFRASTRUCTURE, container only.

The genuine reference's harness (oracle/_ref/ref_harness) runs triangle cases with LES 1 (eles::calc_sgsf_upts, src/eles.cpp:2395-2650;
eles_tris::compute_filter_upts, src/eles_tris.cpp:786-970) and dumps the closure's keys, Jacobian_fpts and, by model, wall_distance and
filter_upts.  Per case it runs at level 1 on the mesh and keys of a fixture of tests/golden/tris with the case's closure, two steps each.
A file is a DELTA file: the closure's keys and arrays, the states after every step (the cylinder: after the last), s0_div_tconf_upts,
dt_step*, meta_json, based_on.  The tool asserts that every array it does not store equals the base fixture's bit for bit
(tests/tri_les_util.py loads a file on top of its base).  tl_p3_smag_walls runs on a mesh of its own (a 4 x 4 box, periodic in x,
an isothermal moving wall at y- and an adiabatic one at y+, with the boundary keys of hex_p2_les_smag) and is stored whole, with the
wall-face cubature of the reference (HFX_DUMP_INTERS_CUBPTS) for the wall forces of a history row.

Filter types: 2 (modal) and 3 (element average) only -- filter_type 0 is a FatalError on triangles and type 1 indexes
weight_volume_cubpts by solution point.

A file is written only if (tests/tri_les_util.py: conditions)
  1. the oracle in lockstep (general_util.oracle_steps) meets every dumped state at tri_util's bars;
  2. the run with the closure removed differs from the fixture's final state by more than MOVED = 1e-7 of max |u| (10^4 times the GPU
     bar: a stage that silently skips the closure cannot pass);
  3. Jacobian_fpts . JGinv_fpts = detjac_fpts I at every flux point below 1e-12 of max |detjac_fpts| (printed);
  4. tl_p3_smag_walls: y^2 Kappa^2 is the smaller length scale at some solution points and C_s^2 Delta^2 at others;
  5. the similarity cases: Lu / Le are non-zero.
Every case meets 2. with the keys of the hexahedral fixtures (C_s 0.325 and filter_ratio 1 or 2; Smagorinsky 0.17 and 1.5): none was
re-keyed.  Each case's keys are in CASES below and in its meta_json.

tl_p3_cylinder_shock (capture_shock) is the closure beside shock capturing: the keys of ts_p3_cylinder's driver run (the shipped
viscous cylinder case: shock_cap 1, s0 0.001, restart and Tecplot files after every step) + the WALE closure through the genuine DRIVER
(oracle/_ref/HiFiLES_ref), read as tools/capture_tris_shock.py reads it.  Written only if (tests/tri_les_util.py: shock_conditions) the
oracle with both ingredients meets the restart state at 1e-12 and the Tecplot sensor at 1e-10, no sensor of any stage lies within 5e-4
of s0, some stage filters some elements and not all, the state moves by more than 1e-7 without the closure and the Jacobian identity
holds.  As captured: state 2.4e-15, sensor 6.8e-15, closest sensor 2.4e-3, filtered 0 / 11 / 0 / 0 / 12 / 2 / 4 / 8 of 714, moved 4.6e-3.

Nothing under oracle/ or tests/golden/tris is written: everything runs in a temporary directory, and no bytecode cache is left.

    python tools/capture_tris_les.py            # all
    python tools/capture_tris_les.py tl_p3_wale
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from capture_tris import BC_KEYS, CYLINDER_MESH, DROP, HARNESS, MAX_BYTES, REF_HOME, box_vertices, read_dump, tri_case  # noqa: E402
import tri_util as T  # noqa: E402
import tri_les_util as TL  # noqa: E402

N_STEPS = 2
WALE = dict(LES=1, SGS_model=1, C_s=0.325, filter_ratio=1.0)
CASES = [
    dict(name="tl_p1_wale", base="tri_p1_n4_deformed", les=WALE),
    dict(name="tl_p2_wale", base="tri_p2_n3_deformed", les=WALE),
    dict(name="tl_p3_wale", base="tri_p3_n4_deformed", les=WALE),
    dict(name="tl_p4_wale", base="tri_p4_n2_deformed", les=WALE),
    dict(name="tl_p5_wale", base="tri_p5_n2_deformed", les=WALE),
    dict(name="tl_p3_smag_walls", whole=tri_case("tl_p3_smag_walls", n=4, level=1, order=3, steps=N_STEPS, orient_seed=3,
                                                 bcs={"y-": "WallT", "y+": "WallQ"}, LES=1, SGS_model=0, C_s=0.17, filter_ratio=1.5, **BC_KEYS)),
    dict(name="tl_p3_wsm", base="tri_p3_n4_deformed", les=dict(LES=1, SGS_model=2, C_s=0.325, filter_ratio=2.0, filter_type=2)),
    dict(name="tl_p3_sim", base="tri_p3_n4_deformed", les=dict(LES=1, SGS_model=4, C_s=0.325, filter_ratio=2.0, filter_type=3)),
    dict(name="tl_p3_svv", base="tri_p3_n4_deformed", les=dict(LES=1, SGS_model=3, C_s=0.325, filter_ratio=2.0, filter_type=2)),
    dict(name="tl_p3_cylinder", base="tri_p3_cylinder", les=dict(WALE, shock_cap=0), last_only=True),
]


def identical(a, b):
    """bit for bit; the scalars an inviscid run leaves unset are NaN in both"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def harness(td, keys, steps, name, env=None):
    with open(os.path.join(td, "input"), "w") as f:
        for k, v in keys.items():
            f.write("%s %s\n" % (k, repr(v) if isinstance(v, float) else v))
    r = subprocess.run([HARNESS, "input", "dump.bin", str(steps), "1"], cwd=td, env=dict(os.environ, HIFILES_HOME=REF_HOME, **(env or {})),
                       capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
        raise SystemExit("ref_harness failed for %s" % name)
    return read_dump(os.path.join(td, "dump.bin"))


def capture(c):
    whole = c.get("whole")
    base = None if whole else T.load(c["base"])
    meta0 = whole if whole else json.loads(bytes(base["meta_json"]).decode())
    keys = dict(meta0["keys"])
    keys.update(c.get("les", {}))
    keys["n_steps"] = N_STEPS
    keys.pop("dz_cyclic", None)
    xv = None
    with tempfile.TemporaryDirectory() as td:
        if meta0.get("n") is None:
            shutil.copyfile(CYLINDER_MESH, os.path.join(td, "mesh.neu"))
        else:
            n = [meta0["n"], meta0["n"]] if isinstance(meta0["n"], int) else meta0["n"]
            xv = box_vertices(n, 2, amp=meta0["amp"])
            T.write_neu_tris(os.path.join(td, "mesh.neu"), n, xv, bcs=meta0.get("bcs"), orient_seed=meta0.get("orient_seed"))
        # (the walls: with the wall-face cubature as the reference formed it, for the wall forces of a history row -- the host mirror
        # builds none on triangles; tests/full_loop_util.py: fixture_device_arrays)
        arrs = harness(td, keys, N_STEPS, c["name"], {"HFX_DUMP_INTERS_CUBPTS": "1"} if whole else None)
    if base is not None and int(np.ravel(arrs["adv_type"])[0]) < 3:  # (only the low-storage schemes read RK_a / RK_b)
        arrs["RK_a"], arrs["RK_b"] = base["RK_a"], base["RK_b"]
    nstage = int(arrs["sizes"][7])
    last = tuple("u_step%d_stage%d" % (s, nstage - 1) for s in range(N_STEPS - 1 if c.get("last_only") else 0, N_STEPS))
    full = {k: v for k, v in arrs.items() if k not in DROP and (not k.startswith("u_step") or k in last)}
    bad = [k for k, v in full.items() if v.dtype.kind == "f" and v.size > 1 and not np.isfinite(v).all()]
    if bad:
        raise SystemExit("%s: the reference's dump is not finite: %s" % (c["name"], bad))
    if int(full["sizes"][6]) != 0:
        raise SystemExit("%s: the reference ran element class %d, not triangles" % (c["name"], int(full["sizes"][6])))
    assert int(np.ravel(full["LES"])[0]) == 1 and int(np.ravel(full["SGS_model"])[0]) == keys["SGS_model"]

    if whole:
        out, same = dict(full), []
        out["xv"] = xv
        d = dict(out)
    else:
        out, same = {}, []
        for k, v in full.items():
            if k in TL.LES_KEYS or k.startswith(TL.RESULTS):
                out[k] = v
            elif k in base and identical(v, base[k]):
                same.append(k)
            else:
                raise SystemExit("%s: the harness's %s is not the base fixture's" % (c["name"], k))
        gone = [k for k in base if k not in full and not k.startswith(TL.STALE) and k != "xv"]
        assert not gone, "%s: the base fixture's %s are not in the dump" % (c["name"], gone)
        out["based_on"] = np.frombuffer(c["base"].encode(), dtype=np.uint8)
        d = TL.overlay(base, out)
        for k, v in full.items():
            assert identical(d[k], v), k
    meta = dict(name=c["name"], based_on=c.get("base"), steps=N_STEPS, level=1, keys=keys, stored=sorted(out),
                n=meta0.get("n"), amp=meta0.get("amp"), bcs=meta0.get("bcs"), orient_seed=meta0.get("orient_seed"),
                generator="tools/capture_tris_les.py via oracle/_ref/ref_harness (genuine reference)")

    # ---- the conditions, on what a test will load
    cond = TL.conditions(d, c["name"])
    if cond["failures"]:
        raise SystemExit("%s: not written: %s" % (c["name"], cond["failures"]))
    meta.update({k: v for k, v in cond.items() if k != "failures"})
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    os.makedirs(TL.GOLDEN, exist_ok=True)
    path = os.path.join(TL.GOLDEN, c["name"] + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    if size > MAX_BYTES:
        os.remove(path)
        raise SystemExit("%s: %d bytes, more than a committed file may have" % (path, size))
    extra = "".join(", %s %s" % (k, cond[k]) for k in ("wall_points", "grid_points", "Lu", "Le") if k in cond)
    print("%-18s %6.1f kB  %d elements, model %d, lockstep worst %s %.1e, moved %.1e, Jacobian identity %.1e%s; %d arrays stored, %d the base's"
          % (c["name"], size / 1e3, int(d["sizes"][0]), TL.model(d), cond["worst"][0], cond["worst"][1], cond["moved"], cond["jacobian"], extra,
             len(out), len(same)))


def capture_shock():
    """tl_p3_cylinder_shock: the keys ts_p3_cylinder's driver run had (the shipped viscous cylinder case with shock_cap 1, restart and
    Tecplot files after every step) + the WALE closure, through the genuine driver; the state of the last step's restart file and the
    sensor column after every step.  Every array of the block is ts_p3_cylinder's or tl_p3_cylinder's (tests/tri_les_util.py:
    compose_shock), so the file holds the closure's scalars and the driver's results alone"""
    from capture_tris_shock import DRIVER, parse_restart, parse_sensor, run, write_input  # (imports the library's Python layer)
    import glob
    import tri_shock_util as TS
    shock_from, les_from = "ts_p3_cylinder", "tl_p3_cylinder"
    smeta = json.loads(bytes(np.load(os.path.join(TS.GOLDEN, shock_from + ".npz"))["meta_json"]).decode())
    steps = int(smeta["steps"])
    dkeys = dict(smeta["keys"], **WALE)
    les = TL.load(les_from)
    sz = [int(v) for v in les["sizes"]]
    ne, nu, nf = sz[0], sz[1], sz[3]
    with tempfile.TemporaryDirectory() as td:
        shutil.copyfile(CYLINDER_MESH, os.path.join(td, "mesh.neu"))
        write_input(os.path.join(td, "input"), dkeys)
        run([DRIVER, "input"], td, TL.SHOCK)
        u_rest = parse_restart(os.path.join(td, "Rest_%09d_p0000.dat" % steps), ne, nu, nf)
        plt = {int(os.path.basename(p).split("_")[1]): p for p in glob.glob(os.path.join(td, "Mesh_*_p0000.plt"))}
        sens = [parse_sensor(plt[s], ne) for s in range(1, steps + 1)]
    out = {k: les[k] for k in TL.LES_SCALARS}
    out.update(shock_from=np.frombuffer(shock_from.encode(), dtype=np.uint8), les_from=np.frombuffer(les_from.encode(), dtype=np.uint8),
               restart_steps=np.array([steps], dtype=np.int32), u_restart=np.stack([u_rest]), sensor_rows=np.stack(sens))
    cond, _ = TL.shock_conditions(TL.compose_shock(out))
    if cond["failures"]:
        raise SystemExit("%s: not written: %s (all figures: %s)" % (TL.SHOCK, cond["failures"], cond))
    meta = dict(name=TL.SHOCK, shock_from=shock_from, les_from=les_from, steps=steps, keys=dkeys, n_eles=ne,
                generator="tools/capture_tris_les.py via oracle/_ref/HiFiLES_ref (genuine reference)", **{k: v for k, v in cond.items() if k != "failures"})
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(TL.GOLDEN, TL.SHOCK + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    if size > MAX_BYTES:
        os.remove(path)
        raise SystemExit("%s: %d bytes, more than a committed file may have" % (path, size))
    print("%-18s %6.1f kB  %d elements, s0 %.4e, filtered %s, closest %.1e, state %.1e, sensor %.1e, moved %.1e, Jacobian identity %.1e"
          % (TL.SHOCK, size / 1e3, ne, smeta["s0"], cond["filtered_per_stage"], cond["closest_sensor_to_s0"], cond["state"], cond["sensor"],
             cond["moved"], cond["jacobian"]))


if __name__ == "__main__":
    want = sys.argv[1:]
    for c in CASES:
        if not want or c["name"] in want:
            capture(c)
    if not want or TL.SHOCK in want:
        capture_shock()  # (behind tl_p3_cylinder, whose arrays it takes)
