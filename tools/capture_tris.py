#!/usr/bin/env python3
"""Capture the triangle fixtures (tests/golden/tris/tri_*.npz) -- TEST INFRASTRUCTURE, container only.

Per case the genuine reference's harness (oracle/_ref/ref_harness) runs on a periodic box of n x n squares, each cut along the same
diagonal into two triangles (tests/tri_util.py: write_neu_tris; Gambit element type 3, 3 nodes, counter-clockwise), deformed through
gen_neu_mesh.box_vertices.  With orient_seed every element's node list is rotated by a seeded 0, 1 or 2 places.  tri_p3_cylinder
runs on the reference's own shipped mesh (714 six-node curved triangles), which is read where it lies and is not copied.

A file is written only if the restatement reproduces it on the CPU: tests/oracle_py in lockstep on the dumped inputs meets every
dumped state at the bars of tests/test_oracle_vs_golden.py (tests/tri_util.py: lockstep).

Nothing under oracle/ is written: everything runs in a temporary directory, and no bytecode cache is left.

    python tools/capture_tris.py            # all
    python tools/capture_tris.py tri_p3_bdy
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True  # (importing capture_golden would otherwise leave oracle/__pycache__)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gen_neu_mesh import box_vertices  # noqa: E402
from capture_golden import BASE, BC_KEYS, P_TGV, case, read_dump  # noqa: E402
import tri_util as T  # noqa: E402

REF_HOME = os.environ.get("HIFILES_HOME", "/root/reference")
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
GOLDEN = T.GOLDEN
MAX_BYTES = 1 << 20
CYLINDER_MESH = os.path.join(REF_HOME, "testcases", "navier-stokes", "cylinder", "cylinder_2ndorder_tri_vis.neu")

TRI_KEYS = dict(upts_type_tri=0, fpts_type_tri=0, vcjh_scheme_tri=1, c_tri=0.0)
assert BASE["sparse_tri"] == 0


def tri_case(name, **kw):
    kw.setdefault("amp", 0.1)
    return case(name, dims=2, **kw, **TRI_KEYS)


# the solver keys of the shipped input_cylinder_visc (P3, HLLC, RK34, CFL time step, LDG 0.5 / 0.5, Sutherland's law, uniform flow
# at Mach 1.1, a supersonic inlet and an isothermal wall); shock capturing and the monitors off
CYLINDER = dict(
    equation=0, viscous=1, riemann_solve_type=3, vis_riemann_solve_type=0, ic_form=1, test_case=0, order=3, dt_type=1, CFL=0.5,
    dt=0.0001, adv_type=2, ldg_beta=0.5, ldg_tau=0.5, mesh_file="mesh.neu", LES=0, restart_flag=0,
    p_res=2, write_type=0, monitor_res_freq=100000, plot_freq=100000000, restart_dump_freq=100000000, monitor_cp_freq=100000000,
    res_norm_type=1, error_norm_type=1, sparse_tri=0, sparse_quad=0, sparse_hexa=0, sparse_tet=0, sparse_pri=0,
    gamma=1.4, prandtl=0.72, S_gas=120.0, T_gas=291.15, R_gas=286.9, mu_gas=1.827e-05,
    Mach_free_stream=1.0, L_free_stream=1.0, T_free_stream=300.0, rho_free_stream=1.17723946, fix_vis=0,
    bc_Sup_In_type="sup_in", bc_Sup_In_p_static=101325.0, bc_Sup_In_mach=1.1, bc_Sup_In_T_static=300.0,
    bc_Isotherm_Fix_type="isotherm_wall", bc_Isotherm_Fix_T_static=300.0,
    Mach_c_ic=1.1, T_c_ic=300.0, rho_c_ic=1.17723946, shock_cap=0,
    # (an inlet group makes the reference's InitSolution read the interface-cubature metrics, which it sets up only when forces
    # are requested -- capture_golden.BC_KEYS)
    calc_force=1, area_ref=1.0, **TRI_KEYS)

CASES = [
    # the smallest element: 3 solution and 6 flux points
    tri_case("tri_p1_n4_deformed", n=4, level=1, order=1, steps=2),
    # every intermediate of one residual; element orientations mixed
    tri_case("tri_p2_n3_deformed", n=3, level=2, order=2, steps=1, orient_seed=2),
    # the shipped cases' order; 32 elements, every pair of local faces among the interior faces
    tri_case("tri_p3_n4_deformed", n=4, level=1, order=3, steps=2, orient_seed=3),
    tri_case("tri_p4_n2_deformed", n=2, level=1, order=4, steps=1),
    tri_case("tri_p5_n2_deformed", n=2, level=1, order=5, steps=1),
    # the run-wide physics switches, each against tri_p2_n3_deformed's mesh without the rotation
    tri_case("tri_p2_roem_sutherland", n=3, level=1, order=2, steps=1, riemann_solve_type=2, fix_vis=0, T_c_ic=350.0),
    tri_case("tri_p2_rusanov_ldg", n=3, level=1, order=2, steps=1, riemann_solve_type=0, ldg_tau=0.3, ldg_beta=0.25),
    # (the isentropic vortex of tet_p2_inviscid: the Taylor-Green state needs the viscous reference values -- with ic_form 7 and
    # viscous 0 the reference stops with "Residual is NaN" in its first residual)
    tri_case("tri_p2_inviscid", n=3, level=1, order=2, steps=1, viscous=0, ic_form=0, dt=0.001, rho_c_ic=1.0, u_c_ic=1.0, v_c_ic=1.0,
             w_c_ic=0.0, p_c_ic=1.0),
    tri_case("tri_p2_cfl_local", n=3, level=1, order=2, steps=2, dt_type=2, CFL=0.4, adv_type=0),
    # walls in y (isothermal moving, adiabatic), a characteristic far field and characteristic in- and outflow in x
    # (the cells of the x- side take the inlet and the far field in turn; the groups and keys are quad_p3_bdy's)
    tri_case("tri_p3_bdy", n=4, level=2, order=3, steps=1, bcs={"y-": "WallT", "y+": "WallQ", "x-": ["InR", "Far2"], "x+": "Out"},
             bc_Far2_type="char", bc_Far2_p_static=P_TGV, bc_Far2_mach=0.12, bc_Far2_T_static=295.0, bc_Far2_nx=0.8, bc_Far2_ny=0.6,
             **BC_KEYS),
    dict(name="tri_p3_cylinder", n=None, dims=2, amp=None, steps=2, level=1, keys=CYLINDER, bcs=None, orient_seed=None, mesh=CYLINDER_MESH,
         keep=("u_step1_stage3",)),
]
# the base case of each physics row (tests/test_tris_oracle.py: the row moves the final state)
PHYSICS_BASE = "tri_p2_base"
CASES.insert(5, tri_case(PHYSICS_BASE, n=3, level=1, order=2, steps=1))

# arrays of a dump that no triangle test reads (reference-element tables for the host-setup tests of the other classes)
DROP = ("tloc_fpts", "tnorm_fpts")


def capture(c):
    with tempfile.TemporaryDirectory() as td:
        if c.get("mesh"):
            shutil.copyfile(c["mesh"], os.path.join(td, "mesh.neu"))
            xv = None
        else:
            n = [c["n"], c["n"]] if isinstance(c["n"], int) else c["n"]
            xv = box_vertices(n, 2, amp=c["amp"])
            T.write_neu_tris(os.path.join(td, "mesh.neu"), n, xv, bcs=c.get("bcs"), orient_seed=c.get("orient_seed"))
        keys = dict(c["keys"])
        keys["n_steps"] = c["steps"]
        keys.pop("dz_cyclic", None)
        with open(os.path.join(td, "input"), "w") as f:
            for k, v in keys.items():
                f.write("%s %s\n" % (k, repr(v) if isinstance(v, float) else v))
        env = dict(os.environ, HIFILES_HOME=REF_HOME)
        r = subprocess.run([HARNESS, "input", "dump.bin", str(c["steps"]), str(c["level"])], cwd=td, env=env, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
            raise SystemExit("ref_harness failed for %s" % c["name"])
        arrs = read_dump(os.path.join(td, "dump.bin"))
    keep = c.get("keep")
    out = {k: v for k, v in arrs.items() if k not in DROP and (keep is None or not k.startswith("u_step") or k in keep)}
    if xv is not None:
        out["xv"] = xv
    meta = dict(name=c["name"], n=c["n"], dims=2, amp=c["amp"], steps=c["steps"], level=c["level"], keys=keys, bcs=c.get("bcs"),
                orient_seed=c.get("orient_seed"), mesh=os.path.basename(c["mesh"]) if c.get("mesh") else "tests/tri_util.py: write_neu_tris",
                generator="tools/capture_tris.py via oracle/_ref/ref_harness (genuine reference)")
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    # (the scalars of the viscous non-dimensionalisation, R_ref and uvw_ref, are unset in an inviscid run: arrays only)
    bad = [k for k, v in out.items() if v.dtype.kind == "f" and v.size > 1 and not np.isfinite(v).all()]
    if bad:
        raise SystemExit("%s: the reference's dump is not finite: %s" % (c["name"], bad))
    if int(out["sizes"][6]) != 0:
        raise SystemExit("%s: the reference ran element class %d, not triangles" % (c["name"], int(out["sizes"][6])))
    errs = T.lockstep(out)
    bad = T.failures(errs)
    if bad:
        raise SystemExit("%s: the restatement misses the reference: %s" % (c["name"], bad))
    os.makedirs(GOLDEN, exist_ok=True)
    path = os.path.join(GOLDEN, c["name"] + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    if size > MAX_BYTES:
        os.remove(path)
        raise SystemExit("%s: %d bytes, more than a committed file may have" % (path, size))
    worst = max(((k, v) for k, v in errs.items() if not k.startswith("nan_")), key=lambda kv: kv[1][0] / kv[1][1])
    print("%-26s %7.1f kB  %d elements, %d checks, worst %s %.1e (bar %.0e)" % (c["name"], size / 1e3, int(out["sizes"][0]), len(errs), worst[0],
                                                                                 worst[1][0], worst[1][1]))


if __name__ == "__main__":
    want = sys.argv[1:]
    for c in CASES:
        if not want or c["name"] in want:
            capture(c)
