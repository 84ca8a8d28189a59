#!/usr/bin/env python3
"""Capture the mixed quadrilateral / triangle fixtures (tests/golden/mixed2d/mx_*.npz) -- TEST INFRASTRUCTURE, container only.

Per case the genuine reference's harness (oracle/_ref/ref_harness, unchanged) runs on a periodic 4 x 4 box of squares of which some
stay quadrilaterals and the others are cut into two triangles (tests/mixed2d_util.py: write_neu_mixed2d), deformed through
gen_neu_mesh.box_vertices.  The harness dumps a mesh of two element classes for the plain Navier-Stokes / Euler path.

A file is written only if the restatement reproduces it on the CPU: tests/mixed_util.MixedOracle in lockstep on the dumped inputs
meets every dumped state of both classes at the bars of tests/tri_util.py (tests/mixed2d_util.py: lockstep), and only if the
interior faces show the class pairs the case claims.

Nothing under oracle/ is written: everything runs in a temporary directory, and no bytecode cache is left.

    python tools/capture_mixed2d.py            # all
    python tools/capture_mixed2d.py mx_p3_walls
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gen_neu_mesh import box_vertices  # noqa: E402
from capture_golden import BC_KEYS, P_TGV, case, read_dump  # noqa: E402
import mixed2d_util as X  # noqa: E402
import tri_util as T  # noqa: E402

REF_HOME = os.environ.get("HIFILES_HOME", "/root/reference")
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
MAX_BYTES = 1 << 20
TRI_KEYS = dict(upts_type_tri=0, fpts_type_tri=0, vcjh_scheme_tri=1, c_tri=0.0)
ALL_PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1)]
HALF_PAIRS = [(0, 0), (1, 0), (1, 1)]  # (layout "half": every cross face has the quadrilateral on its left)


def mx_case(name, layout, pairs, **kw):
    kw.setdefault("amp", 0.1)
    c = case(name, dims=2, n=4, **kw, **TRI_KEYS)
    c["layout"], c["pairs"] = layout, pairs
    return c


CASES = [
    mx_case("mx_p1_n4", "checker", ALL_PAIRS, level=1, order=1, steps=2),
    # every intermediate of one residual
    mx_case("mx_p2_n4", "half", HALF_PAIRS, level=2, order=2, steps=1),
    mx_case("mx_p3_n4", "checker", ALL_PAIRS, level=1, order=3, steps=2),
    mx_case("mx_p4_n4", "half", HALF_PAIRS, level=1, order=4, steps=1),
    # quadrilateral rows on both walls, triangles between: walls in y (isothermal moving, adiabatic), characteristic in- and
    # outflow and a far field in x (the groups and keys of tri_p3_bdy); claimed: both like pairs and at least one cross pair
    mx_case("mx_p3_walls", "walls", [(0, 0), (1, 1)], level=1, order=3, steps=1, bcs={"y-": "WallT", "y+": "WallQ", "x-": ["InR", "Far2"], "x+": "Out"},
            bc_Far2_type="char", bc_Far2_p_static=P_TGV, bc_Far2_mach=0.12, bc_Far2_T_static=295.0, bc_Far2_nx=0.8, bc_Far2_ny=0.6, **BC_KEYS),
    # the run-wide physics switches, each against mx_p2_n4 (the keys of the triangle fixtures of these names)
    mx_case("mx_p2_inviscid", "half", HALF_PAIRS, level=1, order=2, steps=1, viscous=0, ic_form=0, dt=0.001, rho_c_ic=1.0, u_c_ic=1.0, v_c_ic=1.0,
            w_c_ic=0.0, p_c_ic=1.0),
    mx_case("mx_p2_roem_sutherland", "half", HALF_PAIRS, level=1, order=2, steps=1, riemann_solve_type=2, fix_vis=0, T_c_ic=350.0),
    mx_case("mx_p2_rusanov_ldg", "half", HALF_PAIRS, level=1, order=2, steps=1, riemann_solve_type=0, ldg_tau=0.3, ldg_beta=0.25),
]

# arrays of a dump that no test here reads (reference-element tables for the host-setup tests of the other classes)
DROP = ("tloc_fpts", "tnorm_fpts")


def capture(c):
    with tempfile.TemporaryDirectory() as td:
        n = [c["n"], c["n"]]
        xv = box_vertices(n, 2, amp=c["amp"])
        X.write_neu_mixed2d(os.path.join(td, "mesh.neu"), n, xv, c["layout"], bcs=c.get("bcs"))
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
    out = {k: v for k, v in arrs.items() if not k.endswith(DROP)}
    out["xv"] = xv
    meta = dict(name=c["name"], n=c["n"], dims=2, amp=c["amp"], steps=c["steps"], level=c["level"], keys=keys, bcs=c.get("bcs"), layout=c["layout"],
                mesh="tests/mixed2d_util.py: write_neu_mixed2d", generator="tools/capture_mixed2d.py via oracle/_ref/ref_harness (genuine reference)")
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    bad = [k for k, v in out.items() if v.dtype.kind == "f" and v.size > 1 and not np.isfinite(v).all()]
    if bad:
        raise SystemExit("%s: the reference's dump is not finite: %s" % (c["name"], bad))
    if "classes" not in out or sorted(int(v) for v in out["classes"]) != [0, 1]:
        raise SystemExit("%s: the reference did not run triangles and quadrilaterals (classes %s)" % (c["name"], out.get("classes")))
    census = X.pair_census(out)
    if not set(c["pairs"]) <= set(census) or not any(a != b for a, b in census):
        raise SystemExit("%s: the interior faces show the class pairs %s, the case claims %s" % (c["name"], census, c["pairs"]))
    errs = X.lockstep(out)
    bad = T.failures(errs)
    if bad:
        raise SystemExit("%s: the restatement misses the reference: %s" % (c["name"], bad))
    os.makedirs(X.GOLDEN, exist_ok=True)
    path = os.path.join(X.GOLDEN, c["name"] + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    if size > MAX_BYTES:
        os.remove(path)
        raise SystemExit("%s: %d bytes, more than a committed file may have" % (path, size))
    worst = max(((k, v) for k, v in errs.items() if not k.startswith("nan_")), key=lambda kv: kv[1][0] / kv[1][1])
    print("%-24s %7.1f kB  %d + %d elements, pairs %s, %d checks, worst %s %.1e (bar %.0e)"
          % (c["name"], size / 1e3, X.sizes(out, 0)[0], X.sizes(out, 1)[0], census, len(errs), worst[0], worst[1][0], worst[1][1]))


if __name__ == "__main__":
    want = sys.argv[1:]
    for c in CASES:
        if not want or c["name"] in want:
            capture(c)
