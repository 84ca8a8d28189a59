#!/usr/bin/env python3
"""Capture the wall-model fixtures (tests/golden/wall_model/wm_*.npz) -- TEST INFRASTRUCTURE, container only.

Per case the genuine reference's harness (oracle/_ref/ref_harness, level 2, two RK45 steps) runs a channel between an isothermal and
an adiabatic no-slip wall with `wall_model 1 | 2` and `bc_<group>_use_wm 1`.  The fluid is the Taylor-Green one with a larger
viscosity (mu_gas), so that the model's Reynolds numbers lie on both sides of Werner-Wengle's switch at 11.81^2.

The two-dimensional cases run on a MOVED mesh.  The committed generator only shears quadrilaterals into parallelograms, on which
the whole far row of solution points ties for the largest wall distance and the reference's pick of the model's input point is
decided by rounding.  Here the generator's vertices are wrapped, in this process only, around the write_neu call: every interior
vertex moves by a seeded offset, the wall rows stay and the two x-periodic images move alike.  The moved vertices are stored as xv.

A file is written only if, on the restatement of tests/wall_model_util.py:
  * on every model face the largest and second-largest dist_min differ by more than 1e-6 relative (no tie in the input point);
  * no Rey lies within 1e-6 relative of 11.81^2;
  * in model-2 files neither the last nor the next-to-last |dutau| lies in [0.5e-6, 2e-6];
  * each model-1 family (hex, quad) has at least a quarter of its points, or for the quads at least 4, on each branch;
  * the restatement reproduces the reference's wall flux: inv + fn . tdA equals s0_norm_tconf_fpts within 1e-13 of the block's
    largest |norm_tconf| at the model faces.

Nothing under oracle/ is written: everything runs in a temporary directory, and no bytecode cache is left.

    python tools/capture_wall_model.py            # all
    python tools/capture_wall_model.py wm_quad_p3_ww
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
import gen_neu_mesh  # noqa: E402
from capture_golden import BC_KEYS, case, read_dump, write_neu  # noqa: E402
import wall_model_util as W  # noqa: E402

REF_HOME = os.environ.get("HIFILES_HOME", "/root/reference")
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
GOLDEN = os.path.join(ROOT, "tests", "golden", "wall_model")
MAX_BYTES = 1 << 20
# the interior vertices of the quad meshes move by up to this fraction of a cell.  Of the seeds 1-9, 1, 3 and 9 pass every condition
# below for both quad cases; 9 has the most even split between Werner-Wengle's branches (12 / 20 points)
MOVE_SEED, MOVE_FRACTION = 9, 0.06

WM = dict(BC_KEYS, bc_WallT_use_wm=1, bc_WallQ_use_wm=1)
HEX = dict(n=[3, 3, 2], amp=0.1, steps=2, level=2, order=2, bcs={"z-": "WallT", "z+": "WallQ"}, mu_gas=4e-4)
QUAD = dict(dims=2, n=[4, 3], amp=0.1, steps=2, level=2, order=3, bcs={"y-": "WallT", "y+": "WallQ"}, mu_gas=1e-4, move=True)


def wm_case(name, base, **over):
    base = dict(base)
    move = base.pop("move", False)
    keys = dict(WM)
    keys.update(over)
    c = case(name, **base, **keys)
    c["move"] = move
    return c


CASES = [
    wm_case("wm_hex_p2_ww", HEX, wall_model=1),
    wm_case("wm_hex_p2_br", HEX, wall_model=2),
    wm_case("wm_hex_p2_ww_sutherland", HEX, wall_model=1, fix_vis=0),
    # a wall without the model (the adiabatic one) beside a wall with it in the same face block
    wm_case("wm_hex_p2_ww_wale", HEX, wall_model=1, LES=1, SGS_model=1, C_s=0.325, filter_ratio=1.0, bc_WallQ_use_wm=0),
    wm_case("wm_quad_p3_ww", QUAD, wall_model=1),
    wm_case("wm_quad_p3_br", QUAD, wall_model=2),
]

# of the harness's level-2 dump everything but the large intermediates of the first residual that no wall-model test reads
DROP = ("s0_grad_disu_upts_ref", "s0_grad_disu_upts", "s0_grad_disu_fpts", "s0_tdisf_upts_inv", "s0_tdisf_upts", "s0_norm_tdisf_fpts",
        "s0_div_tconf_upts_disc", "s0_sgsf_upts", "s0_sgsf_fpts")


def moved_vertices(n, dims, seed=MOVE_SEED, fraction=MOVE_FRACTION):
    """box_vertices wrapped: the interior rows of a 2-D box move by a seeded offset; walls (first and last row in y) stay, the
    vertices at x = 0 and x = length move alike"""
    plain = gen_neu_mesh.box_vertices

    def wrapped(nn, dd, length=2.0 * np.pi, amp=0.0):
        xv = plain(nn, dd, length, amp)
        if dd != 2:
            return xv
        nx, ny = nn[0], nn[1]
        rng = np.random.RandomState(seed)
        off = (rng.rand(ny + 1, nx + 1, 2) - 0.5) * 2.0 * fraction * np.array([length / nx, length / ny])
        off[0], off[ny] = 0.0, 0.0
        off[:, nx] = off[:, 0]
        return xv + off.reshape(-1, 2)

    return plain, wrapped


def check(c, arrs):
    """the conditions of the module docstring; returns the census"""
    cen = W.census(arrs)
    name = c["name"]
    if not cen["gap"] > 1e-6:
        raise SystemExit("%s: the input point of a face ties (relative gap %.2e)" % (name, cen["gap"]))
    if cen["model"] == 1:
        if not cen["rey_margin"] > 1e-6:
            raise SystemExit("%s: a Rey lies at the switch (margin %.2e)" % (name, cen["rey_margin"]))
        need = 4 if c["dims"] == 2 else (cen["n_points"] + 3) // 4
        if min(cen["laminar"], cen["turbulent"]) < need:
            raise SystemExit("%s: %d laminar / %d turbulent points, fewer than %d on a branch" % (name, cen["laminar"], cen["turbulent"], need))
    elif cen["dutau_band"]:
        raise SystemExit("%s: a closing |dutau| lies in [0.5e-6, 2e-6]" % name)
    add, _ = W.wall_flux(arrs)
    L, _ = W.bdy_block(arrs)
    n_fpts = arrs["s0_disu_fpts"].shape[0]
    pts = L[:, W.model_faces(arrs)].ravel()
    f, e = pts % n_fpts, pts // n_fpts
    want = arrs["s0_norm_tconf_fpts"][f, e, :]
    got = arrs["s0_norm_tconf_fpts_inv"][f, e, :] + add[f, e, :]
    err = float(np.abs(got - want).max() / np.abs(want).max())
    if not err <= 1e-13:
        raise SystemExit("%s: the restatement misses the reference's wall flux by %.2e" % (name, err))
    cen["restatement"] = err
    return cen


def capture(c):
    with tempfile.TemporaryDirectory() as td:
        plain, wrapped = moved_vertices(c["n"], c["dims"])
        if c["move"]:
            gen_neu_mesh.box_vertices = wrapped
        try:
            xv = write_neu(os.path.join(td, "mesh.neu"), c["n"], c["dims"], amp=c["amp"], bcs=c.get("bcs"))
        finally:
            gen_neu_mesh.box_vertices = plain
        keys = dict(c["keys"])
        keys["n_steps"] = c["steps"]
        if c["dims"] == 2:
            keys.pop("dz_cyclic")
        with open(os.path.join(td, "input"), "w") as f:
            for k, v in keys.items():
                f.write("%s %s\n" % (k, repr(v) if isinstance(v, float) else v))
        env = dict(os.environ, HIFILES_HOME=REF_HOME)
        r = subprocess.run([HARNESS, "input", "dump.bin", str(c["steps"]), str(c["level"])], cwd=td, env=env, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
            raise SystemExit("ref_harness failed for %s" % c["name"])
        arrs = read_dump(os.path.join(td, "dump.bin"))
    out = {k: v for k, v in arrs.items() if k not in DROP}
    out["xv"] = xv
    meta = dict(name=c["name"], n=c["n"], dims=c["dims"], amp=c["amp"], steps=c["steps"], level=c["level"], keys=c["keys"],
                bcs=c.get("bcs"), orient_seed=None, moved=bool(c["move"]), move_seed=MOVE_SEED, move_fraction=MOVE_FRACTION,
                generator="tools/capture_wall_model.py via oracle/_ref/ref_harness (genuine reference)")
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    if not np.all([np.isfinite(v).all() for k, v in out.items() if v.dtype.kind == "f"]):
        raise SystemExit("%s: the reference's dump is not finite" % c["name"])
    cen = check(c, out)
    os.makedirs(GOLDEN, exist_ok=True)
    path = os.path.join(GOLDEN, c["name"] + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    if size > MAX_BYTES:
        os.remove(path)
        raise SystemExit("%s: %d bytes, more than a committed file may have" % (path, size))
    print("%-26s %7.1f kB  %s" % (c["name"], size / 1e3, cen))


if __name__ == "__main__":
    want = sys.argv[1:]
    for c in CASES:
        if not want or c["name"] in want:
            capture(c)
