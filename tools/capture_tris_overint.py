#!/usr/bin/env python3
"""Capture the fixtures of over-integration on triangles (tests/golden/tris_overint/to_*.npz) -- TEST INFRASTRUCTURE, container only.

The genuine reference's harness (oracle/_ref/ref_harness) runs triangle cases with over_int 1 (eles_tris::set_over_int,
src/eles_tris.cpp:674-700; eles::evaluate_invFlux_over_int, src/eles.cpp:1480-1545) and dumps opp_over_int_cubpts, over_int_filter and
JGinv_over_int_cubpts.  Per case it runs at level 1 on the mesh and keys of a fixture of tests/golden/tris with over_int 1 and the
case's over_int_order (tri_util's level-2 restatement of s0_tdisf_upts_inv is the plain evaluate_invFlux and misses an over-integrated
run), two steps each (to_p3_bdy one).  A file is a DELTA file: the three over-integration arrays, over_int, the states after every step,
s0_div_tconf_upts, dt_step*, meta_json, based_on -- and, for a case that changes keys of its base (`rekey`: the inviscid vortex of
tri_p2_inviscid on tri_p1_n4_deformed's mesh), the arrays those keys change.  The tool asserts that every array it does not store
equals the base fixture's bit for bit, and that a case without `rekey` stores nothing else (tests/tri_overint_util.py loads a file
on top of its base).

A file is written only if (tests/tri_overint_util.py: conditions)
  1. the oracle in lockstep meets every dumped state at tri_util's bars;
  2. the run with the over-integration arrays removed differs from the fixture's final state by more than MOVED = 1e-7 of max |u| (10^4
     times the GPU bar: a stage that silently skips de-aliasing cannot pass);
  3. the curved case (the shipped cylinder mesh): JGinv_over_int_cubpts varies over the cubature points of an element.
tri_p3_bdy with over_int_order 6 moves the state by 7.7e-8 only: it is captured with over_int_order 2.  n_cubpts = n_upts (P3 with
over_int_order 3) moves the state by 3e-16 and is left out.

Nothing under oracle/ or tests/golden/tris is written: everything runs in a temporary directory, and no bytecode cache is left.

    python tools/capture_tris_overint.py            # all
    python tools/capture_tris_overint.py to_p3
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
from capture_tris import CYLINDER_MESH, DROP, HARNESS, MAX_BYTES, REF_HOME, box_vertices, read_dump  # noqa: E402
import tri_util as T  # noqa: E402
import tri_overint_util as TO  # noqa: E402

N_STEPS = 2
# keys of the inviscid isentropic vortex (tri_p2_inviscid); the Taylor-Green state moves a P1 run by 1.4e-8 only
VORTEX = ("viscous", "ic_form", "dt", "rho_c_ic", "u_c_ic", "v_c_ic", "w_c_ic", "p_c_ic")
CASES = [
    dict(name="to_p1_o3", base="tri_p1_n4_deformed", over_int_order=3, rekey="tri_p2_inviscid"),  # 10 points: 3 + 3 + 3 + 1
    dict(name="to_p1_o2", base="tri_p1_n4_deformed", over_int_order=2, rekey="tri_p2_inviscid"),  # 6 = 2 x 3: NU divides n_cubpts
    dict(name="to_p2", base="tri_p2_inviscid", over_int_order=5),                                 # 21: 6 + 6 + 6 + 3
    dict(name="to_p3", base="tri_p3_n4_deformed", over_int_order=6),                              # 28: 10 + 10 + 8
    dict(name="to_p3_o2", base="tri_p3_n4_deformed", over_int_order=2),                           # 6: one partial chunk, n_cubpts < NU
    dict(name="to_p3_bdy", base="tri_p3_bdy", over_int_order=2, steps=1),                         # walls, far field, in- and outflow (one step, as
    # its base: the inlet ramps, and the lockstep does not advance the ramp counter from step to step)
    dict(name="to_p4", base="tri_p4_n2_deformed", over_int_order=6),                              # 28: 15 + 13
    dict(name="to_p5", base="tri_p5_n2_deformed", over_int_order=7),                              # 36: 21 + 15
    dict(name="to_p3_cylinder", base="tri_p3_cylinder", over_int_order=4, curved=True),           # 15: 10 + 5; 714 curved elements
]


def identical(a, b):
    """bit for bit; the scalars an inviscid run leaves unset (R_ref, uvw_ref) are NaN in both"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def capture(c):
    STEPS = c.get("steps", N_STEPS)
    base = T.load(c["base"])
    meta0 = json.loads(bytes(base["meta_json"]).decode())
    keys = dict(meta0["keys"])
    if c.get("rekey"):
        other = json.loads(bytes(T.load(c["rekey"])["meta_json"]).decode())["keys"]
        keys.update({k: other[k] for k in VORTEX})
    keys.update(n_steps=STEPS, over_int=1, over_int_order=c["over_int_order"])
    with tempfile.TemporaryDirectory() as td:
        if meta0.get("n") is None:
            shutil.copyfile(CYLINDER_MESH, os.path.join(td, "mesh.neu"))
        else:
            n = [meta0["n"], meta0["n"]] if isinstance(meta0["n"], int) else meta0["n"]
            T.write_neu_tris(os.path.join(td, "mesh.neu"), n, box_vertices(n, 2, amp=meta0["amp"]), bcs=meta0.get("bcs"),
                             orient_seed=meta0.get("orient_seed"))
        with open(os.path.join(td, "input"), "w") as f:
            for k, v in keys.items():
                f.write("%s %s\n" % (k, repr(v) if isinstance(v, float) else v))
        r = subprocess.run([HARNESS, "input", "dump.bin", str(STEPS), "1"], cwd=td, env=dict(os.environ, HIFILES_HOME=REF_HOME),
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-3000:] + r.stderr[-3000:])
            raise SystemExit("ref_harness failed for %s" % c["name"])
        arrs = read_dump(os.path.join(td, "dump.bin"))
    if int(np.ravel(arrs["adv_type"])[0]) < 3:  # (only the low-storage schemes read RK_a / RK_b: else the dump's are whatever the memory held)
        arrs["RK_a"], arrs["RK_b"] = base["RK_a"], base["RK_b"]
    nstage = int(arrs["sizes"][7])
    last = tuple("u_step%d_stage%d" % (s, nstage - 1) for s in range(STEPS))
    full = {k: v for k, v in arrs.items() if k not in DROP and (not k.startswith("u_step") or k in last)}
    bad = [k for k, v in full.items() if v.dtype.kind == "f" and v.size > 1 and not np.isfinite(v).all()]
    if bad:
        raise SystemExit("%s: the reference's dump is not finite: %s" % (c["name"], bad))
    assert int(np.ravel(full["over_int"])[0]) == 1 and full["opp_over_int_cubpts"].shape[0] == TO.n_cubpts(c["over_int_order"])

    # ---- the delta against the base fixture
    out, same = {}, []
    for k, v in full.items():
        if k in TO.OWN or k.startswith(TO.RESULTS):
            out[k] = v
        elif k in base and identical(v, base[k]):
            same.append(k)
        else:
            assert c.get("rekey"), "%s: the harness's %s is not the base fixture's" % (c["name"], k)
            out[k] = v
    gone = [k for k in base if k not in full and not k.startswith(TO.STALE) and k != "xv"]
    assert not gone or c.get("rekey"), "%s: the base fixture's %s are not in the dump" % (c["name"], gone)
    if gone:  # (an inviscid run has no opp_4 / opp_5 / opp_6 ...)
        out["dropped"] = np.frombuffer(json.dumps(sorted(gone)).encode(), dtype=np.uint8)
    out["based_on"] = np.frombuffer(c["base"].encode(), dtype=np.uint8)
    meta = dict(name=c["name"], based_on=c["base"], steps=STEPS, level=1, keys=keys, over_int_order=c["over_int_order"],
                n_cubpts=int(full["opp_over_int_cubpts"].shape[0]), stored=sorted(out),
                generator="tools/capture_tris_overint.py via oracle/_ref/ref_harness (genuine reference)")

    # ---- the conditions, on what a test will load
    os.makedirs(TO.GOLDEN, exist_ok=True)
    path = os.path.join(TO.GOLDEN, c["name"] + ".npz")
    d = TO.overlay(base, out)
    for k, v in full.items():
        assert identical(d[k], v), k
    cond = TO.conditions(d, curved=bool(c.get("curved")))
    if cond["failures"]:
        raise SystemExit("%s: not written: %s" % (c["name"], cond["failures"]))
    meta.update(moved_without_over_int=cond["moved"], metric_variation=cond["metric_variation"], worst_lockstep=cond["worst"])
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    if size > MAX_BYTES:
        os.remove(path)
        raise SystemExit("%s: %d bytes, more than a committed file may have" % (path, size))
    print("%-16s %6.1f kB  %d elements, %d cubature points, lockstep worst %s %.1e, moved %.1e, metric variation %.1e; %d arrays stored, %d the base's"
          % (c["name"], size / 1e3, int(d["sizes"][0]), meta["n_cubpts"], cond["worst"][0], cond["worst"][1], cond["moved"],
             cond["metric_variation"], len(out), len(same)))


if __name__ == "__main__":
    want = sys.argv[1:]
    for c in CASES:
        if not want or c["name"] in want:
            capture(c)
