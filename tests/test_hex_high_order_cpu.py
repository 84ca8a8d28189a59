"""Hexahedra of orders 6 and 7 (N = 7, 8 points per direction) on the CPU: the host mirror's operators and metrics and the
oracle's step against the genuine reference's fixtures (tools/capture_hex_high_order.py), and that capture tool itself."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hfx_host as H
import oracle_py as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ["hex_p6_deformed", "hex_p7_deformed"]


def rel(a, b):
    s = np.abs(b).max()
    return np.abs(a - b).max() / (s if s > 0 else 1.0)


def load(name, n=None):
    """the fixture and a host-mirror case of its settings: on the fixture's own mesh, or on an n^3 box of the same generator
    (the mirror's periodic box matching needs three cells per direction; the fixtures have two)"""
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    meta = json.loads(bytes(d["meta_json"]).decode())
    k = meta["keys"]
    kw = dict(order=k["order"], adv_type=k["adv_type"], riemann_solve_type=k["riemann_solve_type"], upts_type=k["upts_type_hexa"],
              vcjh_scheme=k["vcjh_scheme_hexa"], fix_vis=k["fix_vis"], T_c_ic=k["T_c_ic"])
    c = H.Case(meta["n"], xv=d["xv"], **kw) if n is None else H.Case(n, amp=meta["amp"], **kw)
    return c, d, k


@pytest.mark.parametrize("name", NAMES)
def test_host_mirror_operators(name):
    """the 1-D point sets and the VCJH correction of the host mirror at N = 7 and 8: the element operators (which do not
    depend on the mesh) and the reference-element point tables against the reference's"""
    c, d, k = load(name, n=3)
    assert c.sizes[1:4] == [int(v) for v in d["sizes"][1:4]]
    assert c.sizes[1] == (k["order"] + 1) ** 3
    for op in ["opp_0", "opp_3", "opp_6"] + ["opp_%d_%d" % (w, i) for w in (1, 2, 4, 5) for i in range(3)]:
        got, want = c.array(op), d[op]
        assert rel(got, want) < 5e-13, op
        # the tensor-product sparsity the fused tables are built from: the reference's structural zeros are exact here
        assert np.all(got[want == 0.0] == 0.0), op
        assert np.all(np.abs(want[got == 0.0]) < 1e-14), op
    for a in ("loc_upts", "tloc_fpts", "tnorm_fpts"):
        assert rel(c.array(a), d[a]) < 1e-15, a
    c.close()


@pytest.mark.parametrize("name", NAMES)
def test_oracle_step(name):
    """one RK step of the oracle on the fixture's arrays (operators, metrics, faces) against the reference"""
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    oc = O.Case(d)
    e, (f, nb) = oc.c_eles(), oc.c_faces()
    assert O.load().orc_rk_step(C.byref(e), f, nb, C.byref(oc.params)) == -1
    assert rel(oc.arr["u0"], d["u_step0_stage%d" % (int(d["sizes"][7]) - 1)]) < 1e-11


@pytest.mark.parametrize("order", [6, 7])
def test_host_mirror_setup_drives_the_oracle(order):
    """the host mirror's whole setup of a deformed P6 / P7 box (operators, metrics from the mesh, faces) through the oracle:
    a finite step that moves the state"""
    c = H.Case(3, order=order, amp=0.15)
    oc = O.Case(c.registration())
    u0 = oc.arr["u0"].copy()
    e, (f, nb) = oc.c_eles(), oc.c_faces()
    assert O.load().orc_rk_step(C.byref(e), f, nb, C.byref(oc.params)) == -1
    u = oc.arr["u0"]
    assert np.isfinite(u).all() and rel(u, u0) > 1e-8
    c.close()


CHECK = r"""
import os, sys, numpy as np
root, tmp = sys.argv[1], sys.argv[2]
oracle = os.path.realpath(os.path.join(root, "oracle")) + os.sep
writes = []
def hook(event, args):
    if event == "open" and len(args) > 1 and isinstance(args[0], (str, bytes)) and (
            (isinstance(args[1], str) and any(m in args[1] for m in "wax+")) or (isinstance(args[2], int) and args[2] & 3)):
        writes.append(os.path.realpath(args[0]))
    if event in ("os.mkdir", "os.rename", "os.remove", "shutil.copyfile"):
        writes.append(os.path.realpath(str(args[0])))
sys.addaudithook(hook)
sys.argv = [sys.argv[0]]
import importlib.util
spec = importlib.util.spec_from_file_location("capture_hex_high_order", os.path.join(root, "tools", "capture_hex_high_order.py"))
m = importlib.util.module_from_spec(spec)
spec.loader.exec_module(m)
def fake_run_case(c):  # (the reference is not run here: what the tool itself writes is what is checked)
    np.savez_compressed(os.path.join(tmp, c["name"] + ".npz"), u_init=np.zeros(3), u_step0_stage0=np.zeros(3),
                        u_step0_stage4=np.ones(3))
m.run_case = fake_run_case
m.GOLDEN = tmp
for c, drop in m.CASES:
    m.capture(c, drop)
bad = [w for w in writes if w.startswith(oracle)]
assert not bad, bad
assert all(w.startswith(os.path.realpath(tmp)) for w in writes if w.endswith(".npz")), writes
assert sorted(os.listdir(tmp)) == ["hex_p6_deformed.npz", "hex_p7_deformed.npz"]
print("ok")
"""


def test_capture_tool_never_writes_under_oracle(tmp_path):
    """tools/capture_hex_high_order.py reuses oracle/capture_golden.py's case and run_case and leaves oracle/ alone: no write
    under it (an audit hook records every file the tool opens for writing), no bytecode cache, no changed file"""
    oracle = os.path.join(ROOT, "oracle")

    def listing():
        return {os.path.join(r, f): os.stat(os.path.join(r, f)).st_mtime_ns
                for r, _, fs in os.walk(oracle) if "_ref" not in r.split(os.sep) for f in fs}

    before = listing()
    r = subprocess.run([sys.executable, "-c", CHECK, ROOT, str(tmp_path)], capture_output=True, text=True,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE=""))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert listing() == before
