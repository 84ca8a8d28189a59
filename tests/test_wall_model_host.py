"""The wall model without a GPU: the restatement (tests/wall_model_util.py) against the genuine reference's fixtures, the host mirror's
input points against the restatement, the conditions the capture tool set, and a stand-alone host program around the library's
wall_stress (csrc/wall_model.hpp) compiled here with the system compiler.

Bars.  Restatement against the reference: inv + fn . tdA equals s0_norm_tconf_fpts within 1e-13 of the block's largest |norm_tconf|
(both sides are the same operations in the same order; what is left is the compiler's).  A wrong Werner-Wengle branch, a wrong input
point and a per-point input each move the wall flux by more than 1e-6 of its own scale, seven orders above the bar.  The host
program against the restatement: 1e-14 relative (one function, two compilers' libm calls).
"""
import ctypes as C
import glob
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_py as O
import wall_model_util as W

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "wall_model")
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "wm_*.npz")))
HEADER_DIR = os.path.join(os.path.dirname(HERE), "hifiles-solver_amd", "csrc")


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def model_points(d):
    L, _ = W.bdy_block(d)
    n_fpts = d["s0_disu_fpts"].shape[0]
    pts = L[:, W.model_faces(d)].ravel()
    return pts % n_fpts, pts // n_fpts


def test_the_fixtures_are_there():
    assert NAMES == ["wm_hex_p2_br", "wm_hex_p2_ww", "wm_hex_p2_ww_sutherland", "wm_hex_p2_ww_wale", "wm_quad_p3_br", "wm_quad_p3_ww"]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(name):
    d = load(name)
    f, e = model_points(d)
    add, _ = W.wall_flux(d)
    want = d["s0_norm_tconf_fpts"][f, e, :]
    got = d["s0_norm_tconf_fpts_inv"][f, e, :] + add[f, e, :]
    scale = np.abs(d["s0_norm_tconf_fpts"]).max()
    err = np.abs(got - want).max() / scale
    print("%s: restatement misses the reference by %.2e of the block's scale" % (name, err))
    assert err <= 1e-13
    # nothing but the model faces carries the model
    others = np.ones(add.shape[:2], dtype=bool)
    others[f, e] = False
    assert not add[others].any()


@pytest.mark.parametrize("name", NAMES)
def test_mutations_of_the_restatement_miss(name):
    """a wrong input point (the last of the ties instead of the first, here: another point of the element), a per-point instead of
    a per-face input, and for model 1 the other branch, all miss by far more than the bar above"""
    d = load(name)
    f, e = model_points(d)
    right, _ = W.wall_flux(d)
    scale = np.abs(right[f, e, :]).max()
    assert scale > 0
    upt, dist, _ = W.input_points(d)
    n_upts = d["u_init"].shape[0]
    wrong = [W.wall_flux(d, upt=(upt + 1) % n_upts, dist=dist)[0], W.wall_flux(d, per_point=True)[0]]
    if W.meta_of(d)["keys"]["wall_model"] == 1:
        _, infos = W.wall_flux(d)
        lam = W.wall_flux(d, branch="laminar")[0]
        tur = W.wall_flux(d, branch="turbulent")[0]
        # each forced branch is wrong exactly at the points of the other one
        wrong += [lam, tur]
    for k, w in enumerate(wrong):
        miss = np.abs(w[f, e, :] - right[f, e, :]).max() / scale
        print("%s: mutation %d misses by %.2e of the wall flux" % (name, k, miss))
        assert miss > 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_census_conditions(name):
    d = load(name)
    c = W.census(d)
    print(name, c)
    assert c["gap"] > 1e-6
    assert np.asarray(d["bc_flags"]).reshape(3, -1, order="F")[2].any()
    if c["model"] == 1:
        assert c["rey_margin"] > 1e-6
        need = 4 if W.meta_of(d)["dims"] == 2 else (c["n_points"] + 3) // 4
        assert min(c["laminar"], c["turbulent"]) >= need
    else:
        assert not c["dutau_band"]
        assert 5 <= c["newton_max"] <= 6


def test_one_fixture_mixes_walls_with_and_without_the_model():
    d = load("wm_hex_p2_ww_wale")
    fl = np.asarray(d["bc_flags"]).reshape(3, -1, order="F")
    _, ids = W.bdy_block(d)
    walls = [g for g in set(int(i) for i in ids) if fl[0, g] in (W.ISOTHERM_WALL, W.ADIABAT_WALL)]
    assert sorted(int(fl[2, g]) for g in walls) == [0, 1]


@pytest.mark.parametrize("name", NAMES)
def test_mirror_finds_the_same_input_points(name):
    import bdy_util
    d = load(name)
    kk = W.meta_of(d)["keys"]
    over = dict(mu_gas=kk["mu_gas"], wall_model=kk["wall_model"])
    if kk.get("LES"):
        over.update(LES=1, SGS_model=kk["SGS_model"], C_s=kk["C_s"], filter_ratio=kk["filter_ratio"])
    c, _ = bdy_util.case_from_fixture(d, **over)
    try:
        wm, upt, dist, n_wm = c.wall_model_points()
        L, ids = c.bdy_faces()
        fl, _, _, _ = c.bc_list()
        assert wm == kk["wall_model"]
        assert np.array_equal(L, W.bdy_block(d)[0]) and np.array_equal(ids, W.bdy_block(d)[1])
        assert np.array_equal(fl[2], np.asarray(d["bc_flags"]).reshape(3, -1, order="F")[2])
        want_upt, want_dist, _ = W.input_points(d)
        assert n_wm == len(W.model_faces(d))
        assert np.array_equal(upt, want_upt)
        assert np.abs(dist - want_dist).max() <= 1e-13
    finally:
        c.close()


def test_mirror_reads_use_wm_only_with_a_wall_model():
    import bdy_util
    d = load("wm_quad_p3_ww")
    c, _ = bdy_util.case_from_fixture(d, mu_gas=1e-4)  # wall_model 0
    try:
        fl, _, _, _ = c.bc_list()
        assert not fl[2].any()
        assert c.wall_model_points()[3] == 0
    finally:
        c.close()
    import hfx
    with pytest.raises(hfx.HfxError, match="Wall model not implemented!"):
        bdy_util.case_from_fixture(d, mu_gas=1e-4, wall_model=3)


@pytest.mark.parametrize("name", NAMES)
def test_final_state_differs_from_a_run_without_the_model(oracle, name):
    """the oracle (no wall model) on the fixture's inputs with use_wm cleared: its final state is far from the fixture's, so no
    path can pass the parity tests by ignoring the model"""
    d = load(name)
    d["bc_flags"] = np.array(d["bc_flags"]).copy()
    d["bc_flags"][2] = 0
    c = O.Case(d)
    e = c.c_eles()
    f, nfb = c.c_faces()
    bd, nbd = c.c_bdy()
    nstage = int(d["sizes"][7])
    steps = sorted({int(k.split("_")[1][4:]) for k in d if k.startswith("u_step")})
    for st in steps:
        for rk in range(nstage):
            assert oracle.orc_CalcResidual_bdy(C.byref(e), f, nfb, bd, nbd, C.byref(c.params)) == -1
            oracle.orc_AdvanceSolution(C.byref(e), C.byref(c.params), rk)
    want = d["u_step%d_stage%d" % (steps[-1], nstage - 1)]
    diff = max(np.abs(c.arr["u0"][..., k] - want[..., k]).max() / np.abs(want[..., k]).max() for k in range(want.shape[-1]))
    print("%s: without the model the final state differs by %.2e" % (name, diff))
    assert diff > 1e-6


# ---- the stand-alone host program ------------------------------------------------------------------------------------------
PHYS = dict(gamma=1.4, prandtl=0.72, prandtl_t=0.9, Kappa=0.41, rt_inf=1.0, mu_inf=1e-3, c_sth=0.4, fix_vis=1.0)


def case_line(model, P, u_wm, u_w, dist, n):
    v = [len(n), model, P["gamma"], P["prandtl"], P["rt_inf"], P["mu_inf"], P["c_sth"], P["fix_vis"], P["prandtl_t"], P["Kappa"], dist]
    v += list(u_wm) + list(u_w) + list(n)
    return " ".join(float(x).hex() if isinstance(x, float) else str(x) for x in v)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("wm") / "wall_model_host_main")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-I", HEADER_DIR, os.path.join(HERE, "wall_model_host_main.cpp"), "-o", exe],
                   check=True)

    def run(cases, tmp):
        path = os.path.join(os.path.dirname(exe), tmp)
        with open(path, "w") as f:
            f.write("\n".join(case_line(*c) for c in cases) + "\n")
        out = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.split("\n")
        rows = [r.split() for r in out if r.strip()]
        assert len(rows) == len(cases)
        return [([float.fromhex(x) if "nan" not in x and "inf" not in x else float(x) for x in r[:-1]], int(r[-1])) for r in rows]
    return run


def test_program_equals_the_restatement_on_every_fixture_point(program):
    cases, want = [], []
    for name in NAMES:
        _, infos = W.wall_flux(load(name))
        for q in infos:
            cases.append(q["inputs"])
            want.append((q["fn"], len(q.get("dutau", []))))
    got = program(cases, "fixtures.txt")
    worst = 0.0
    for (fn, it), (wfn, wit) in zip(got, want):
        assert it == wit
        scale = max(abs(x) for x in wfn)
        worst = max(worst, max(abs(a - b) for a, b in zip(fn, wfn)) / scale)
    print("host program against the restatement over %d points: %.2e relative" % (len(cases), worst))
    assert worst <= 1e-14
    assert max(it for _, it in got) == 6  # what the fixtures need of the Newton loop


def test_program_zero_relative_speed_is_nan(program):
    u_w = [1.0, 0.0, 0.0, 0.0, 2.5]
    u_wm = [1.0, 0.0, 0.0, 0.2, 2.6]  # velocity along the normal only: no wall-parallel speed
    for (fn, _), model in zip(program([(m, PHYS, u_wm, u_w, 0.1, [0.0, 0.0, 1.0]) for m in (1, 2)], "zero.txt"), (1, 2)):
        assert fn[0] == 0.0
        assert all(math.isnan(x) for x in fn[1:4]), (model, fn)
        assert all(math.isnan(x) for x in W.wall_stress(model, PHYS, u_wm, u_w, 0.1, [0.0, 0.0, 1.0])[0][1:4])


def test_program_negative_iterate_is_nan(program):
    """rho_w dist / mu_w = exp(-3.3): the first Newton step from utau = 1 divides by (ln + 1)/Kappa + C = -0.41 and lands at a
    negative utau, whose logarithm is NaN; the loop leaves by itself, as the reference's does"""
    u_w, u_wm = [1.0, 0.0, 0.0, 0.0, 2.5], [1.0, 0.3, 0.0, 0.0, 2.6]
    dist = math.exp(-3.3) * PHYS["mu_inf"]
    (fn, it), = program([(2, PHYS, u_wm, u_w, dist, [0.0, 0.0, 1.0])], "negative.txt")
    assert it == 2 and math.isnan(fn[1]) and math.isnan(fn[4])
    _, info = W.wall_stress(2, PHYS, u_wm, u_w, dist, [0.0, 0.0, 1.0])
    assert len(info["dutau"]) == 2 and math.isnan(info["dutau"][-1])


def test_program_newton_loop_is_capped(program):
    """at utau of order 1e12 neighbouring doubles lie 1e-4 apart: unless an update is exactly zero, |dutau| never falls to 1e-6
    and the reference's loop would not end.  Here it ends at the cap with NaN"""
    cases = []
    for speed in (7e13, 6e13, 5e13, 9e13, 1.1e14, 4e13):
        e_w = 1e30
        cases.append((2, PHYS, [1.0, speed, 0.0, 0.0, e_w + 0.5 * speed ** 2], [1.0, 0.0, 0.0, 0.0, e_w], 0.1, [0.0, 0.0, 1.0]))
    got = program(cases, "cap.txt")
    assert all(it <= W.NEWTON_CAP for _, it in got)
    capped = [(fn, it) for fn, it in got if it == W.NEWTON_CAP]
    assert capped, [it for _, it in got]
    for fn, _ in capped:
        assert math.isnan(fn[1])
    for (fn, it), c in zip(got, cases):
        if it < W.NEWTON_CAP:  # it converged: an update was exactly zero or below 1e-6
            assert math.isfinite(fn[1])
