"""The host side of the wall-force monitor (csrc/host/eles_forces.cpp) and the yardstick of its tests (tests/wall_force_util.py)
against the output of the GENUINE reference: the five fixtures of tools/capture_wall_forces.py hold the force columns of the
driver's history.plt and its cp file beside the state and the gradient its CalcForces read.  No GPU: the mirror builds the wall
faces and the surface cubature, the np.longdouble restatement of eles::compute_wall_forces is applied to the fixture's arrays.

Bars (derived in tests/wall_force_util.py; S is the un-cancelled scale of each number):
    positions, Cp, Cf     1e-12 S + 5e-13 |value|     the second term: the file prints 13 significant digits
    F totals, CL, CD      1e-12 S + 1e-15 |value|     history.plt prints 15
The position of a point is a convex combination of its element's vertices: S is the largest |coordinate| among them.
"""
import functools
import os

import numpy as np
import pytest

import bdy_util
import wall_force_util as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wall_force")
FIXTURES = ("wf_hex_p2_a", "wf_hex_p2_b", "wf_quad_p3_a", "wf_quad_p3_b", "wf_quad_p3_inviscid")
LD = W.LD


def mirror_case(d, **over):
    """the fixture's case through the host mirror, with the force keys of its input file"""
    import json
    kk = json.loads(bytes(d["meta_json"]).decode())["keys"]
    keys = dict(calc_force=1, area_ref=kk["area_ref"], monitor_cp_freq=kk["monitor_cp_freq"],
                loc_1d_upts=d["loc_upts"][0, :kk["order"] + 1])
    if kk["viscous"]:
        keys.update(nx_c_ic=kk["nx_c_ic"], ny_c_ic=kk["ny_c_ic"], nz_c_ic=kk["nz_c_ic"])
    keys.update(over)
    return bdy_util.case_from_fixture(d, **keys)


def device_arrays(case):
    """what mv_all_cpu_gpu registers for the case's wall faces, in the form tests/wall_force_util.py and hfx.Eles.set_wall_faces
    take: dict(face_ele, face_inter, face_flag, opp, weight, detjac, norm)"""
    wp = case.wall_points()
    n_inters = 2 * case.n_dims
    opp = [case.array("opp_inters_cubpts_%d" % l) for l in range(n_inters)]
    weight = [case.array("weight_inters_cubpts_%d" % l) for l in range(n_inters)]
    dj = [case.array("inter_detjac_inters_cubpts_%d" % l) for l in range(n_inters)]
    nm = [case.array("norm_inters_cubpts_%d" % l) for l in range(n_inters)]
    detjac = [dj[l][:, e] for e, l in zip(wp["ele"], wp["inter"])]
    norm = [nm[l][:, e, :] for e, l in zip(wp["ele"], wp["inter"])]
    return dict(face_ele=wp["ele"], face_inter=wp["inter"], face_flag=wp["flag"], opp=opp, weight=weight, detjac=detjac, norm=norm)


def phys_of(case):
    p = case.params()
    return {k: getattr(p, k) for k in ("gamma", "rt_inf", "mu_inf", "c_sth", "fix_vis", "viscous")}


def ref_of(case):
    r = case.calc_force()
    return {k: r[k] for k in ("rho_c_ic", "u_c_ic", "v_c_ic", "w_c_ic", "p_c_ic", "area_ref")}


@functools.lru_cache(maxsize=None)
def setup(name):
    """everything the tests of one fixture share, computed once: the fixture, the mirror's wall faces, the restatement's values
    and scales on the fixture's state and gradient"""
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    case, meta = mirror_case(d)
    A = device_arrays(case)
    phys, ref = phys_of(case), ref_of(case)
    args = (A["face_ele"], A["face_inter"], A["face_flag"], A["opp"], A["weight"], A["detjac"], A["norm"], d["u_step0_stage0"],
            d.get("s0_grad_disu_upts"), phys, ref)
    val, S = W.both(*args)
    out = dict(d=d, meta=meta, A=A, phys=phys, ref=ref, args=args, val=val, S=S, wp=case.wall_points(), shape=case.array("shape"),
               n_dims=case.n_dims)
    case.close()
    return out


def file_order(x, first):
    """per-point values (j ascending inside a face) -> the row order of the cp file (j descending)"""
    return np.concatenate([x[first[f]:first[f + 1]][::-1] for f in range(len(first) - 1)]) if len(first) > 1 else x


@pytest.mark.parametrize("name", FIXTURES)
def test_wall_faces_are_the_cp_files(name):
    """the mirror's face list: as many faces as the file labels, the same labels in the same order, every face with the rows
    the file gives it"""
    s = setup(name)
    d, wp = s["d"], s["wp"]
    assert [W.LABELS[int(f)] for f in wp["flag"]] == [str(x) for x in d["cp_labels"]]
    first = np.concatenate([[0], np.cumsum(wp["n_points"])])
    assert np.array_equal(first[:-1], d["cp_first"]) and first[-1] == len(d["cp_rows"])
    # one cell between two walls: every element has two wall faces, ascending by element, then by local face
    assert np.array_equal(wp["ele"], np.repeat(np.arange(len(wp["ele"]) // 2), 2))
    assert np.all(wp["inter"][0::2] < wp["inter"][1::2])


@pytest.mark.parametrize("name", FIXTURES)
def test_rows_against_the_reference(name):
    """positions, Cp and Cf of every row of the reference's cp file"""
    s = setup(name)
    d, wp, val, S, nd = s["d"], s["wp"], s["val"], s["S"], s["n_dims"]
    rows = d["cp_rows"]
    viscous = bool(s["phys"]["viscous"])
    assert rows.shape[1] == nd + (2 if viscous else 1)
    first = val["first"]
    # positions: S = the largest |coordinate| among the element's vertices
    ele_of_row = np.repeat(wp["ele"], wp["n_points"])
    S_pos = np.abs(s["shape"]).max(axis=1)[:, ele_of_row]  # (n_dims, rows)
    miss = np.abs(wp["pos"] - rows[:, :nd].T)
    bar = 1e-12 * S_pos + 5e-13 * np.abs(rows[:, :nd].T)
    print("%s: positions worst miss / bar = %.2e" % (name, (miss / bar).max()))
    assert np.all(miss <= bar)
    worst = 0.0
    for key, col in (("cp", nd), ("cf", nd + 1)):
        if col >= rows.shape[1]:
            assert not np.any(val[key])  # an inviscid case: no Cf column, and the restatement's is zero
            continue
        got, sc, want = file_order(val[key], first), file_order(S[key], first), rows[:, col].astype(LD)
        miss = np.abs(got - want)
        bar = LD(1e-12) * sc + LD(5e-13) * np.abs(want)
        worst = max(worst, float((miss / sc).max()))
        print("%s: %s worst |restatement - file| / S = %.2e, / bar = %.2e" % (name, key, (miss / sc).max(), (miss / bar).max()))
        assert np.all(miss <= bar), key
    print("%s: rows worst ratio to S %.2e" % (name, worst))


@pytest.mark.parametrize("name", FIXTURES)
def test_totals_against_the_reference(name):
    """F totals (inviscid + viscous), CL and CD of the reference's history line"""
    s = setup(name)
    d, val, S = s["d"], s["val"], s["S"]
    pairs = [(val["inv_force"] + val["vis_force"], S["inv_force"] + S["vis_force"], d["hist_F"].astype(LD), "F"),
             (val["cl"], S["cl"], LD(d["hist_CL"][0]), "CL"), (val["cd"], S["cd"], LD(d["hist_CD"][0]), "CD")]
    for got, sc, want, what in pairs:
        miss = np.abs(np.atleast_1d(got - want))
        bar = LD(1e-12) * np.atleast_1d(sc) + LD(1e-15) * np.abs(np.atleast_1d(want))
        print("%s: %s worst |restatement - history| / S = %.2e" % (name, what, (miss / np.atleast_1d(sc)).max()))
        assert np.all(miss <= bar), what


def moved(s, **switch):
    """the largest change of any result, in units of its scale, when one physics switch of the restatement is moved"""
    other = W.wall_forces(*s["args"], **switch)
    return max(float((np.abs(np.atleast_1d(other[k] - s["val"][k])) / np.atleast_1d(s["S"][k])).max())
               for k in W.KEYS if np.atleast_1d(s["S"][k]).size and np.all(np.atleast_1d(s["S"][k]) > 0))


def test_restatement_feels_every_switch():
    """the dual flag, fix_vis, aos, the / 3.0 and a slip wall's viscous part each move some result by more than 1e-6 of S"""
    a3, b3, a2, b2 = setup("wf_hex_p2_a"), setup("wf_hex_p2_b"), setup("wf_quad_p3_a"), setup("wf_quad_p3_b")
    assert moved(a3, no_dual=True) > 1e-6 and moved(b2, no_dual=True) > 1e-6 and moved(setup("wf_quad_p3_inviscid"), no_dual=True) > 1e-6
    assert moved(a3, no_aos=True) > 1e-6
    assert moved(a2, third=2.0) > 1e-6 and moved(a3, third=2.0) > 1e-6
    assert moved(b3, slip_viscous=False) > 1e-6 and moved(a2, slip_viscous=False) > 1e-6
    for s in (a3, a2):
        args = list(s["args"])
        args[9] = dict(s["phys"], fix_vis=0.0)
        other = W.wall_forces(*args)
        assert float((np.abs(other["cf"] - s["val"]["cf"]) / s["S"]["cf"]).max()) > 1e-6


def test_input_keys():
    """calc_force, area_ref, monitor_cp_freq as src/input.cpp:102-107,536-537,621-622 treat them"""
    import hfx
    d = setup("wf_quad_p3_a")["d"]
    case, _ = mirror_case(d, area_ref=2.5, monitor_cp_freq=0)
    k = case.calc_force()
    assert k["calc_force"] == 1 and k["monitor_cp_freq"] == 2 ** 31 - 1
    assert k["area_ref"] == 2.5  # L_free_stream is 1
    case.close()
    with pytest.raises(hfx.HfxError, match="area_ref"):
        mirror_case(d, area_ref=0.0)
    # without calc_force: no wall faces and no surface cubature
    case, _ = bdy_util.case_from_fixture(d)
    with pytest.raises(hfx.HfxError, match="calc_force"):
        case.wall_points()
    with pytest.raises(hfx.HfxError):
        case.array("opp_inters_cubpts_0")
    case.close()
