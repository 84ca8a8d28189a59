"""The host mirror's side of the exact-solution error norms and the integral diagnostics (csrc/host/eles_error.cpp,
hfxh_case_set_test_case, hfxh_case_set_integral_quantities): the volume cubature against the genuine reference's fixtures, the
positions against calc_pos, the refusals, the walls of Couette flow.  CPU only: nothing here touches the GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import hfx
import hfx_host as H
from test_host_setup_vs_golden import GOLDEN, case_from_fixture, rel

FIVE = ("loc_volume_cubpts", "weight_volume_cubpts", "opp_volume_cubpts", "vol_detjac_vol_cubpts", "pos_volume_cubpts")


def missing(c, name):
    with pytest.raises(hfx.HfxError, match="unknown array"):
        c.array(name)
    return True


@pytest.mark.parametrize("name", ["hex_p2_integrals", "quad_p3_integrals"])
@pytest.mark.parametrize("by", ["integral_quantities", "test_case"])
def test_volume_cubature_vs_reference(name, by):
    """weight, operator and determinant as the genuine reference built them, at the bars tests/test_host_setup_vs_golden.py
    holds opp_0 (5e-14) and detjac_upts (1e-14) to; either setter builds them; the positions only for a test case, and then
    bit-equal to calc_pos at loc_volume_cubpts"""
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    c, meta = case_from_fixture(d)
    assert all(missing(c, k) for k in FIVE)  # neither setter active: none of the five
    if by == "test_case":
        c.set_test_case(1)
    else:
        c.set_integral_quantities(["kineticenergy", "Enstropy"])
    n_cub = (c.order + 1) ** c.n_dims
    assert c.array("loc_volume_cubpts").shape == (c.n_dims, n_cub)
    for k, bar in (("weight_volume_cubpts", 5e-14), ("opp_volume_cubpts", 5e-14), ("vol_detjac_vol_cubpts", 1e-14)):
        got, want = c.array(k), d[k]
        assert got.shape == want.shape, k
        assert rel(got, want) < bar, (k, rel(got, want))
    if by == "test_case":
        pos = c.array("pos_volume_cubpts")
        assert pos.shape == (n_cub, c.n_eles, c.n_dims)
        loc = c.array("loc_volume_cubpts")
        ele = np.repeat(np.arange(c.n_eles), n_cub)
        want = c.calc_pos(ele, np.tile(loc, (1, c.n_eles)))  # (n_dims, n) for n (element, location) pairs
        assert np.array_equal(pos.transpose(2, 0, 1).reshape(c.n_dims, -1, order="F"), want)
        c.set_test_case(0)
    else:
        assert missing(c, "pos_volume_cubpts")
        c.set_integral_quantities([])
    assert all(missing(c, k) for k in FIVE)  # switched off again: dropped
    c.close()


def test_gauss_rule_is_first_direction_fastest():
    """the tensor Gauss rule with order + 1 points per direction: loc(0) runs fastest, the weights are the products"""
    c = H.Case([3, 3, 1], dims=2, order=2, amp=0.05)
    c.set_test_case(1)
    x, w = np.polynomial.legendre.leggauss(3)
    loc, wt = c.array("loc_volume_cubpts"), c.array("weight_volume_cubpts")
    assert np.abs(loc[0] - np.tile(x, 3)).max() < 1e-15 and np.abs(loc[1] - np.repeat(x, 3)).max() < 1e-15
    assert np.abs(wt - np.outer(w, w).ravel()).max() < 1e-15
    c.close()


def test_refusals_leave_the_case_usable():
    c = H.Case([3, 3, 1], dims=2, order=2, amp=0.05)
    with pytest.raises(hfx.HfxError, match="integral diagnostic quantity not recognized"):
        c.set_integral_quantities(["kineticenergy", "enstrophy"])  # (the reference spells it enstropy)
    for tc in (2, 3, 4):
        with pytest.raises(hfx.HfxError, match="advection-diffusion"):
            c.set_test_case(tc)
    for tc in (-1, 6, 9):
        with pytest.raises(hfx.HfxError, match="Test case not recognized in compute error, exiting"):
            c.set_test_case(tc)
    for norm in (0, 3):
        with pytest.raises(hfx.HfxError, match="Error norm not supported!"):
            c.set_test_case(1, norm)
    with pytest.raises(hfx.HfxError, match="no moving isothermal wall"):
        c.set_test_case(5)  # (a periodic box has no walls at all)
    assert c.test_case() == dict(test_case=0, error_norm_type=2, u_wall=0.0, T_wall=0.0)  # the reference's defaults, untouched
    assert all(missing(c, k) for k in FIVE)
    c.set_test_case(1, 1)
    assert c.test_case()["test_case"] == 1 and c.test_case()["error_norm_type"] == 1
    assert c.array("opp_volume_cubpts").shape == (9, 9)
    with pytest.raises(hfx.HfxError, match="Test case not recognized"):
        c.set_test_case(7)
    assert c.test_case()["test_case"] == 1 and c.array("pos_volume_cubpts").shape == (9, 9, 2)
    # not on the device: the monitors say so
    out = np.zeros((2, 4), order="F")
    assert H.lib().hfxh_case_compute_error(c.h, out.ctypes.data_as(hfx.dp)) != 0
    assert b"not on the device" in H.lib().hfxh_last_error()
    c.close()


def channel(bcs):
    """a 2-D channel: periodic in x, boundary groups 0 and 1 on the lower and the upper side"""
    return H.Case([3, 3, 1], dims=2, order=2, length=1.0, bcs=bcs, sides={"y-": 0, "y+": 1})


def test_couette_walls_from_the_boundary_groups():
    """u_wall is velocity(0) of the isothermal wall that moves, T_wall is T_static of the one at rest (src/eles.cpp:5219-5230),
    both as the non-dimensional bc_list holds them"""
    c = channel([dict(type="isotherm_wall", T_static=300.0), dict(type="isotherm_wall", u=12.5, T_static=315.0)])
    c.set_test_case(5)
    fl, par, R_ref, rc = c.bc_list()
    t = c.test_case()
    assert t["test_case"] == 5
    assert t["u_wall"] == par[1, 1] and t["u_wall"] != 0.0 and t["T_wall"] == par[5, 0]
    ref = c.ref_values()
    assert abs(t["u_wall"] - 12.5 / ref["uvw_ref"]) <= 1e-14 * t["u_wall"]
    assert abs(t["T_wall"] - 300.0 / H.TGV["T_free_stream"]) <= 1e-14 * t["T_wall"]
    assert c.array("pos_volume_cubpts").shape == (9, 9, 2)
    c.close()


def test_couette_refused_when_a_wall_is_missing():
    """the reference reads u_wall or T_wall uninitialised then; the mirror names the missing wall and stays as it was"""
    c = channel([dict(type="isotherm_wall", T_static=300.0), dict(type="isotherm_wall", T_static=315.0)])
    with pytest.raises(hfx.HfxError, match="no moving isothermal wall"):
        c.set_test_case(5)
    assert c.test_case()["test_case"] == 0
    c.set_test_case(1)  # (still usable)
    c.close()
    c = channel([dict(type="adiabat_wall"), dict(type="isotherm_wall", u=12.5, T_static=315.0)])
    with pytest.raises(hfx.HfxError, match="no isothermal wall at rest"):
        c.set_test_case(5)
    assert c.test_case()["test_case"] == 0 and all(missing(c, k) for k in FIVE)
    c.close()


def test_new_declarations_are_exported():
    dev = ("hfx_ctx_set_exact_solution", "hfx_eles_set_error_points", "hfx_eles_compute_error", "hfx_eles_error_launch")
    host = ("hfxh_case_set_test_case", "hfxh_case_get_test_case", "hfxh_case_set_integral_quantities", "hfxh_case_compute_error",
            "hfxh_case_CalcIntegralQuantities")
    declared = hfx.declared_symbols()
    for n in dev:
        assert n in declared and hasattr(hfx.lib(), n), n
    txt = open(os.path.join(hfx.ROOT, "include", "hfx_host.h")).read()
    for n in host:
        assert n + "(" in txt and hasattr(H.lib(), n), n
    assert C.sizeof(hfx.Exact) == 48  # two ints and five doubles, as hfx_exact
