"""What the host mirror builds for the mass-flux body force (run_input.forcing; csrc/host/eles_forcing.cpp): the surface cubature of
the hexahedra (set_inters_cubpts, set_opp_inters_cubpts, set_transforms_inters_cubpts; src/eles_hexas.cpp:284-373,395,
src/eles.cpp:3635-3665,4480-4595), the reference's inflow rule (src/eles.cpp:5312-5338) and the input keys.  Host only.

The box is 4 x 3 x 3 P2 hexes, x and z periodic, isothermal walls in y: the mirror's periodic matching needs three cells in a
periodic direction that is not split, so z has one cell more than the smallest box one could think of."""
import itertools

import numpy as np
import pytest

import hfx_host as H

N = [4, 3, 3]
L = 2.0
WALLS = dict(bcs=[dict(type="isotherm_wall", T_static=310.0)], sides={"y-": 0, "y+": 0})
CFG = dict(order=2, length=L, T_c_ic=300.0, dt=1e-4, body_forcing=1, **WALLS)
# hexahedra: local face -> (axis it is normal to, direction)
HEX_FACE = [(2, -1), (1, -1), (0, 1), (1, 1), (0, -1), (2, 1)]


@pytest.fixture(scope="module")
def affine():
    c = H.Case(N, amp=0.0, **CFG)
    yield c
    c.close()


@pytest.fixture(scope="module")
def deformed():
    c = H.Case(N, amp=0.05, **CFG)
    yield c
    c.close()


def cub(c, l):
    return {k: c.array("%s_%d" % (k, l)) for k in ("opp_inters_cubpts", "weight_inters_cubpts", "loc_inters_cubpts",
                                                   "tnorm_inters_cubpts", "inter_detjac_inters_cubpts", "norm_inters_cubpts")}


@pytest.mark.parametrize("which", ["affine", "deformed"])
def test_opp_rows_sum_to_one(which, request):
    c = request.getfixturevalue(which)
    for l in range(6):
        a = cub(c, l)
        assert a["opp_inters_cubpts"].shape == ((c.order + 1) ** 2, c.n_upts)
        assert np.abs(a["opp_inters_cubpts"].sum(axis=1) - 1.0).max() < 1e-13
        # the rule itself: (order + 1)^2 Gauss points on the face, weights of the square [-1, 1]^2
        assert abs(a["weight_inters_cubpts"].sum() - 4.0) < 1e-13
        ax, sgn = HEX_FACE[l]
        assert np.all(a["loc_inters_cubpts"][ax] == sgn) and np.all(np.abs(np.delete(a["loc_inters_cubpts"], ax, 0)) < 1.0)
        assert np.all(a["tnorm_inters_cubpts"][ax] == sgn) and not np.delete(a["tnorm_inters_cubpts"], ax, 0).any()


def test_face_areas_of_the_affine_box(affine):
    h = [L / n for n in N]
    for l in range(6):
        a = cub(affine, l)
        ax = HEX_FACE[l][0]
        area = np.prod([h[d] for d in range(3) if d != ax])
        got = a["weight_inters_cubpts"] @ a["inter_detjac_inters_cubpts"]  # (n_eles)
        assert got.shape == (affine.n_eles,)
        assert np.abs(got / area - 1.0).max() < 1e-13


def test_normals(affine, deformed):
    for l in range(6):
        n = cub(deformed, l)["norm_inters_cubpts"]
        assert np.abs(np.sqrt((n ** 2).sum(axis=2)) - 1.0).max() < 1e-13
        n = cub(affine, l)["norm_inters_cubpts"]
        ax, sgn = HEX_FACE[l]
        want = np.zeros(3)
        want[ax] = sgn
        assert np.all(n == want[None, None, :]), l  # exactly
    # the deformation does move the faces: the rule's "== -1" then holds nowhere on the x-min plane
    assert np.abs(cub(deformed, 4)["norm_inters_cubpts"][:, :, 0] + 1.0).min() > 1e-6


def test_inflow_rule(affine, deformed):
    ele, inter = affine.inflow_faces()
    nx, ny, nz = N
    want = sorted(0 + nx * (j + ny * k) for j in range(ny) for k in range(nz))
    assert len(ele) == ny * nz and sorted(ele.tolist()) == want
    assert np.all(inter == 4)
    # on the deformed box the x-min plane is warped: no normal is -x exactly and the reference's rule selects nothing
    ele, inter = deformed.inflow_faces()
    assert len(ele) == 0


def test_rule_off_builds_nothing():
    c = H.Case(N, amp=0.0, **dict(CFG, body_forcing=0))
    with pytest.raises(Exception, match="unknown array"):
        c.array("opp_inters_cubpts_4")
    assert len(c.inflow_faces()[0]) == 0
    c.close()


def folded(c, ele, l):
    a = cub(c, l)
    return (a["weight_inters_cubpts"] * a["inter_detjac_inters_cubpts"][:, ele]) @ a["opp_inters_cubpts"]  # c(k, face)


def test_folded_weights_integrate_monomials(affine):
    """u_k = x^a y^b z^c at the solution points, a, b, c <= P: sum over the inflow faces of c(., face) . u is the integral over the
    plane x = 0 of the interpolant, which is the monomial itself, and the rule is exact for it"""
    ele, inter = affine.inflow_faces()
    pos = affine.array("pos_upts")  # (n_upts, n_eles, 3)
    P = affine.order
    worst = 0.0
    for a, b, c in itertools.product(range(P + 1), repeat=3):
        got = 0.0
        for e, l in zip(ele, inter):
            x, y, z = (pos[:, e, d] for d in range(3))
            got += folded(affine, e, l) @ (x ** a * y ** b * z ** c)
        want = (1.0 if a == 0 else 0.0) * L ** (b + 1) / (b + 1) * L ** (c + 1) / (c + 1)
        scale = L ** (b + 1) / (b + 1) * L ** (c + 1) / (c + 1)
        worst = max(worst, abs(got - want) / scale)
    print("worst monomial error %.3g" % worst)
    assert worst < 1e-12


def test_folded_weights_on_the_deformed_box(deformed):
    """detjac varies from cubature point to cubature point there; the folded weights of a face still add up to its area"""
    for e in (0, 5, deformed.n_eles - 1):
        a = cub(deformed, 4)
        dj = a["inter_detjac_inters_cubpts"][:, e]
        assert dj.max() / dj.min() - 1.0 > 1e-4
        assert abs(folded(deformed, e, 4).sum() / (a["weight_inters_cubpts"] @ dj) - 1.0) < 1e-13


def test_input_keys():
    c = H.Case(3, order=1)
    assert c.forcing() == (0, 9.162, 9.162)  # body_forcing off, the reference's hard-coded area and mass flux
    c.close()
    c = H.Case(N, amp=0.0, **dict(CFG, forcing_area=4.0))
    assert c.forcing() == (1, 4.0, 9.162)
    c.set_forcing(3.0, 2.5)  # (host only: nothing to register yet)
    assert c.forcing() == (1, 3.0, 2.5)
    c.close()
    c = H.Case(3, order=1)
    with pytest.raises(Exception, match="body_forcing"):
        c.set_forcing(1.0, 1.0)
    c.close()
