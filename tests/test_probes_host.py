"""Point probes on the host mirror (csrc/host/eles_probes.cpp): the operator row eles::set_opp_probe, locating a point
(calc_p2c of the four element classes, eles::pos_to_loc), and the numpy statement of the probe fields that the device tests
(tests/test_gpu_probes.py) compare against.  No GPU.

The yardstick is the genuine reference's plot-point data of the four *_plot fixtures: a row of opp_p is eval_nodal_basis at a
plot point (src/eles.cpp:3600-3621), which is what set_opp_probe computes for a probe there (src/eles.cpp:3625-3631)."""
import numpy as np
import pytest

import hfx
import probe_util as U

OPP_P_BAR = 5e-14  # what tests/test_host_setup_vs_golden.py grants the mirror's opp_p on these fixtures


def rel(a, b):
    s = np.abs(b).max()
    return np.abs(a - b).max() / (s if s > 0 else 1.0)


@pytest.fixture(scope="module", params=U.PLOT_FIXTURES)
def cls(request):
    m, shape, ele_type = U.mirror(request.param)
    yield request.param, U.load(request.param), m, shape, ele_type
    m.close()


# ---- 1. opp_probe against the reference ------------------------------------------------------------------------------------
def test_opp_probe_at_the_plot_points_vs_reference(cls):
    name, d, m, shape, ele_type = cls
    got = m.opp_probe(d["loc_ppts"])  # (n_upts, n_ppts): column j is the row of plot point j
    err = rel(got.T, d["opp_p"])
    print("%s: opp_probe against the reference's opp_p %.3e" % (name, err))
    assert got.T.shape == d["opp_p"].shape
    assert err < OPP_P_BAR


# ---- 2. locating ------------------------------------------------------------------------------------------------------------
def interior_plot_points(d, ele_type):
    return [j for j in range(d["loc_ppts"].shape[1]) if np.all(np.abs(d["loc_ppts"][:, j]) < 1 - 1e-12)] if ele_type in (1, 4) else []


def test_locating_returns_the_element_and_the_location(cls):
    """strictly interior plot points of the tensor-product fixtures (eight per hexahedron at p_res 4, one per quad at p_res 3)
    and 200 seeded random points with |loc_i| <= 0.6 in every class: mapped to physical space with the mirror's calc_pos, located
    again.  pos_to_loc stops after a step of at most 1e-6, which leaves a quadratically small error: 1e-10.  Against a numpy
    restatement of the same iteration: 1e-13."""
    name, d, m, shape, ele_type = cls
    n_eles = shape.shape[2]
    interior = interior_plot_points(d, ele_type)
    assert len(interior) == {"hex_p3_plot": 8, "quad_p2_plot": 1}.get(name, 0)
    locs = [d["loc_ppts"][:, j] for j in interior for _ in range(n_eles)]
    eles = [e for _ in interior for e in range(n_eles)]
    rnd = U.random_interior_locs(ele_type, 200, seed=20 + ele_type)
    rng = np.random.default_rng(7)
    locs += [rnd[:, i] for i in range(200)]
    eles += [int(e) for e in rng.integers(0, n_eles, 200)]
    assert n_eles - 1 in eles and 0 in eles
    locs = np.array(locs).T.copy(order="F")
    pos = m.calc_pos(eles, locs)
    p2c, got = m.locate(pos)
    assert np.array_equal(p2c, np.array(eles))
    err = np.abs(got - locs).max()
    want = np.array([U.newton(ele_type, shape[:, :, e], pos[:, i]) for i, e in enumerate(eles)]).T
    err_np = np.abs(got - want).max()
    print("%s: %d points, |loc - loc_true| %.3e, mirror against the numpy iteration %.3e" % (name, len(eles), err, err_np))
    assert err <= 1e-10
    assert err_np <= 1e-13


def test_numpy_calc_pos_is_the_mirrors(cls):
    """the restated shape functions the numpy iteration runs on are the mirror's"""
    name, d, m, shape, ele_type = cls
    locs = U.random_interior_locs(ele_type, 10, seed=3)
    eles = [i % shape.shape[2] for i in range(10)]
    want = np.array([shape[:, :, e] @ U.shape_basis(ele_type, locs[:, i])[0] for i, e in enumerate(eles)]).T
    assert np.abs(m.calc_pos(eles, locs) - want).max() < 1e-14 * np.abs(want).max()


def test_a_point_outside_the_mesh_is_nobodys(cls):
    name, d, m, shape, ele_type = cls
    far = shape.max() + 10.0
    inside = m.calc_pos([0], np.zeros((shape.shape[0], 1)) + (-0.5 if ele_type in (2, 3) else 0.0))
    p2c, loc = m.locate(np.column_stack([np.full(shape.shape[0], far), inside[:, 0]]))
    assert list(p2c) == [-1, 0]


def test_case_registers_only_the_points_it_holds():
    """hfxh_case_set_probes on the host: p2c, p2t, loc_probe and the global index of each located probe; the point outside is
    left out; refusals leave the case as it was"""
    m, shape, ele_type = U.mirror("hex_p3_plot")
    n_eles = shape.shape[2]
    locs = U.random_interior_locs(4, 5, seed=11)
    eles = [n_eles - 1, 0, 3, 3, 7]
    pos = m.calc_pos(eles, locs)
    pos = np.insert(pos, 2, shape.max() + 10.0, axis=1)  # the third point lies outside
    m.set_probes(pos, ["RHO", "Pressure"], probe_freq=2, capacity=4)
    p = m.probes()
    assert list(p["p2c"]) == eles and list(p["global_index"]) == [0, 1, 3, 4, 5] and set(p["p2t"]) == {4}
    assert np.abs(p["loc_probe"] - locs).max() <= 1e-10
    with pytest.raises(hfx.HfxError, match="not implemented"):
        m.set_probes(pos, ["rho", "mach"])
    with pytest.raises(hfx.HfxError, match="probe_freq"):
        m.set_probes(pos, ["rho"], probe_freq=0)
    assert list(m.probes()["p2c"]) == eles
    m.set_probes(pos, [])
    assert len(m.probes()["p2c"]) == 0
    m.close()
    q, _, _ = U.mirror("quad_p2_plot")
    with pytest.raises(hfx.HfxError, match="z velocity"):
        q.set_probes(np.zeros((2, 1)), ["u", "w"])
    q.close()


def test_newton_that_does_not_converge_is_an_error():
    """a position that is not a finite point never brings the Newton step below 1e-6: the mirror's iteration is capped and
    reports it, where the reference's loop either never ends or leaves a NaN location behind; the case stays usable"""
    m, shape, ele_type = U.mirror("quad_p2_plot")
    for bad in ([np.inf, 0.0], [np.nan, 0.0]):
        with pytest.raises(hfx.HfxError, match="did not converge"):
            m.pos_to_loc(0, bad)
    inside = m.calc_pos([0], np.zeros((2, 1)))
    assert np.abs(m.pos_to_loc(0, inside[:, 0])).max() <= 1e-10
    m.close()


# ---- 3. summation order ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.PLOT_FIXTURES)
def test_fields_do_not_depend_on_the_summation_order(name):
    """The expected values of the device tests are the six field formulas on the fixture's genuine disu_ppts.  The device sums
    the contraction in another order than the reference (64 lane partials, then a butterfly): evaluated in REVERSED order the
    fields move by less than 1e-13 of each field's largest magnitude, so the device's 1e-12 is neither loose nor out of reach --
    and the ascending contraction of u_init reproduces the reference's disu_ppts to the same measure."""
    d = U.load(name)
    n_ppts, n_eles, n_fields = d["disu_ppts"].shape
    names = U.field_names(n_fields - 2)
    gamma = 1.4
    ele = np.repeat(np.arange(n_eles), n_ppts)
    opp = np.tile(d["opp_p"].T, (1, n_eles))  # column (e, j) = row j of opp_p
    want = U.probe_fields(d["disu_ppts"].transpose(1, 0, 2).reshape(-1, n_fields), names, gamma)
    fwd = U.probe_fields(U.interpolate(opp, ele, d["u_init"]), names, gamma)
    rev = U.probe_fields(U.interpolate_reversed(opp, ele, d["u_init"]), names, gamma)
    for f, a, b in zip(names, U.field_rel(fwd, want), U.field_rel(rev, fwd)):
        print("%s %s: ascending against the reference %.3e, reversed against ascending %.3e" % (name, f, a, b))
        assert a < 1e-13 and b < 1e-13
