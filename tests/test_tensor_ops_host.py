"""The inputs and the reference of tests/test_gpu_tensor_ops.py, without a device.

tests/test_gpu_tensor_ops.py holds the sum-factorised over-integration and shock-capturing kernels (csrc/tensor_ops.hip) against a
numpy longdouble reference at every instantiated size.  Here: (a) that reference agrees with the oracle and with the genuine
reference's fixtures; (b) the host mirror's matrices at every size have the properties that define them, checked without the
mirror's formulas; (c) the inputs discriminate -- every mistake these kernels can make (a slipped prefetch, a dropped point, a wrong
pass stride, a folded matrix along the wrong direction, weights in the wrong mode order, the wrong sensor field) moves the reference
by far more than any bar; (d) on every run the device tests make, the filter decision cannot hang on rounding; (e) the
re-orientation rule of JGinv_over_int_cubpts (tests/reorient.py) is the right one."""
import glob
import os

import numpy as np
import pytest
from numpy.polynomial import legendre as NL

import reorient as RO
import tensor_ops_util as T

LD = T.LD
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
MOVES = 1e-6  # what a mutation must move the reference by, relative to its largest magnitude


def fixture(name):
    return T.cached(("fixture", name), lambda: dict(np.load(os.path.join(GOLDEN, name + ".npz"))))


def tensor_fixtures(key):
    """the fixtures of quadrilaterals / hexahedra that hold `key`"""
    out = []
    for n in FIXTURES:
        if n.startswith(("hex_", "quad_")) and "_tgv" not in n:
            with np.load(os.path.join(GOLDEN, n + ".npz")) as d:
                if key in d.files and "sizes" in d.files and "u_init" in d.files:
                    out.append(n)
    return out


OVERINT_FIXTURES = [n for n in tensor_fixtures("s0_tdisf_upts_inv") if n in tensor_fixtures("over_int")]
SENSOR_FIXTURES = tensor_fixtures("s0_sensor")


# ---- the mode order and the polynomials, restated ---------------------------------------------------------------------------------

def hierarchical_degrees(nd, p):
    """the degrees (one row per mode) in the reference's order: by the sum of the degrees, inside a sum the last direction's degree
    ascending, then the one before (eval_legendre_basis_3D_hierarchical, src/eles_hexas.cpp:1364; 2-D: src/eles_quads.cpp:1116)"""
    out = []
    if nd == 3:
        for s in range(3 * p + 1):
            for k in range(s + 1):
                for j in range(s - k + 1):
                    i = s - k - j
                    if i <= p and j <= p and k <= p:
                        out.append((i, j, k))
    else:
        for s in range(2 * p + 1):
            for j in range(s + 1):
                i = s - j
                if i <= p and j <= p:
                    out.append((i, j))
    return np.array(out)


def legendre_at(x, m):
    return NL.legval(np.asarray(x, dtype=np.float64), [0.0] * m + [1.0])


def tensor_legendre(loc, deg):
    """prod_d P_deg[d](loc[d, :])"""
    out = np.ones(loc.shape[1])
    for d in range(loc.shape[0]):
        out = out * legendre_at(loc[d], int(deg[d]))
    return out


def vandermonde(reg):
    nd, p = int(reg["sizes"][4]), int(reg["sizes"][5])
    return np.stack([tensor_legendre(np.asarray(reg["loc_upts"]), deg) for deg in hierarchical_degrees(nd, p)], axis=1)


def expf_sigma(deg, p, fac, order, cutoff):
    """the diagonal of set_exp_filter (src/eles_hexas.cpp:953-985) for one mode"""
    eta_c = cutoff / p
    s = 1.0
    for m in deg:
        eta = m / p
        if eta > eta_c:
            s *= np.exp(-fac * ((eta - eta_c) / (1.0 - eta_c)) ** order)
    return s


# ---- (a) the longdouble reference against the oracle and the fixtures ---------------------------------------------------------------

@pytest.mark.parametrize("dims,N,Nc", T.OVER_INT_SIZES)
def test_reference_over_integration_vs_oracle(oracle, dims, N, Nc):
    reg = T.registration(dims, N - 1, Nc - 1)
    assert reg["opp_over_int_cubpts"].shape == (Nc ** dims, N ** dims) and reg["over_int_filter"].shape == (N ** dims, Nc ** dims)
    want = T.ref_over_int(reg, reg["u_init"])
    got = T.oracle_over_int(reg, reg["u_init"])
    assert T.relerr(got, want.astype(np.float64)) < 1e-13


@pytest.mark.parametrize("cutoff", [0, 1])
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("dims,N", T.SHOCK_SIZES)
def test_reference_shock_capture_vs_oracle(oracle, dims, N, field, cutoff):
    reg = T.registration(dims, N - 1, None, dict(T.FILTER, shock_det_field=field, expf_cutoff=cutoff))
    u = T.spread_sensors(reg, T.SEED)
    reg = T.with_s0(reg, T.pick_s0(T.ref_sensor(reg, u)))
    want_s, want_u = T.ref_shock(reg, u)
    got_s, got_u = T.oracle_shock(reg, u)
    assert T.relerr(got_s, want_s.astype(np.float64)) < 1e-13
    assert np.array_equal(got_s >= reg["s0"][0], want_s >= reg["s0"][0])
    assert T.relerr(got_u, want_u.astype(np.float64)) < 1e-13


@pytest.mark.parametrize("name", OVERINT_FIXTURES)
def test_reference_over_integration_vs_fixture(name):
    d = fixture(name)
    assert T.relerr(T.ref_over_int(d, d["u_init"]).astype(np.float64), d["s0_tdisf_upts_inv"]) < 1e-12


@pytest.mark.parametrize("name", SENSOR_FIXTURES)
def test_reference_sensor_vs_fixture(name):
    d = fixture(name)
    got = T.ref_sensor(d, d["s0_u_before_shock_capture"]).astype(np.float64)
    assert T.relerr(got, np.ravel(d["s0_sensor"])) < 1e-9


def test_the_new_fixtures_are_among_them():
    new = ["hex_p1_overint_shock_min", "hex_p1_overint_shock_max", "hex_p5_overint_shock", "quad_p1_overint_shock",
           "quad_p5_overint_shock", "quad_p2_overint_shock"]
    assert set(new) <= set(OVERINT_FIXTURES) and set(new) <= set(SENSOR_FIXTURES)
    sizes = {(int(fixture(n)["sizes"][4]), int(fixture(n)["sizes"][5]) + 1, round(fixture(n)["opp_over_int_cubpts"].shape[0] ** (1.0 / int(fixture(n)["sizes"][4]))))
             for n in new}
    assert sizes == {(3, 2, 2), (3, 2, 10), (3, 6, 6), (2, 2, 2), (2, 6, 10), (2, 3, 5)}


# ---- (b) the mirror's matrices at every size ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,N,Nc", T.OVER_INT_SIZES)
def test_over_integration_matrices(dims, N, Nc):
    """over_int_filter . opp_over_int_cubpts = I (a polynomial of the solution space is projected on itself), and what the
    projection removes from ANY function at the cubature points is orthogonal to every tensor Legendre polynomial of degree < N
    per direction under the Gauss weights"""
    reg = T.registration(dims, N - 1, Nc - 1)
    opp, filt, loc = np.asarray(reg["opp_over_int_cubpts"]), np.asarray(reg["over_int_filter"]), np.asarray(reg["loc_over_int_cubpts"])
    assert np.abs(filt @ opp - np.eye(N ** dims)).max() < 1e-12
    x, w = NL.leggauss(Nc)
    for d in range(dims):  # a tensor Gauss set, first direction fastest
        assert np.abs(np.sort(np.unique(np.round(loc[d], 12))) - np.round(x, 12)).max() < 1e-11
    weight = np.ones(Nc ** dims)
    for d in range(dims):
        weight = weight * w[np.argmin(np.abs(loc[d][:, None] - x[None, :]), axis=1)]
    g = np.random.RandomState(7).standard_normal(Nc ** dims)
    r = g - opp @ (filt @ g)
    for deg in hierarchical_degrees(dims, N - 1):
        assert abs(np.sum(weight * tensor_legendre(loc, deg) * r)) < 1e-12 * np.abs(g).max(), deg


@pytest.mark.parametrize("cutoff", [0, 1])
@pytest.mark.parametrize("dims,N", T.SHOCK_SIZES)
def test_shock_capture_matrices(dims, N, cutoff):
    """inv_vandermonde . vandermonde = I with the Vandermonde matrix of the hierarchical tensor Legendre basis restated here;
    exp_filter = V diag(sigma) V^-1 with sigma from the reference's set_exp_filter formula, and it keeps the element mean (mode
    0); the high-mode flags are the reference's rule (a degree == order in some direction); norm_basis_persson its formula"""
    p = N - 1
    reg = T.registration(dims, p, None, dict(T.FILTER, expf_cutoff=cutoff))
    V = vandermonde(reg)
    W, E = np.asarray(reg["inv_vandermonde"]), np.asarray(reg["exp_filter"])
    assert np.abs(W @ V - np.eye(N ** dims)).max() < 1e-12
    deg = hierarchical_degrees(dims, p)
    sigma = np.array([expf_sigma(m, p, T.FILTER["expf_fac"], T.FILTER["expf_order"], cutoff) for m in deg])
    assert np.abs(E - V @ (sigma[:, None] * np.linalg.inv(V))).max() < 1e-12
    assert sigma[0] == 1.0 and np.abs(W[0] @ E - W[0]).max() < 1e-12 * np.abs(W[0]).max()
    assert np.array_equal(np.ravel(reg["persson_high_modes"]).astype(bool), (deg == p).any(axis=1))
    assert np.abs(np.ravel(reg["norm_basis_persson"]) - np.prod(2.0 / (2.0 * deg + 1.0), axis=1)).max() < 1e-15
    if p > cutoff:
        assert sigma.min() < 1e-10  # (the shipped filter removes the highest mode: tensor_ops_util.GENTLE says why that matters)


# ---- (c) the inputs discriminate --------------------------------------------------------------------------------------------------------

MUTATION_SIZES = [(2, 2, 2), (2, 4, 6), (2, 6, 10), (3, 2, 2), (3, 3, 5), (3, 5, 7), (3, 2, 10)]


def moved(a, b):
    return T.relerr(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))


@pytest.mark.parametrize("dims,N,Nc", MUTATION_SIZES)
def test_over_integration_mutations_move_the_reference(dims, N, Nc):
    reg = T.registration(dims, N - 1, Nc - 1)
    u, jg = np.asarray(reg["u_init"]), np.asarray(reg["JGinv_over_int_cubpts"])
    want = T.ref_over_int(reg, u)
    # a slipped prefetch: the metrics, or the state, of element e + k (k workgroups further: caps 1-3) in place of e's
    for k in (1, 2, 3):
        assert moved(T.ref_over_int(reg, u, jg=np.roll(jg, -k, axis=3)), want) > MOVES, ("metrics", k)
        assert moved(T.ref_over_int(reg, np.roll(u, -k, axis=1)), want) > MOVES, ("state", k)
    # the last cubature point dropped (a loop bound one short, a point of the last partial pass of the lanes)
    assert moved(T.ref_over_int(reg, u, opp=np.asarray(reg["opp_over_int_cubpts"])[:-1], filt=np.asarray(reg["over_int_filter"])[:, :-1],
                                jg=jg[:, :, :-1]), want) > MOVES
    # the cubature points of two directions exchanged (a pass with the wrong stride leaves the values transposed)
    swap = np.arange(Nc ** dims).reshape([Nc] * dims, order="F").swapaxes(0, 1).ravel(order="F")
    assert moved(T.ref_over_int(reg, u, jg=jg[:, :, swap]), want) > MOVES
    # the folded form: sum_l A_l tdisf_l, A_l = opp_2[l] - opp_3 opp_1[l]; the matrix of one direction used along another
    A = [np.asarray(reg["opp_2_%d" % l], dtype=LD) - np.asarray(reg["opp_3"], dtype=LD) @ np.asarray(reg["opp_1_%d" % l], dtype=LD)
         for l in range(dims)]
    nu, ne, nf, nd = want.shape
    fold = lambda mats: sum(mats[l] @ want[:, :, :, l].reshape(nu, ne * nf, order="F") for l in range(nd))
    assert moved(fold([A[1], A[0]] + A[2:]), fold(A)) > MOVES


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("dims,N", T.SHOCK_SIZES)
def test_shock_capture_mutations_move_the_reference(dims, N, field):
    reg = T.registration(dims, N - 1, None, dict(T.FILTER, shock_det_field=field))
    u = T.spread_sensors(reg, T.SEED)
    want = T.ref_sensor(reg, u)
    # the sensor weights left in the hierarchical order while the modal coefficients are in tensor order
    deg = hierarchical_degrees(dims, N - 1)
    t_of_h = sum(deg[:, d] * N ** d for d in range(dims))
    m2 = (np.asarray(reg["inv_vandermonde"], dtype=LD) @ np.asarray(u[:, :, 0 if field == 0 else dims + 1], dtype=LD)) ** 2
    m2_tensor = np.zeros_like(m2)
    m2_tensor[t_of_h] = m2
    nb, hi = np.asarray(np.ravel(reg["norm_basis_persson"]), dtype=LD), np.ravel(reg["persson_high_modes"]).astype(bool)
    right = (m2_tensor[t_of_h][hi] * nb[hi, None]).sum(axis=0) / (m2_tensor[t_of_h] * nb[:, None]).sum(axis=0)
    assert moved(right, want) < 1e-15  # (the permutation itself is the right one)
    wrong = (m2_tensor[hi] * nb[hi, None]).sum(axis=0) / (m2_tensor * nb[:, None]).sum(axis=0)
    # (the four modes of a P1 quadrilateral are in the same order either way: the one size at which there is nothing to get wrong)
    assert np.array_equal(t_of_h, np.arange(N ** dims)) == ((dims, N) == (2, 2))
    if (dims, N) != (2, 2):
        assert moved(wrong, want) > MOVES
    # the other field
    assert moved(T.ref_sensor(reg, u, field=dims + 1 if field == 0 else 0), want) > MOVES
    # the state or the sensor of another element
    for k in (1, 2, 3):
        assert moved(np.roll(want, -k), want) > MOVES


# ---- (d) sensor conditions on every run the device tests make ------------------------------------------------------------------------

@pytest.mark.parametrize("cutoff", [0, 1])
@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("dims,N", T.SHOCK_SIZES)
def test_sensor_conditions_of_the_per_method_cases(dims, N, field, cutoff):
    reg = T.registration(dims, N - 1, None, dict(T.FILTER, shock_det_field=field, expf_cutoff=cutoff))
    u = T.spread_sensors(reg, T.SEED)
    s = T.ref_sensor(reg, u).astype(np.float64)
    s0 = T.pick_s0(s)
    assert T.quarter_each_way(s, s0) and T.clear_of_s0(s, s0)


STAGE_SHOCK_CASES = [(dims, N, Nc, oi) for dims in (2, 3) for (N, Nc) in T.STAGE_SIZES[dims] for oi in (False, True)]


@pytest.mark.parametrize("dims,N,Nc,over_int", STAGE_SHOCK_CASES)
def test_sensor_conditions_of_the_stage_cases(oracle, dims, N, Nc, over_int):
    """at every stage of the oracle's run at least a quarter of the elements are filtered and a quarter are not, and no sensor
    lies within 1e-6 of s0"""
    reg, u = T.stage_case(dims, N, Nc, over_int, True)
    s0 = float(reg["s0"][0])
    sens = T.stage_oracle(dims, N, Nc, over_int, True)["sensors"]
    assert sens.shape[:2] == (T.STAGE_STEPS, 5)
    for st in range(sens.shape[0]):
        for rk in range(sens.shape[1]):
            assert T.quarter_each_way(sens[st, rk], s0), (st, rk, np.sort(sens[st, rk]), s0)
            assert T.clear_of_s0(sens[st, rk], s0), (st, rk)


@pytest.mark.parametrize("dims,N,Nc", [(2, 2, 2), (3, 3, 5), (2, 6, 10), (3, 6, 6)])
def test_stage_result_sees_a_slipped_prefetch(oracle, dims, N, Nc):
    """the state the stage tests compare after two steps (at 1e-11) moves by more than 1e-6 when every element takes the cubature
    metrics of the next one, and by more than 1e-5 per step at all: the time step is not so small that the residual hides"""
    reg, u0 = T.stage_case(dims, N, Nc, True, False)
    want = T.stage_oracle(dims, N, Nc, True, False)
    assert T.relerr(want["u"][0], u0) > 1e-5
    slipped = dict(reg, JGinv_over_int_cubpts=np.roll(np.asarray(reg["JGinv_over_int_cubpts"]), -1, axis=3))
    assert T.relerr(T.oracle_steps(slipped, T.STAGE_STEPS, u_init=u0)["u"][-1], want["u"][-1]) > MOVES


# ---- (e) re-oriented blocks -----------------------------------------------------------------------------------------------------------

REORIENTED = [(3, 5, 7), (2, 4, 6)]
ORIENT_SEED = {3: 1, 2: 3}  # (tests/test_element_orientation.py: all 24 / 4 rotations present)


def reoriented_case(dims, N, Nc):
    """(plain registration with s0 and the spread state as u_init, the same re-oriented, rot)"""
    def make():
        reg, u = T.stage_case(dims, N, Nc, True, True)
        plain = dict(T.solver_keys(reg), u_init=u)
        rot = RO.orientation_vector(int(reg["sizes"][0]), dims, ORIENT_SEED[dims])
        assert len(set(rot)) == (24 if dims == 3 else 4)
        turned = RO.reorient(plain, rot, reg["loc_upts"], reg["tloc_fpts"], reg["loc_over_int_cubpts"])
        return plain, turned, rot
    return T.cached(("reoriented", dims, N, Nc), make)


def reoriented_oracle(dims, N, Nc, which):
    return T.cached(("reoriented_oracle", dims, N, Nc, which),
                    lambda: T.oracle_steps(reoriented_case(dims, N, Nc)[which], T.STAGE_STEPS))


@pytest.mark.parametrize("dims,N,Nc", REORIENTED)
def test_oracle_does_not_depend_on_the_orientation(oracle, dims, N, Nc):
    plain, turned, rot = reoriented_case(dims, N, Nc)
    a, b = reoriented_oracle(dims, N, Nc, 0), reoriented_oracle(dims, N, Nc, 1)
    for st in range(T.STAGE_STEPS):
        assert T.relerr(RO.back(b["u"][st], rot), a["u"][st]) < 1e-12, st
    s0 = float(plain["s0"][0])
    assert T.relerr(b["sensors"], a["sensors"]) < 1e-10
    assert np.array_equal(b["sensors"] >= s0, a["sensors"] >= s0)
    for st in range(T.STAGE_STEPS):
        for rk in range(a["sensors"].shape[1]):
            assert T.quarter_each_way(b["sensors"][st, rk], s0) and T.clear_of_s0(b["sensors"][st, rk], s0)


@pytest.mark.parametrize("dims,N,Nc", REORIENTED)
def test_unpermuted_cubature_metrics_are_noticed(oracle, dims, N, Nc):
    plain, turned, rot = reoriented_case(dims, N, Nc)
    wrong = dict(turned, JGinv_over_int_cubpts=plain["JGinv_over_int_cubpts"])
    got = T.oracle_steps(wrong, 1)["u"][0]
    assert T.relerr(RO.back(got, rot), reoriented_oracle(dims, N, Nc, 0)["u"][0]) > MOVES
    # ... and on the operation alone
    a = T.ref_over_int(turned, turned["u_init"])
    b = T.ref_over_int(wrong, turned["u_init"])
    assert moved(b, a) > MOVES
