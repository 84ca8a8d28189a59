"""Sum-factorised over-integration and shock capturing (csrc/tensor_ops.hip) at every instantiated size: TEST INFRASTRUCTURE.

What tests/test_tensor_ops_host.py (no device) and tests/test_gpu_tensor_ops.py share:

  - registrations of small host-mirror boxes with over-integration and / or shock capturing, in the fixtures' form;
  - a plain reference of the two operations in numpy longdouble, from the DENSE registered matrices and nothing else (no 1-D
    factor, no mode permutation: what the kernels recover from the matrices is not used to judge them);
  - sensor inputs on which the filter decision is not a matter of rounding;
  - a lockstep run of the oracle over whole steps, in the call order of tests/test_oracle_vs_golden.py.

Everything returned from a cache is read-only.
"""
import ctypes as C

import numpy as np

LD = np.longdouble

# the instantiation table of csrc/tensor_ops.hip: N solution points per direction (P1..P5), N <= Nc <= 10 cubature points
NS = (2, 3, 4, 5, 6)
NC_MAX = 10
OVER_INT_SIZES = [(dims, N, Nc) for dims in (2, 3) for N in NS for Nc in range(N, NC_MAX + 1)]
SHOCK_SIZES = [(dims, N) for dims in (2, 3) for N in NS]
assert len(OVER_INT_SIZES) == 70 and len(SHOCK_SIZES) == 10

# 27 hexahedra / 16 quadrilaterals: the smallest blocks on which a capped grid gives its workgroups unequal trips (persistent_grid_cap
# 2: 14 and 13, or 8 and 8; 3: 9 each, or 6 / 5 / 5)
SHAPE = {3: [3, 3, 3], 2: [4, 4, 1]}
AMP = 0.1
# (tests/test_element_orientation.py: at this Mach number and viscosity every term of the residual moves the state within two steps)
MACH, MU_GAS = 0.5, 1.827e-03
# the filter of the reference's shipped cases (hex_p4_jet), and a gentle one for runs of several stages: the shipped one removes the
# highest mode of an element the first time it fires, after which the element's sensor is far below s0 for good and the later
# stages would exercise the filter branch on no element.  The gentle one takes exp(-0.001) off a mode of degree `order` per
# direction: a filtered element's sensor falls by at most 0.6 % per stage (6 % over two steps), so only the few elements that
# close above s0 change sides during a run, and the filtered state still differs from the unfiltered one by 1e-5 of the high
# modes, seven decades above the bars.
FILTER = dict(expf_fac=36.0, expf_order=4, expf_cutoff=1)
GENTLE = dict(expf_fac=0.001, expf_order=4, expf_cutoff=0)

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def frozen(a):
    a = np.asfortranarray(a)
    a.setflags(write=False)
    return a


def relerr(a, b):
    scale = np.abs(b).max()
    return float(np.abs(a - b).max() / (scale if scale > 0 else 1.0))


def curved_quads_xv(n):
    """vertices of the periodic box of n[0] x n[1] quadrilaterals, every one moved along both axes by a product of waves in x and
    y.  (The host mirror's own 2-D deformation moves x by a function of y alone and y by one of x alone: every quadrilateral stays
    a parallelogram, its metrics are the same at all of its points, and a kernel that reads the metrics of the wrong cubature
    point of the right element goes unnoticed -- tests/test_tensor_ops_host.py, the exchanged directions.)"""
    L = 6.2831853071795862
    iy, ix = np.indices((n[1] + 1, n[0] + 1))
    x, y = L * ix.ravel() / n[0], L * iy.ravel() / n[1]
    return np.asfortranarray(np.stack([x + AMP * np.sin(x + 0.4) * np.cos(y + 0.3), y + AMP * np.cos(x + 0.7) * np.sin(y + 0.2)], axis=1))


def registration(dims, order, over_int_order=None, shock=None, mesh="deformed", n=None):
    """the registration dict (hfx_host.Case.registration) of a periodic box of the host mirror with over-integration
    (over_int_order: Nc - 1) and / or shock capturing (shock: dict of shock_det_field, s0 and the expf_* keys; defaults density, 0,
    FILTER), plus loc_upts, tloc_fpts, loc_over_int_cubpts.  mesh: "deformed" (amp 0.1: every element, and every point of an
    element, has metrics of its own; in 2-D the vertices of curved_quads_xv) or "box"; n: cells per direction (default SHAPE)"""
    sh = None if shock is None else dict(dict(shock_det_field=0, s0=0.0, **FILTER), **shock)
    key = ("reg", dims, order, over_int_order, None if sh is None else tuple(sorted(sh.items())), mesh, None if n is None else tuple(n))

    def make():
        import hfx_host as H
        shape = list(n) if n is not None else SHAPE[dims]
        kw = dict(order=order, amp=AMP if mesh == "deformed" else 0.0, Mach_c_ic=MACH, mu_gas=MU_GAS)
        if dims == 2:
            kw["dims"] = 2
            if mesh == "deformed":
                kw["xv"] = curved_quads_xv(shape)
        if over_int_order is not None:
            kw.update(over_int=1, over_int_order=over_int_order)
        if sh is not None:
            kw.update(shock_cap=1, **sh)
        c = H.Case(shape, **kw)
        reg = c.registration()
        reg["loc_upts"], reg["tloc_fpts"] = c.array("loc_upts"), c.array("tloc_fpts")
        if over_int_order is not None:
            reg["loc_over_int_cubpts"] = c.array("loc_over_int_cubpts")
        c.close()
        for v in reg.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        return reg
    return cached(key, make)


def solver_keys(reg):
    """`reg` without the point locations: what oracle_py.Case, build() and reorient take"""
    return {k: v for k, v in reg.items() if k not in ("loc_upts", "tloc_fpts", "loc_over_int_cubpts")}


def with_s0(reg, s0):
    return dict(reg, s0=np.array([float(s0)]))


# ---- the two operations in longdouble, from the dense matrices -----------------------------------------------------------------

def euler_flux(u, gamma):
    """F[pt, ele, field, dir] of the conserved state u[pt, ele, field] (src/flux.cpp, calc_invf_2d / calc_invf_3d)"""
    nd = u.shape[2] - 2
    rho, E = u[:, :, 0], u[:, :, nd + 1]
    v = [u[:, :, 1 + i] / rho for i in range(nd)]
    p = (gamma - 1) * (E - sum(u[:, :, 1 + i] * v[i] for i in range(nd)) / 2)
    F = np.zeros(u.shape + (nd,), dtype=u.dtype)
    for m in range(nd):
        F[:, :, 0, m] = u[:, :, 1 + m]
        for i in range(nd):
            F[:, :, 1 + i, m] = u[:, :, 1 + i] * v[m] + (p if i == m else 0)
        F[:, :, nd + 1, m] = (E + p) * v[m]
    return F


def ref_over_int(reg, u, opp=None, filt=None, jg=None):
    """eles::evaluate_invFlux_over_int (src/eles.cpp:1480-1545): over_int_filter . (JGinv_over_int_cubpts . F_inv(opp_over_int_cubpts
    . u)) per element, field and direction, in the layout of s0_tdisf_upts_inv (n_upts, n_eles, n_fields, n_dims), longdouble.
    opp / filt / jg: other matrices or metrics than the registered ones (the mutations of tests/test_tensor_ops_host.py)"""
    opp = np.asarray(reg["opp_over_int_cubpts"] if opp is None else opp, dtype=LD)
    filt = np.asarray(reg["over_int_filter"] if filt is None else filt, dtype=LD)
    jg = np.asarray(reg["JGinv_over_int_cubpts"] if jg is None else jg, dtype=LD)  # (ref dir, phys dir, cubpt, ele)
    u = np.asarray(u, dtype=LD)
    nu, ne, nf = u.shape
    nd, nc = nf - 2, opp.shape[0]
    ucub = (opp @ u.reshape(nu, ne * nf, order="F")).reshape((nc, ne, nf), order="F")
    F = euler_flux(ucub, LD(float(np.ravel(reg["gamma"])[0])))
    t = np.zeros((nc, ne, nf, nd), dtype=LD)
    for l in range(nd):
        for m in range(nd):
            t[:, :, :, l] += jg[l, m][:, :, None] * F[:, :, :, m]
    return (filt @ t.reshape(nc, ne * nf * nd, order="F")).reshape((nu, ne, nf, nd), order="F")


def ref_sensor(reg, u, field=None, high=None):
    """eles_hexas / eles_quads ::shock_det_persson (src/eles_hexas.cpp:1007-1059, src/eles_quads.cpp:837-890): the modal coefficients
    inv_vandermonde . u[field], squared; the sum over the modes with a degree == order in some direction, weighted by
    norm_basis_persson, over the weighted sum over all modes.  longdouble (n_eles)"""
    u = np.asarray(u, dtype=LD)
    nd = u.shape[2] - 2
    if field is None:
        field = 0 if int(np.ravel(reg["shock_det_field"])[0]) == 0 else nd + 1
    m2 = (np.asarray(reg["inv_vandermonde"], dtype=LD) @ u[:, :, field]) ** 2
    nb = np.asarray(np.ravel(reg["norm_basis_persson"]), dtype=LD)
    hi = np.ravel(reg["persson_high_modes"] if high is None else high).astype(bool)
    return (m2[hi] * nb[hi, None]).sum(axis=0) / (m2 * nb[:, None]).sum(axis=0)


def ref_shock(reg, u, s0=None):
    """eles::shock_capture (src/eles.cpp:2918-2959): (sensor, u with exp_filter . u on all fields of the elements with sensor >= s0,
    every other element untouched), longdouble"""
    s0 = float(np.ravel(reg["s0"])[0]) if s0 is None else float(s0)
    u = np.asarray(u, dtype=LD)
    nu, ne, nf = u.shape
    sensor = ref_sensor(reg, u)
    out = u.copy(order="F")
    el = np.flatnonzero(sensor >= LD(s0))
    if el.size:
        out[:, el, :] = (np.asarray(reg["exp_filter"], dtype=LD) @ u[:, el, :].reshape(nu, el.size * nf, order="F")).reshape(
            (nu, el.size, nf), order="F")
    return sensor, out


# ---- sensor inputs that discriminate ----------------------------------------------------------------------------------------------

def spread_sensors(reg, seed, u=None):
    """u_init (or u) with a seeded multiple of the element's HIGHEST tensor mode (degree `order` in every direction: the last
    column of the Vandermonde matrix, i.e. of inv_vandermonde's inverse) added to the sensor field of every element.  Relative
    amplitudes log-uniform over two decades, 1e-3 .. 1e-1 of the element's mean of that field (|P_n| <= 1 and the kinetic energy
    at Mach 0.5 is 7 % of the total: density and pressure stay positive, asserted).  The sensors gain amplitude^2, four decades;
    from P2 on that is far above the smooth field's own sensors, at P1 (whose own are 1e-2) it moves them by their own size."""
    u = np.array(reg["u_init"] if u is None else u, dtype=np.float64, order="F")
    nd = u.shape[2] - 2
    field = 0 if int(np.ravel(reg["shock_det_field"])[0]) == 0 else nd + 1
    mode = np.linalg.inv(np.asarray(reg["inv_vandermonde"]))[:, -1]
    mode = mode / np.abs(mode).max()
    rng = np.random.RandomState(seed)
    amp = 10.0 ** rng.uniform(-3.0, -1.0, size=u.shape[1])
    u[:, :, field] += mode[:, None] * (amp * u[:, :, field].mean(axis=0))[None, :]
    rho, E = u[:, :, 0], u[:, :, nd + 1]
    p = E - 0.5 * (u[:, :, 1:nd + 1] ** 2).sum(axis=2) / rho
    assert rho.min() > 0 and p.min() > 0
    return u


def pick_s0(sensors):
    """the geometric mean of the two sorted values on either side of the median"""
    s = np.sort(np.asarray(sensors, dtype=np.float64).ravel())
    m = s.size // 2
    return float(np.sqrt(s[m - 1] * s[m]))


def clear_of_s0(sensors, s0, rel=1e-6):
    return bool((np.abs(np.asarray(sensors, dtype=np.float64) - s0) > rel * s0).all())


def quarter_each_way(sensors, s0):
    n = np.asarray(sensors).size
    hit = int((np.asarray(sensors) >= s0).sum())
    return 4 * hit >= n and 4 * (n - hit) >= n


# ---- whole steps of the oracle ------------------------------------------------------------------------------------------------------

def oracle_steps(reg, n_steps, u_init=None, threads=4):
    """The oracle over n_steps RK steps on `reg` (over-integration inside every residual where reg has it, shock capturing after
    every stage where it has that): dict of u (the state after each step) and -- with shock capturing -- sensors (n_steps,
    n_stages, n_eles) as every stage's shock_capture left them.  The stage order is rk_stage's of
    tests/test_oracle_vs_golden.py."""
    import oracle_py as O
    from test_oracle_vs_golden import rk_stage
    o = O.load()
    c = O.Case(solver_keys(reg), u_init=u_init)
    e = c.c_eles()
    f, nfb = c.c_faces()
    bd, nbd = c.c_bdy()
    sh = c.c_shock() if c.shock_cap else None
    n_rk = c.params.n_rk if c.params.adv_type else 1
    us, sensors = [], np.zeros((n_steps, n_rk, c.n_eles))
    o.orc_set_threads(threads)  # (the same bits with any number of threads: tests/test_oracle_vs_golden.py)
    try:
        for st in range(n_steps):
            for rk in range(n_rk):
                rk_stage(o, c, e, f, nfb, bd, nbd, sh, rk)
                if sh is not None:
                    sensors[st, rk] = c.arr["sensor"]
            us.append(frozen(c.arr["u0"].copy(order="F")))
    finally:
        o.orc_set_threads(1)
    assert all(np.isfinite(u).all() for u in us)
    return dict(u=us, sensors=frozen(sensors) if sh is not None else None)


def oracle_over_int(reg, u):
    """orc_evaluate_invFlux_over_int on the state u: tdisf_upts (n_upts, n_eles, n_fields, n_dims)"""
    import oracle_py as O
    c = O.Case(solver_keys(reg), u_init=u)
    e = c.c_eles()
    O.load().orc_evaluate_invFlux_over_int(C.byref(e), C.byref(c.params), C.c_int(c.n_cub), e.opp_over_int_cubpts, e.over_int_filter,
                                           e.JGinv_over_int_cubpts)
    return c.arr["tdisf_upts"].copy(order="F")


def oracle_shock(reg, u):
    """orc_shock_capture on the state u: (sensor, u after the filter)"""
    import oracle_py as O
    c = O.Case(solver_keys(reg), u_init=u)
    e = c.c_eles()
    sh = c.c_shock()
    O.load().orc_shock_capture(C.byref(e), C.byref(sh))
    return c.arr["sensor"].copy(), c.arr["u0"].copy(order="F")


# ---- the stage cases of tests/test_gpu_tensor_ops.py (3), with the input and the threshold both test files use ----------------------

STAGE_SIZES = {2: [(2, 2), (2, 10), (3, 5), (4, 6), (5, 7), (6, 6), (6, 10)],
               3: [(2, 2), (2, 10), (3, 5), (4, 6), (5, 7), (5, 9), (6, 6)]}
STAGE_STEPS = 2
SEED = 5  # of spread_sensors; tests/test_tensor_ops_host.py asserts what it has to deliver


def stage_case(dims, N, Nc, over_int, shock, reoriented=False):
    """(registration with s0 set, initial state) of a stage run at (N, Nc): over_int / shock say which ingredients it has.  With shock
    capturing the initial state is spread_sensors' and s0 pick_s0 of the longdouble sensors of that state; the filter is GENTLE."""
    def make():
        reg = registration(dims, N - 1, Nc - 1 if over_int else None, dict(GENTLE) if shock else None)
        u = np.asarray(reg["u_init"])
        if shock:
            u = spread_sensors(reg, SEED)
            reg = with_s0(reg, pick_s0(ref_sensor(reg, u)))
        return reg, frozen(u)
    return cached(("stage", dims, N, Nc, over_int, shock), make)


def stage_oracle(dims, N, Nc, over_int, shock):
    def make():
        reg, u = stage_case(dims, N, Nc, over_int, shock)
        return oracle_steps(reg, STAGE_STEPS, u_init=u)
    return cached(("stage_oracle", dims, N, Nc, over_int, shock), make)
