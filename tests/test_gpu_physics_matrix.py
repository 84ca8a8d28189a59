"""Every run-wide switch of the face-point physics on every common-flux kernel family: kernel family x switch row.

The pairwise kernels take the Riemann solver as a template argument (csrc/face_kernels.hpp: `template <int ND, int RS>`), the
per-method path, the partition-face kernels and the boundary kernels take the runtime dispatch; every (kernel, ND, RS) is
machine code of its own, and the fixtures of the genuine reference vary one switch at a time on one element class each
(tests/test_branch_census.py::test_switch_table).  Here every family runs every row for two time steps and is held
against the oracle (oracle/oracle.c, pinned against the fixtures by tests/test_oracle_vs_golden.py) on the same registration
and the same initial state:

    1e-11 on disu_upts0 after the step, 1e-11 on div_tconf_upts (the residual of the step's last stage), both relative to the
    array's largest magnitude -- the bound that the families meet against the reference's fixtures.

A family's registration comes from the host mirror (hfx_host.Case(...).registration()) or, for tetrahedra and prisms, from the
fixtures tet_p2_n2_deformed / pri_p2_n2_deformed; a row overrides the switches in that dictionary, which is what the oracle
(oracle_py.Case) and the library (hfx.params_from) both read.  The switches are plain flags of hfx_params: the host mirror
computes rt_inf, mu_inf and c_sth whatever fix_vis says (csrc/host/input.cpp).

The cases (CASE_KW, STEPS): the Taylor-Green field at Mach 0.5 (the RoeM rows at Mach 1.2, where its wave speeds clip and where it
differs from HLLC by more than the jumps of a smooth P7 field) and a viscosity a hundred times that of the shipped case (Reynolds
number 16), so that the viscous switches move the result by more than rounding within two steps; the rows with Sutherland's law
start from a temperature field (temperature_field below) -- the Taylor-Green start is isothermal, where the law is a constant.
test_rows_are_discriminating (no GPU) holds every row to a difference of 1e-6 from the baseline row of the same case.

Mach 1.2 on quadrilaterals: the 2-D Taylor-Green pressure is positive only below Mach 1.195 (oracle/capture_golden.py,
quad_p3_transonic), so the combined row runs at 1.15 there.  The fixtures of the general stage hold a state at Mach 0.1: the
rows scale its velocity (to Mach 0.5, and to 1.2 for the combined row) at the fixture's density and pressure.
"""
import ctypes as C
import os

import numpy as np
import pytest

import ragged_partition as RP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_U = 1e-11
TOL_DIV = 1e-11
MIN_DIFF = 1e-6  # five orders above the tolerance

BASELINE = dict(riemann_solve_type=3, fix_vis=1, ldg_beta=0.5, ldg_tau=0.0, viscous=1)
# row -> (switch overrides, supersonic start, temperature field)
ROWS = {
    "hllc": (dict(), False, False),
    "rusanov": (dict(riemann_solve_type=0), False, False),
    "roem": (dict(riemann_solve_type=2), True, False),  # (supersonic: RoeM and HLLC differ by the jumps, small at P7 below Mach 1)
    "sutherland": (dict(fix_vis=0), False, True),
    "ldg_tau": (dict(ldg_beta=0.25, ldg_tau=0.3), False, False),
    "beta_minus": (dict(ldg_beta=-0.5), False, False),
    "inviscid": (dict(viscous=0), False, False),
    "roem_sutherland_tau_mach1.2": (dict(riemann_solve_type=2, fix_vis=0, ldg_tau=0.3), True, True),
}
MACH, MACH_SUPERSONIC, MACH_SUPERSONIC_2D = 0.5, 1.2, 1.15
CASE_KW = dict(mu_gas=1.827e-03)
STEPS = 2


def relerr(a, b):
    scale = np.abs(b).max()
    return np.abs(a - b).max() / (scale if scale > 0 else 1.0)


# ---- geometries: the smallest shape at which each kernel form is selected ------------------------------------------------------

def walls_geometry():
    from test_partition_ragged import walls_kw, BOX
    return dict(n=BOX, **walls_kw())


GEOMETRIES = {
    "quad_p3": lambda: dict(n=[4, 3, 1], dims=2, order=3, amp=0.1),
    "quad_p7": lambda: dict(n=[4, 3, 1], dims=2, order=7, amp=0.1),
    "hex_p2": lambda: dict(n=[3, 3, 3], order=2, amp=0.1),
    "hex_p4": lambda: dict(n=[3, 3, 3], order=4, amp=0.1),
    "hex_p4_box": lambda: dict(n=[3, 3, 3], order=4, amp=0.0),  # undeformed: the per-element metric record
    "hex_p6": lambda: dict(n=[3, 3, 3], order=6, amp=0.1),
    "hex_p2_343": lambda: dict(n=[3, 4, 3], order=2, amp=0.1),
    "walls": walls_geometry,
    "tet_p2": "tet_p2_n2_deformed",
    "pri_p2": "pri_p2_n2_deformed",
}

# family -> (geometry, how it runs, fused mode, options, names hfx_time_fused_kernels must / must not report)
FAMILIES = {
    "methods_hex_p2": ("hex_p2", "run_steps", 0, (), (), ()),
    "methods_quad_p3": ("quad_p3", "run_steps", 0, (), (), ()),
    "split2_quad_p3": ("quad_p3", "run_steps", 2, (), ("split_gradient_kernel", "face_flux_kernel"), ()),
    "split3_quad_p3": ("quad_p3", "run_steps", 3, (), ("split_flux_tensor_kernel", "face_flux2_kernel"), ()),
    "split2_quad_p7": ("quad_p7", "run_steps", 2, (), ("split_gradient_kernel", "face_flux_kernel"), ()),
    "split3_quad_p7": ("quad_p7", "run_steps", 3, (), ("face_flux2_kernel",), ()),
    "split2_hex_p2": ("hex_p2", "run_steps", 2, (), ("split_gradient_kernel", "face_flux_kernel"), ()),
    "split3_hex_p2": ("hex_p2", "run_steps", 3, (), ("split_flux_kernel", "face_flux2_kernel"), ()),  # (dictionary rows)
    "split2_hex_p4": ("hex_p4", "run_steps", 2, (), ("split_gradient_kernel", "face_flux_kernel"), ()),
    "split3_hex_p4_general_metrics": ("hex_p4", "run_steps", 3, (), ("split_flux_tensor_kernel", "face_flux2_kernel"),
                                      ("affine_metrics", "affine_block")),
    "split3_hex_p4_affine_two_wave": ("hex_p4_box", "run_steps", 3, (), ("face_flux2_kernel", "affine_metrics", "two_wave"), ()),
    "split3_hex_p4_affine_loader_wave": ("hex_p4_box", "run_steps", 3, (("flux_two_wave", 0),), ("face_flux2_kernel", "affine_metrics"),
                                         ("two_wave",)),
    # 343 points per element: a request for variant 3 runs variant 2 with the wide operator rows (tests/test_gpu_fused_high_order.py)
    "split_hex_p6_wide_rows": ("hex_p6", "run_steps", 3, (), ("split_gradient_kernel", "face_flux_kernel"), ("face_flux2_kernel",)),
    "general_tet_p2": ("tet_p2", "run_steps", 4, (), (), ()),
    "general_pri_p2": ("pri_p2", "run_steps", 4, (), (), ()),
    "partition_faces_hex_p2": ("hex_p2_343", "partitioned", 3, (), (), ()),
    "boundary_faces_hex_p2": ("walls", "run_steps", 3, (), ("face_flux2_kernel",), ()),
}
# an inviscid block forms no LDG corrections and does not take the affine form of the flux kernel (csrc/fused_hex.hip, split_plan;
# tests/test_gpu_flux_two_wave.py::test_inviscid_run_keeps_the_register_pipeline): the block is found affine and keeps the per-point metrics
INVISCID_FORM = {"split3_hex_p4_affine_two_wave": (("face_flux2_kernel", "affine_block"), ("affine_metrics", "two_wave")),
                 "split3_hex_p4_affine_loader_wave": (("face_flux2_kernel", "affine_block"), ("affine_metrics", "two_wave"))}
# the one refusal by design: the box of walls_kw() has an isothermal and an adiabatic wall, which the reference
# (src/input.cpp:406-407, :427-428) and hfx_bdy_inters_create refuse on an inviscid run
REFUSED = {("boundary_faces_hex_p2", "inviscid")}


# ---- registrations, states and the oracle's results: computed once, never written to -------------------------------------------

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def geometry_registration(geometry, supersonic):
    """(registration dict of the undivided mesh, pos_upts) with the Taylor-Green start at the row's Mach number"""
    def make():
        g = GEOMETRIES[geometry]
        if isinstance(g, str):
            d = dict(np.load(os.path.join(GOLDEN, g + ".npz")))
            reg = {k: d[k] for k in d if not k.startswith(("s0_", "u_step", "meta_json"))}
            reg["mu_inf"] = d["mu_inf"] * (CASE_KW["mu_gas"] / 1.827e-05)  # the fixtures hold the shipped case's viscosity
            reg["u_init"] = scale_velocity(d["u_init"], float(np.ravel(d["gamma"])[0]),
                                           (MACH_SUPERSONIC if supersonic else MACH) / 0.1)
            return reg, d["pos_upts"]
        import hfx_host as H
        g = g()
        mach = MACH if not supersonic else MACH_SUPERSONIC_2D if g.get("dims", 3) == 2 else MACH_SUPERSONIC
        c = H.Case(g.pop("n"), Mach_c_ic=mach, **dict(CASE_KW, **g))
        reg, pos = c.registration(), c.array("pos_upts")
        c.close()
        return reg, pos
    return cached(("geometry", geometry, supersonic), make)


def primitives(u, gamma):
    nd = u.shape[2] - 2
    rho = u[..., 0]
    v = u[..., 1:nd + 1] / rho[..., None]
    p = (gamma - 1.0) * (u[..., nd + 1] - 0.5 * rho * (v * v).sum(axis=-1))
    return rho, v, p


def conserved(rho, v, p, gamma):
    return np.asfortranarray(np.concatenate([rho[..., None], rho[..., None] * v,
                                             (p / (gamma - 1.0) + 0.5 * rho * (v * v).sum(axis=-1))[..., None]], axis=-1))


def scale_velocity(u, gamma, factor):
    rho, v, p = primitives(u, gamma)
    return conserved(rho, factor * v, p, gamma)


def temperature_field(u, pos, gamma):
    """the same velocity and pressure at a density that varies by 10 % over the box: T = p / (rho R) no longer uniform"""
    rho, v, p = primitives(u, gamma)
    s = np.sin(pos[..., 0] + 0.3) * np.cos(pos[..., 1] - 0.2)
    if pos.shape[-1] == 3:
        s = s * np.cos(pos[..., 2] + 0.1)
    return conserved(rho * (1.0 + 0.1 * s), v, p, gamma)


def row_registration(geometry, row, switches=None):
    """the geometry's registration with the row's switches and the row's initial state"""
    over, supersonic, t_field = ROWS[row]
    reg, pos = geometry_registration(geometry, supersonic)
    reg = dict(reg)
    if t_field:
        reg["u_init"] = temperature_field(reg["u_init"], pos, float(np.ravel(reg["gamma"])[0]))
    for k, v in dict(BASELINE, **(over if switches is None else switches)).items():
        reg[k] = np.array([float(v)])
    return reg


def oracle_result(geometry, row, switches=None):
    """(u, div) of the oracle after STEPS steps: the row, or (switches = {}) the baseline on the row's initial state"""
    def make():
        import oracle_py as O
        O.load().orc_set_threads(4)  # (the same bits with any number of threads: tests/test_oracle_vs_golden.py)
        try:
            u, div = RP.undivided_oracle(row_registration(geometry, row, switches), STEPS)
        finally:
            O.load().orc_set_threads(1)
        u, div = u.copy(), div.copy()
        assert np.isfinite(u).all() and np.isfinite(div).all()
        u.setflags(write=False)
        div.setflags(write=False)
        return u, div
    state = (ROWS[row][1], ROWS[row][2])
    key = ("oracle", geometry, state, tuple(sorted(dict(BASELINE, **(ROWS[row][0] if switches is None else switches)).items())))
    return cached(key, make)


def matrix():
    return [(f, r) for f in FAMILIES for r in ROWS]


# ---- discriminating power (the oracle alone) ------------------------------------------------------------------------------------

def test_rows_are_discriminating():
    """every row's result differs from the baseline row's on the same case and the same initial state by at least 1e-6 in the
    norm of the comparison, on the state AND on the residual: a kernel that ran the baseline's switch misses the tolerance by
    five orders"""
    geometries = sorted({FAMILIES[f][0] for f in FAMILIES})
    low = []
    print()
    print("%-12s %-30s %12s %12s" % ("geometry", "row", "state", "residual"))
    for g in geometries:
        for row in ROWS:
            if row == "hllc" or ("boundary_faces_hex_p2", row) in REFUSED and g == "walls":
                continue
            u, div = oracle_result(g, row)
            u0, div0 = oracle_result(g, row, {})
            du, dd = relerr(u, u0), relerr(div, div0)
            print("%-12s %-30s %12.3e %12.3e" % (g, row, du, dd))
            if min(du, dd) < MIN_DIFF:
                low.append((g, row, du, dd))
    assert not low, low


def test_every_family_meets_every_row_or_refuses_it():
    assert REFUSED <= set(matrix())
    assert {FAMILIES[f][0] for f in FAMILIES} == set(GEOMETRIES)


# ---- the device ----------------------------------------------------------------------------------------------------------------

def kernel_names(e, faces):
    import hfx
    kt, names = (C.c_double * 8)(), (C.c_char * 256)()
    hfx.check(hfx.lib().hfx_time_fused_kernels(e.h, hfx._face_array(faces), C.c_int(len(faces)), C.c_int(1), kt, names))
    return names.value.decode().split(",")


def run_steps_family(reg, mode, options, must, must_not):
    import hfx
    from test_gpu_methods_vs_golden import build
    ctx = hfx.Context(0)
    e, faces = None, []
    try:
        if mode in (2, 3):
            ctx.set_fused_mode(mode)
        for k, v in options:
            ctx.set_option(k, v)
        e, faces = build(ctx, reg)
        hfx.run_steps(e, faces, STEPS, fused=mode)
        u, div = e.download(hfx.DISU_UPTS0), e.download(hfx.DIV_TCONF_UPTS)
        assert e.check_nan() == -1
        grids = hfx.fused_launch_grids(e.h)
        if mode in (2, 3):
            # the split stage's persistent kernels ran: update / residual, and on a viscous run flux / gradient
            slots = {s for s, _, _ in grids}
            assert 3 in slots and (1 in slots or not int(np.ravel(reg["viscous"])[0])), grids
            names = kernel_names(e, faces)  # (last: it advances the state)
            print("kernels: %s" % names)
            for n in must:
                assert n in names, (n, names)
            for n in must_not:
                assert n not in names, (n, names)
        else:
            assert grids == [], grids  # no split fused stage ran on this block
        return u, div
    finally:
        for f in faces:
            f.close()
        if e is not None:
            e.close()
        ctx.close()


def partitioned_family(geometry, row, mode):
    """hfx_run_steps_partitioned over the library's own transport on a block that is its own neighbour in x and z"""
    import hfx
    import hfx_host as H
    def tables():
        g = GEOMETRIES[geometry]()
        c = H.Case(g.pop("n"), self_partition=[1, 0, 1], Mach_c_ic=MACH_SUPERSONIC if ROWS[row][1] else MACH, **dict(CASE_KW, **g))
        reg, (L, Rlut, _), seg = c.registration(), c.mpi_faces(), c.mpi_segments()
        c.close()
        return reg, L, Rlut, seg
    cut, L, Rlut, seg = cached(("self_partition", geometry, ROWS[row][1]), tables)
    whole = row_registration(geometry, row)
    assert L.shape[1] > 0 and cut["int2_L"].shape[1] + L.shape[1] // 2 == whole["int2_L"].shape[1]
    reg = dict(whole, int2_L=cut["int2_L"], int2_R=cut["int2_R"])  # the row's switches and state on the cut block's tables
    r = RP.GpuPart(reg, L, Rlut, seg, fused_mode=mode)
    comm = hfx.Comm(r.ctx.h, hfx.comm_unique_id(), 1, 0)
    try:
        fi = (C.c_void_p * len(r.ints))(*[f.h for f in r.ints])
        fm = (C.c_void_p * 1)(r.m.h)
        hfx.check(hfx.lib().hfx_run_steps_partitioned(r.e.h, fi, C.c_int(len(r.ints)), fm, C.c_int(1), comm.h, C.c_int(STEPS)))
        r.ctx.synchronize()
        u, div = r.e.download(hfx.DISU_UPTS0), r.e.download(hfx.DIV_TCONF_UPTS)
        grids = hfx.fused_launch_grids(r.e.h)
    finally:
        comm.close()
        r.close()
    slots = {s for s, _, _ in grids}
    assert 3 in slots and (1 in slots or not int(np.ravel(reg["viscous"])[0])), grids
    return u, div


@pytest.mark.gpu
@pytest.mark.parametrize("family,row", matrix(), ids=["%s-%s" % fr for fr in matrix()])
def test_family_row_vs_oracle(family, row):
    import hfx
    geometry, how, mode, options, must, must_not = FAMILIES[family]
    if (family, row) in REFUSED:
        with pytest.raises(hfx.HfxError):
            run_steps_family(row_registration(geometry, row), mode, options, must, must_not)
        return
    want_u, want_div = oracle_result(geometry, row)
    if row == "inviscid":
        must, must_not = INVISCID_FORM.get(family, (must, must_not))
    if how == "partitioned":
        u, div = partitioned_family(geometry, row, mode)
    else:
        u, div = run_steps_family(row_registration(geometry, row), mode, options, must, must_not)
    eu, ed = relerr(u, want_u), relerr(div, want_div)
    print("%s / %s: state %.3e, residual %.3e" % (family, row, eu, ed))
    assert eu < TOL_U, (family, row, eu, ed)
    assert ed < TOL_DIV, (family, row, eu, ed)
