"""Folded faces (option fold_faces, default on): in a viscous run with |ldg_beta| = 1/2 the two-wave flux kernel of P4 hexahedra
forms the common flux of the interior pairs itself -- the flux-point lane whose projected viscous flux has the non-zero weight
writes norm_tconf of both sides -- and the stage launches no face_flux2_kernel on interior faces.  Every case holds the default
run against the run with fold_faces 0 (the three-launch stage) and against the per-method path at the project's bar for one form
against another (1e-12: tests/test_gpu_flux_two_wave.py), prints whether the two forms agree bit for bit, and reads from
hfx_time_fused_kernels whether the form ran: "folded_faces" among the names and 0.0 ms for the face kernel's step when it launched
nothing (with boundary faces the step still launches their kernels: its time is then theirs)."""
import ctypes as C
import os

import numpy as np
import pytest

import hfx
import hfx_host as H
import partition_util as PU
from test_gpu_affine_metrics import sheared_xv
from test_gpu_flux_two_wave import ELEMENT, left_over_face, methods_state, partitioned_worker, set_option
from test_gpu_methods_vs_golden import relerr
from test_gpu_one_sided_ldg import WALLS

pytestmark = pytest.mark.gpu

TOL_FORM, TOL_PARTITION = 1e-12, 1e-11
FACE_STEP = 2  # slot of the common-flux step (face_flux2_kernel) in hfx_time_fused_kernels
BOX = [4, 3, 3]


def stage_times(e, faces, nb):
    """(kernel names, ms[8]) of hfx_time_fused_kernels, one repetition (it advances the state)"""
    kt, names = (C.c_double * 8)(), (C.c_char * 256)()
    hfx.check(hfx.lib().hfx_time_fused_kernels(e, faces, C.c_int(nb), C.c_int(1), kt, names))
    return names.value.decode().split(","), list(kt)


def run(n, steps, opts=(), **kw):
    """(state after `steps` steps of the split stage, kernel names, ms of the stage's steps, (left-over face, need), launch grids)"""
    c = H.Case(n, **kw)
    c.to_device(0)
    for k, v in opts:
        set_option(c, k, v)
    c.run_steps_lib(steps, fused=3)
    c.sync_host()
    u = c.array("disu_upts0").copy()
    grids = hfx.fused_launch_grids(c.handles()[1])
    face = left_over_face(c)
    ctx, e, f, nb = c.handles()
    names, ms = stage_times(e, f, nb)  # (last: it advances the state)
    c.close()
    return u, names, ms, face, grids


def assert_folded(names, ms, launches_nothing=True):
    assert "folded_faces" in names and "two_wave" in names and "face_flux2_kernel" in names, names
    if launches_nothing:
        assert ms[FACE_STEP] == 0.0, ms


def assert_not_folded(names, ms):
    assert "folded_faces" not in names and "face_flux2_kernel" in names, names
    assert ms[FACE_STEP] > 0.0, ms


def check_folded(key, n, steps, opts=(), bdy=False, **kw):
    """the default run folds, fold_faces 0 does not; both against each other and the default against the per-method path"""
    want = methods_state(key, n, steps, **kw)
    on, names_on, ms_on, face, _ = run(n, steps, opts, **kw)
    off, names_off, ms_off, _, _ = run(n, steps, list(opts) + [("fold_faces", 0)], **kw)
    assert_folded(names_on, ms_on, launches_nothing=not bdy)
    assert_not_folded(names_off, ms_off)
    e_f, e_m = relerr(on, off), relerr(on, want)
    print("%s: folded vs three-launch stage %.3g (bit for bit: %s), vs per-method %.3g; face step %.4f ms | %.4f ms; left-over face %s"
          % (key, e_f, np.array_equal(on, off), e_m, ms_on[FACE_STEP], ms_off[FACE_STEP], face))
    assert e_f < TOL_FORM
    assert e_m < TOL_FORM
    return on, face


@pytest.mark.parametrize("beta", [0.5, -0.5])
def test_periodic_box_either_sign_of_beta(beta):
    """the side that folds changes with the sign"""
    check_folded(("box", beta), BOX, 2, amp=0.0, ldg_beta=beta)


@pytest.mark.parametrize("riemann", [0, 3])  # (rusanov, hllc: the rows of tests/test_gpu_physics_matrix.py)
def test_every_riemann_solver_that_folds(riemann):
    check_folded(("box_riemann", riemann), BOX, 2, amp=0.0, riemann_solve_type=riemann)


def test_roem_keeps_the_face_kernel():
    """RoeM (riemann_solve_type 2) is not folded: its FOLD instantiation spilled 34 registers (pow), and folded it missed the
    oracle's residual bound at supersonic face states (1.47e-11 against 1e-11, tests/test_gpu_physics_matrix.py, row roem).  The
    plan keeps the three-launch stage, and the option changes nothing."""
    kw = dict(amp=0.0, riemann_solve_type=2)
    want = methods_state(("box_riemann", 2), BOX, 2, **kw)
    on, names_on, ms_on, _, _ = run(BOX, 2, **kw)
    off, names_off, ms_off, _, _ = run(BOX, 2, [("fold_faces", 0)], **kw)
    assert_not_folded(names_on, ms_on)
    assert_not_folded(names_off, ms_off)
    assert np.array_equal(on, off)
    assert relerr(on, want) < TOL_FORM


def test_two_sided_ldg_keeps_the_face_kernel():
    """beta = 1/4, tau = 0.3: both sides' Fn enter, the plan does not fold and the option changes nothing"""
    kw = dict(amp=0.0, ldg_beta=0.25, ldg_tau=0.3)
    want = methods_state("box_beta_quarter", BOX, 2, **kw)
    on, names_on, ms_on, _, _ = run(BOX, 2, **kw)
    off, names_off, ms_off, _, _ = run(BOX, 2, [("fold_faces", 0)], **kw)
    assert_not_folded(names_on, ms_on)
    assert_not_folded(names_off, ms_off)
    assert np.array_equal(on, off)
    assert relerr(on, want) < TOL_FORM


@pytest.mark.parametrize("beta", [0.5, -0.5])
def test_walls_boundary_points_keep_their_kernels(beta):
    """walls in y: the boundary points store Fn for the boundary kernels (which the common-flux step still launches), the interior
    pairs beside them fold"""
    key = "box_walls" if beta > 0 else "box_walls_minus"
    check_folded(key, BOX, 2, bdy=True, amp=0.0, ldg_beta=beta, **WALLS)


def test_sheared_box_left_normal_is_no_axis():
    n = [4, 4, 4]
    check_folded("sheared", n, 2, xv=sheared_xv(n))


_unforced = {}


@pytest.mark.parametrize("forced", range(6))
def test_left_over_pass_forms_the_common_flux(forced):
    """flux_two_wave_face puts the 22 left-over points on a face of the caller's choice: on three of the six every element needs
    them (the host's own choice is one of the others, and the pass's point physics never runs), and the left-over pass forms the
    pairs' common flux"""
    kw = dict(amp=0.0)
    if "u" not in _unforced:
        _unforced["u"], names, ms, _unforced["face"], _ = run(BOX, 2, **kw)
        _unforced["u"].setflags(write=False)
        assert_folded(names, ms)
    got, names, ms, (face, need), _ = run(BOX, 2, [("flux_two_wave_face", forced)], **kw)
    assert_folded(names, ms)
    free_face, free_need = _unforced["face"]
    print("forced face %d: reported %d, need per face %s (the host's choice: %d); vs the unforced run %.3g (bit for bit: %s)"
          % (forced, face, need, free_face, relerr(got, _unforced["u"]), np.array_equal(got, _unforced["u"])))
    assert face == forced and need == free_need
    assert sorted(need) == [0, 0, 0, 36, 36, 36] and need[free_face] == 0
    assert relerr(got, _unforced["u"]) < TOL_FORM
    want = methods_state(("box", 0.5), BOX, 2, amp=0.0, ldg_beta=0.5)  # (ldg_beta 1/2 is the default)
    assert relerr(got, want) < TOL_FORM


@pytest.mark.parametrize("cap", [2, 3])
def test_capped_grids_fold_on_later_trips_bit_for_bit(cap):
    """27 elements on 2 or 3 workgroups: the second and later trips of the element loop"""
    n, kw = [3, 3, 3], dict(amp=0.0)
    free, names, ms, _, g0 = run(n, 2, **kw)
    got, names_c, ms_c, _, grids = run(n, 2, [("persistent_grid_cap", cap)], **kw)
    assert_folded(names, ms)
    assert_folded(names_c, ms_c)
    flux0 = [(g, w) for s, g, w in g0 if s == ELEMENT]
    flux = [(g, w) for s, g, w in grids if s == ELEMENT]
    print("cap %d: flux kernel grids %s (uncapped %s)" % (cap, flux, flux0))
    assert flux0 == [(27, 27)] and flux == [(cap, 27)]
    assert np.array_equal(got, free)
    assert relerr(got, methods_state("cube", n, 2, **kw)) < TOL_FORM


def test_self_partitioned_block_equals_the_undivided_one(tmp_path):
    """a block that is its own neighbour in x, y and z: element lists, partition-face points (partner word -1: they keep Fn and
    their one-sided kernels) beside interior pairs that fold"""
    n, cfg = [4, 4, 4], dict(order=4, amp=0.0)
    one, names, ms, _, _ = run(n, 2, amp=0.0)
    assert_folded(names, ms)
    PU.spawn(partitioned_worker, 1, (n, dict(cfg, self_partition=[1, 1, 1]), 2, str(tmp_path)))
    u = PU.assemble(str(tmp_path), "u", n, [1, 1, 1], one.shape)
    plan = np.load(os.path.join(str(tmp_path), "plan_rank0.npy"))
    print("self-partitioned: left-over face %d, flux kernel grids %s; vs undivided %.3g" % (plan[0], plan[7:], relerr(u, one)))
    assert plan[0] in range(6) and len(plan[7:]) >= 2  # the two-wave form ran on the lists, in more than one launch
    assert relerr(u, one) < TOL_PARTITION


def run_registration(reg, options=()):
    """(state, kernel names, ms) after EO.STEPS steps of the split stage on a registration (tests/test_gpu_element_orientation.py)"""
    import test_element_orientation as EO
    from test_gpu_methods_vs_golden import build
    ctx = hfx.Context(0)
    e, faces = None, []
    try:
        ctx.set_fused_mode(3)
        for k, v in options:
            ctx.set_option(k, v)
        e, faces = build(ctx, reg)
        hfx.run_steps(e, faces, EO.STEPS, fused=3)
        u = e.download(hfx.DISU_UPTS0)
        assert e.check_nan() == -1
        names, ms = stage_times(e.h, hfx._face_array(faces), len(faces))
        return u, names, ms
    finally:
        for f in faces:
            f.close()
        if e is not None:
            e.close()
        ctx.close()


def test_mixed_orientation_partner_is_no_mirror_point():
    """every element of the box turned its own way (tests/reorient.py): the partner point's number is not the mirror of the own,
    and the left normal is the partner's"""
    import test_element_orientation as EO
    reg = EO.registration("hex_p4_box", "hllc_beta_plus", True)
    on, names_on, ms_on = run_registration(reg)
    off, names_off, ms_off = run_registration(reg, (("fold_faces", 0),))
    assert_folded(names_on, ms_on)
    assert_not_folded(names_off, ms_off)
    print("mixed orientation: folded vs three-launch stage %.3g (bit for bit: %s)" % (relerr(on, off), np.array_equal(on, off)))
    assert relerr(on, off) < TOL_FORM
