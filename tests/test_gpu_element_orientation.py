"""Every kernel form of the tensor-element path on blocks of MIXED element orientation (tests/reorient.py), raw C ABI.

A box of the host mirror numbers all its cells alike; tests/test_element_orientation.py states what that hides from the kernels and
proves, on the oracle, the transform that re-orients every element.  Here each kernel family runs the re-oriented registration for
two time steps and is held to

    1e-11 on disu_upts0 and on div_tconf_upts against the oracle on the SAME registration (the bar of test_gpu_physics_matrix.py),
    1e-12 on disu_upts0 against the device run of the un-oriented registration, mapped back to its point order (the project's bar
    for one form against another: tests/test_gpu_flux_two_wave.py, tests/test_gpu_one_sided_ldg.py),

and reads from hfx_time_fused_kernels / hfx_fused_launch_grids that its kernel form ran.  The partition-face cases cut the
re-oriented 4 x 4 x 4 box of tests/test_partition_ragged.py and keep that module's tolerances against the undivided oracle."""
import ctypes as C

import numpy as np
import pytest

import ragged_partition as RP
import reorient as RO
import test_element_orientation as EO
from test_gpu_physics_matrix import kernel_names

pytestmark = pytest.mark.gpu

TOL_U = TOL_DIV = 1e-11
TOL_FORM = 1e-12
ELEMENT = 1  # slot of the flux kernel in hfx_fused_launch_grids
V, INV = EO.VISCOUS_ROWS, ["rusanov_inviscid"]
SGS_LAUNCHES = "sgsf_upts_kernel + ell_apply_kernel (SGS flux)"

# family -> (geometry, fused mode, options, names hfx_time_fused_kernels must / must not report, rows)
FAMILIES = {
    "methods_hex_p2": ("hex_p2", 0, (), (), (), V + INV + ["wale"]),
    "methods_quad_p3": ("quad_p3", 0, (), (), (), V + INV),
    "split2_hex_p2": ("hex_p2", 2, (), ("split_gradient_kernel", "face_flux_kernel"), (), V + INV),
    "split3_hex_p2": ("hex_p2", 3, (), ("split_flux_kernel", "face_flux2_kernel"), (), V + INV),  # (dictionary rows)
    "split2_hex_p4": ("hex_p4", 2, (), ("split_gradient_kernel", "face_flux_kernel"), (), V + INV),
    "split3_hex_p4": ("hex_p4", 3, (), ("split_flux_tensor_kernel", "face_flux2_kernel"), ("affine_metrics", "affine_block"), V + INV),
    "split2_quad_p3": ("quad_p3", 2, (), ("split_gradient_kernel", "face_flux_kernel"), (), V + INV),
    "split3_quad_p3": ("quad_p3", 3, (), ("split_flux_tensor_kernel", "face_flux2_kernel"), (), V + INV),
    "split2_quad_p7": ("quad_p7", 2, (), ("split_gradient_kernel", "face_flux_kernel"), (), V + INV),
    "split3_quad_p7": ("quad_p7", 3, (), ("face_flux2_kernel",), (), V + INV),
    # 343 points per element: a request for variant 3 runs variant 2 with the wide operator rows (tests/test_gpu_fused_high_order.py)
    "split_hex_p6_wide_rows": ("hex_p6", 3, (), ("split_gradient_kernel", "face_flux_kernel"), ("face_flux2_kernel",), ["hllc_beta_plus"]),
    "walls_split2": ("walls", 2, (), ("split_gradient_kernel", "face_flux_kernel"), (), V),
    "walls_split3": ("walls", 3, (), ("face_flux2_kernel",), (), V),
    # the closure in the flux kernel (variant 3 stays), and variant 2 with the SGS flux from launches of its own
    "wale_split3_hex_p4": ("hex_p4", 3, (), ("split_flux_tensor_kernel", "face_flux2_kernel"), (SGS_LAUNCHES,), ["wale"]),
    "wale_split2_hex_p4": ("hex_p4", 2, (), ("split_gradient_kernel", "face_flux_kernel", SGS_LAUNCHES), (), ["wale"]),
}
# the affine block: every element's metrics are one signed, permuted (box) or full (sheared) matrix of its own
for _g in ("hex_p4_box", "hex_p4_sheared"):
    FAMILIES["two_wave_" + _g] = (_g, 3, (), ("face_flux2_kernel", "affine_metrics", "two_wave"), (), V + INV)
    FAMILIES["loader_wave_" + _g] = (_g, 3, (("flux_two_wave", 0),), ("face_flux2_kernel", "affine_metrics"), ("two_wave",), V)
    FAMILIES["general_metrics_" + _g] = (_g, 3, (("affine_metrics", 0),), ("face_flux2_kernel", "affine_block"), ("affine_metrics", "two_wave"), V)
# an inviscid block forms no LDG corrections and does not take the affine form (csrc/fused_hex.hip, split_plan): found affine, it
# keeps the per-point metrics
INVISCID_FORM = (("face_flux2_kernel", "affine_block"), ("affine_metrics", "two_wave"))


def matrix():
    return [(f, r) for f in FAMILIES for r in FAMILIES[f][5]]


def run_block(reg, mode, options=(), must=(), must_not=(), two_wave_face=False):
    """(u, div, kernel names, launch grids, (face, need) of hfx_flux_two_wave_face) after EO.STEPS steps of hfx_run_steps"""
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
        hfx.run_steps(e, faces, EO.STEPS, fused=mode)
        u, div = e.download(hfx.DISU_UPTS0), e.download(hfx.DIV_TCONF_UPTS)
        assert e.check_nan() == -1
        grids = hfx.fused_launch_grids(e.h)
        names, lowest = [], None
        if mode in (2, 3):
            # the split stage's persistent kernels ran: update / residual, and on a viscous run flux / gradient
            slots = {s for s, _, _ in grids}
            assert 3 in slots and (1 in slots or not int(np.ravel(reg["viscous"])[0])), grids
            if two_wave_face:
                face, need = C.c_int(-2), (C.c_long * 6)()
                hfx.check(hfx.lib().hfx_flux_two_wave_face(e.h, hfx._face_array(faces), C.c_int(len(faces)), C.byref(face), need))
                lowest = (face.value, list(need))
            names = kernel_names(e, faces)  # (last: it advances the state)
            for n in must:
                assert n in names, (n, names)
            for n in must_not:
                assert n not in names, (n, names)
        else:
            assert grids == [], grids  # no split fused stage ran on this block
        return u, div, names, grids, lowest
    finally:
        for f in faces:
            f.close()
        if e is not None:
            e.close()
        ctx.close()


_plain = {}


def plain_state(family, row):
    """the device's state on the un-oriented registration, the same family and row: computed once, left unchanged"""
    if (family, row) not in _plain:
        geometry, mode, options = FAMILIES[family][:3]
        u = run_block(EO.registration(geometry, row, False), mode, options)[0]
        u.setflags(write=False)
        _plain[(family, row)] = u
    return _plain[(family, row)]


def check(family, row, u, div, names):
    geometry = FAMILIES[family][0]
    want_u, want_div = EO.oracle_result(geometry, row, True)
    eu, ed = EO.relerr(u, want_u), EO.relerr(div, want_div)
    ef = EO.relerr(RO.back(u, EO.rot_of(geometry)), plain_state(family, row))
    print("%s / %s: kernels %s; against the oracle: state %.3e, residual %.3e; against the un-oriented block on the device: state %.3e"
          % (family, row, ",".join(names) if names else "per-method path", eu, ed, ef))
    assert eu < TOL_U and ed < TOL_DIV, (family, row, eu, ed)
    assert ef < TOL_FORM, (family, row, ef)


@pytest.mark.parametrize("family,row", matrix(), ids=["%s-%s" % fr for fr in matrix()])
def test_family_on_elements_of_mixed_orientation(family, row):
    geometry, mode, options, must, must_not, _ = FAMILIES[family]
    affine = geometry in ("hex_p4_box", "hex_p4_sheared")
    if affine and row in INV:
        must, must_not = INVISCID_FORM
    reg = EO.registration(geometry, row, True)
    u, div, names, grids, lowest = run_block(reg, mode, options, must, must_not, two_wave_face=affine)
    if affine:
        # (whatever form ran, the block was detected affine)
        assert "affine_metrics" in names or "affine_block" in names, names
    if "two_wave" in names:
        from test_gpu_flux_two_wave import need_per_face
        face, need = lowest
        ne, beta = int(reg["sizes"][0]), float(np.ravel(reg["ldg_beta"])[0])
        print("%s / %s: left-over face %d, need per face %s of %d elements" % (family, row, face, need, ne))
        assert need == need_per_face(reg)
        assert face == need.index(min(need))
        if abs(beta) == 0.5:
            assert all(0 < v < ne for v in need), need
        else:
            assert need == [ne] * 6
    elif affine:
        assert lowest[0] == -1
    check(family, row, u, div, names)


@pytest.mark.parametrize("cap", [2, 3])
@pytest.mark.parametrize("options", [(), (("flux_two_wave", 0),)], ids=["two_wave", "loader_wave"])
def test_capped_grids_carry_the_record_between_orientations(options, cap):
    """27 elements on 2 or 3 workgroups: the metric record and the partner data of the next element travel through the software
    pipeline while the current one, of another orientation, is computed.  Bit for bit the uncapped run."""
    reg = EO.registration("hex_p4_box", "hllc_beta_plus", True)
    must = ("affine_metrics",) + (() if options else ("two_wave",))
    free, _, names, g0, _ = run_block(reg, 3, options, must)
    got, div, _, grids, _ = run_block(reg, 3, tuple(options) + (("persistent_grid_cap", cap),), must)
    flux0, flux = [(g, w) for s, g, w in g0 if s == ELEMENT], [(g, w) for s, g, w in grids if s == ELEMENT]
    print("cap %d %s: flux kernel grids %s (uncapped %s)" % (cap, names, flux, flux0))
    assert flux0 == [(27, 27)] and flux == [(cap, 27)]
    assert np.array_equal(got, free)
    family = "two_wave_hex_p4_box" if not options else "loader_wave_hex_p4_box"
    check(family, "hllc_beta_plus", got, div, names)


# ---- partition faces between elements of different orientation -------------------------------------------------------------------

PART_TOL_U, PART_TOL_DIV = 1e-11, 5e-10  # tests/test_partition_ragged.py, TOL_U / TOL_DIV


def ragged_oracle():
    def make():
        u, div = RP.undivided_oracle(EO.ragged_registration(True)[0], EO.STEPS)
        u, div = u.copy(), div.copy()
        u.setflags(write=False)
        div.setflags(write=False)
        return u, div
    return EO.cached(("ragged", "oracle"), make)


def check_partitioned(what, u, div):
    u1, div1 = ragged_oracle()
    eu, ed = EO.relerr(u, u1), EO.relerr(div, div1)
    print("%s: against the undivided oracle: state %.3e, residual %.3e" % (what, eu, ed))
    assert eu < PART_TOL_U and ed < PART_TOL_DIV


@pytest.mark.parametrize("mode", ["fused", "fused2", "methods"])
@pytest.mark.parametrize("name", ["ragged4", "ragged6"])
def test_ragged_cuts_of_the_re_oriented_box(name, mode):
    """hfx_stage_partitioned / the per-method entry points in lockstep: the in-face order of a partition face is Rlut's alone"""
    import test_partition_ragged as TR
    reg = EO.ragged_registration(True)[0]
    parts = RP.cut(reg, TR.part_vector(name))
    out, grids = RP.gpu_lockstep(RP.part_tables(parts), EO.STEPS, mode)
    shape = ragged_oracle()[0].shape
    if mode != "methods":
        assert all(g and {s for s, _, _ in g} == {1, 3} for g in grids), grids  # flux / gradient kernel, update / residual kernel
    print("%s %s: launch grids %s" % (name, mode, grids))
    check_partitioned("%s %s" % (name, mode), RP.assemble(parts, [o[0] for o in out], shape), RP.assemble(parts, [o[1] for o in out], shape))


@pytest.mark.parametrize("fused_mode", [3, 2])
def test_rccl_cut_self_of_the_re_oriented_box(fused_mode):
    """hfx_run_steps_partitioned over the library's RCCL transport: one rank, three virtual parts, element lists"""
    import hfx
    import test_partition_ragged as TR
    reg = EO.ragged_registration(True)[0]
    d, L, Rlut, seg = RP.cut_self(reg, TR.part_vector(TR.VIRTUAL3))
    assert len(seg) == 6 and len({EO.in_face_map(Rlut[:, i], 3) for i in range(L.shape[1])}) >= 4
    r = RP.GpuPart(d, L, Rlut, seg, fused_mode=fused_mode)
    comm = hfx.Comm(r.ctx.h, hfx.comm_unique_id(), 1, 0)
    try:
        fi = (C.c_void_p * len(r.ints))(*[f.h for f in r.ints])
        fm = (C.c_void_p * 1)(r.m.h)
        hfx.check(hfx.lib().hfx_run_steps_partitioned(r.e.h, fi, C.c_int(len(r.ints)), fm, C.c_int(1), comm.h, C.c_int(EO.STEPS)))
        r.ctx.synchronize()
        u, div = r.e.download(hfx.DISU_UPTS0), r.e.download(hfx.DIV_TCONF_UPTS)
        grids = hfx.fused_launch_grids(r.e.h)
    finally:
        comm.close()
        r.close()
    print("fused mode %d: launch grids %s" % (fused_mode, grids))
    assert {s for s, _, _ in grids} == {1, 3}, grids
    check_partitioned("cut_self, fused mode %d" % fused_mode, u, div)
