"""The two-wave form of the affine flux kernel (P4 hexahedra on an affine block, option flux_two_wave): two heavy waves per
workgroup, four workgroups resident per CU, the 22 flux points without a partner lane as an extra pass of one wave, placed by the
host on the local face whose projected viscous flux the block needs least often.  Every case reads from hfx_time_fused_kernels
whether the form ran, and holds the state against the per-method path and against the loader-wave form (flux_two_wave 0) at the
project's bar for one form against another (tests/test_gpu_one_sided_ldg.py, tests/test_gpu_affine_metrics.py); capped grids are
held bit for bit against the uncapped run, a self-partitioned block against the undivided one."""
import ctypes as C
import os

import numpy as np
import pytest

import hfx
import hfx_host as H
import partition_util as PU
from test_gpu_affine_metrics import sheared_xv
from test_gpu_methods_vs_golden import relerr
from test_gpu_one_sided_ldg import WALLS, ldg_switch_flips, needed_points

pytestmark = pytest.mark.gpu

TOL_FORM, TOL_PARTITION = 1e-12, 1e-11
ELEMENT = 1  # slot of the flux kernel in hfx_fused_launch_grids
N_LEFT, N_FACE = 150 - 128, 25  # P4: flux points without a partner lane, flux points of a local face


class _Ctx:
    def __init__(self, h):
        self.h = h


def set_option(case, name, value):
    hfx.Context.set_option(_Ctx(case.handles()[0]), name, value)


def kernel_names(c):
    ctx, e, f, nb = c.handles()
    kt, names = (C.c_double * 8)(), (C.c_char * 256)()
    hfx.check(hfx.lib().hfx_time_fused_kernels(e, f, C.c_int(nb), C.c_int(1), kt, names))
    return names.value.decode().split(",")


def left_over_face(c):
    """(face, need[6]) as the library reports them"""
    ctx, e, f, nb = c.handles()
    face, need = C.c_int(-2), (C.c_long * 6)()
    hfx.check(hfx.lib().hfx_flux_two_wave_face(e, f, C.c_int(nb), C.byref(face), need))
    return face.value, list(need)


def run(n, steps, fused, opts=(), order=4, xv=None, **kw):
    """(state after `steps` steps, kernel names of the stage, launch grids of the last stage, (face, need), the case's tables)"""
    c = H.Case(n, xv=xv, order=order, **kw)
    c.to_device(0)
    for k, v in opts:
        set_option(c, k, v)
    c.run_steps_lib(steps, fused=fused)
    c.sync_host()
    u = c.array("disu_upts0").copy()
    grids = hfx.fused_launch_grids(c.handles()[1]) if fused else []
    face = left_over_face(c) if fused else None
    reg = c.registration() if fused else None
    names = kernel_names(c) if fused else []  # (last: it advances the state)
    c.close()
    return u, names, grids, face, reg


_methods = {}


def methods_state(key, n, steps, **kw):
    """the per-method path's state: computed once per case and left unchanged"""
    if key not in _methods:
        _methods[key] = run(n, steps, False, **kw)[0]
        _methods[key].setflags(write=False)
        c = H.Case(n, **kw)
        assert relerr(_methods[key], c.array("disu_upts0")) > 1e-8  # (the state moved)
        c.close()
    return _methods[key]


def check_forms(key, n, steps, opts=(), **kw):
    """two_wave ran by default and did not with the option off; both against the per-method path and against each other"""
    want = methods_state(key, n, steps, **kw)
    on, names_on, grids, face, reg = run(n, steps, 3, opts, **kw)
    off, names_off, _, face_off, _ = run(n, steps, 3, list(opts) + [("flux_two_wave", 0)], **kw)
    print("%s: kernels %s | %s" % (key, names_on, names_off))
    assert "two_wave" in names_on and "affine_metrics" in names_on
    assert "two_wave" not in names_off and "affine_metrics" in names_off
    assert face[0] in range(6) and face_off[0] == -1
    e_m, e_f = relerr(on, want), relerr(on, off)
    print("%s: two-wave vs per-method %.3g, vs loader-wave form %.3g, loader-wave form vs per-method %.3g" % (key, e_m, e_f, relerr(off, want)))
    assert e_m < TOL_FORM
    assert e_f < TOL_FORM
    return face, reg, grids


def needed_mask(d):
    """needed_points (tests/test_gpu_one_sided_ldg.py) point by point: the flux points whose Fn the stage needs"""
    sz = [int(v) for v in d["sizes"]]
    ne, nfp, nd = sz[0], sz[2], sz[4]
    beta = float(np.ravel(d["ldg_beta"])[0])
    norm = np.asarray(d["norm_fpts"], dtype=np.float64).reshape((nfp * ne, nd), order="F")
    needed = np.ones(nfp * ne, dtype=bool)
    L = np.ravel(d["int2_L"], order="F").astype(np.int64)
    R = np.ravel(d["int2_R"], order="F").astype(np.int64)
    b = np.where(ldg_switch_flips(norm[L]), -beta, beta)
    needed[L] = (0.5 + b) != 0.0
    needed[R] = (0.5 - b) != 0.0
    assert int(needed.sum()) == needed_points(d)[0]
    return needed.reshape((ne, nfp))


def need_per_face(d):
    """elements that take the extra pass with the left-over points on local face f: any of the face's first 22 points needed"""
    m = needed_mask(d)
    return [int(m[:, N_FACE * f:N_FACE * f + N_LEFT].any(axis=1).sum()) for f in range(6)]


BOX = [4, 3, 3]


@pytest.mark.parametrize("beta", [0.5, -0.5])
def test_periodic_box_puts_the_left_over_points_on_a_face_nobody_needs(beta):
    """|beta| = 1/2 on a periodic box: one face of every opposite pair is needed in every element, the other in none; the sign
    of beta exchanges them, and the host's choice follows"""
    kw = dict(amp=0.0, ldg_beta=beta)
    (face, need), reg, _ = check_forms(("box", beta), BOX, 2, **kw)
    want = need_per_face(reg)
    print("beta %+.1f: left-over face %d, need per face %s (numpy %s)" % (beta, face, need, want))
    assert need == want
    assert sorted(want) == [0, 0, 0, 36, 36, 36]
    assert want[face] == min(want) == 0 and face == want.index(0)
    # the same face is needed in every element at the other sign
    other = dict(reg)
    other["ldg_beta"] = np.array([-beta])
    assert need_per_face(other)[face] == 36


def test_every_point_needed_the_extra_pass_always_runs():
    kw = dict(amp=0.0, ldg_beta=0.25, ldg_tau=0.3)
    (face, need), reg, _ = check_forms("box_beta_quarter", BOX, 2, **kw)
    assert need == need_per_face(reg) == [36] * 6 and face == 0


def test_walls_boundary_points_among_the_left_over_points():
    """walls in y: partner word -1 (always needed), the gradient stored at the boundary points"""
    kw = dict(amp=0.0, ldg_beta=0.5, **WALLS)
    (face, need), reg, _ = check_forms("box_walls", BOX, 2, **kw)
    want = need_per_face(reg)
    print("walls: left-over face %d, need per face %s" % (face, need))
    assert need == want and want[face] == min(want) and max(want) > min(want)
    other, _ = check_forms("box_walls_minus", BOX, 2, amp=0.0, ldg_beta=-0.5, **WALLS)[:2]
    assert other[1][other[0]] == min(other[1])


def test_sheared_box_full_metric_tensor():
    n = [4, 4, 4]
    check_forms("sheared", n, 2, xv=sheared_xv(n))


def test_inviscid_run_keeps_the_register_pipeline():
    """(the affine form forms LDG corrections: an inviscid block has none and does not take it)"""
    kw = dict(amp=0.0, viscous=0, ic_form=0)  # (the isentropic vortex: the Taylor-Green state needs the viscous reference values)
    want = methods_state("inviscid", BOX, 2, **kw)
    on, names, _, face, _ = run(BOX, 2, 3, **kw)
    off = run(BOX, 2, 3, [("flux_two_wave", 0)], **kw)[0]
    assert "two_wave" not in names and face[0] == -1
    assert relerr(on, want) < TOL_FORM and relerr(on, off) < TOL_FORM


@pytest.mark.parametrize("order", [3, 5])
def test_other_orders_do_not_take_the_form(order):
    kw = dict(amp=0.0)
    want = methods_state(("order", order), [3, 3, 3], 1, order=order, **kw)
    on, names, _, face, _ = run([3, 3, 3], 1, 3, order=order, **kw)
    off = run([3, 3, 3], 1, 3, [("flux_two_wave", 0)], order=order, **kw)[0]
    print("P%d: %s" % (order, names))
    assert "two_wave" not in names and face[0] == -1
    assert relerr(on, want) < TOL_FORM and relerr(on, off) < TOL_FORM


@pytest.mark.parametrize("cap", [2, 3, 8, 16])
def test_capped_grids_loop_and_agree_bit_for_bit(cap):
    """27 elements on 2, 3, 8 or 16 workgroups: the single state slot's refill, the record's second buffer, the tail iteration and
    (caps 8 and 16, XCD order) workgroups without work show from the second trip on"""
    n, kw = [3, 3, 3], dict(amp=0.0)
    want = methods_state("cube", n, 2, **kw)
    free, names, g0, _, _ = run(n, 2, 3, **kw)
    got, names_c, grids, _, _ = run(n, 2, 3, [("persistent_grid_cap", cap)], **kw)
    off = run(n, 2, 3, [("persistent_grid_cap", cap), ("flux_two_wave", 0)], **kw)[0]
    assert "two_wave" in names and "two_wave" in names_c
    flux0 = [(g, w) for s, g, w in g0 if s == ELEMENT]
    flux = [(g, w) for s, g, w in grids if s == ELEMENT]
    print("cap %d: flux kernel grids %s (uncapped %s)" % (cap, flux, flux0))
    assert flux0 == [(27, 27)] and flux == [(cap, 27)]
    assert -(-27 // cap) >= 2  # trips of the busiest workgroup
    assert np.array_equal(got, free)
    assert relerr(got, want) < TOL_FORM and relerr(got, off) < TOL_FORM


def partitioned_worker(rank, world, port, n_local, cfg, n_steps, outdir):
    """PU.gpu_worker's fused run on the library's own transport, and whether the block's plan is the two-wave form"""
    import torch
    torch.cuda.set_device(0)
    dist = PU.init_pg(rank, world, port, "gloo")
    try:
        cfg, sp = PU.case_kw(cfg)
        c = H.Case(list(n_local), rank=rank, pgrid=[1, 1, 1], self_partition=sp, **cfg)
        c.to_device(0)
        c.set_comm(hfx.comm_unique_id())
        c.run_partitioned(n_steps)
        c.sync_host()
        np.save(os.path.join(outdir, "u_rank%d.npy" % rank), c.array("disu_upts0"))
        grids = hfx.fused_launch_grids(c.handles()[1])
        face, need = left_over_face(c)  # (the block's tables exist: the plan of the stages that ran)
        np.save(os.path.join(outdir, "plan_rank%d.npy" % rank), np.array([face] + need + [g for s, g, w in grids if s == ELEMENT]))
        c.close()
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_self_partitioned_block_equals_the_undivided_one(tmp_path):
    """a block that is its own neighbour in x, y and z: element lists, partition-face points (partner word -1) on every face"""
    n, cfg = [4, 4, 4], dict(order=4, amp=0.0)
    one, names, _, _, _ = run(n, 2, 3, **cfg)
    assert "two_wave" in names
    PU.spawn(partitioned_worker, 1, (n, dict(cfg, self_partition=[1, 1, 1]), 2, str(tmp_path)))
    u = PU.assemble(str(tmp_path), "u", n, [1, 1, 1], one.shape)
    plan = np.load(os.path.join(str(tmp_path), "plan_rank0.npy"))
    print("self-partitioned: left-over face %d, need %s, flux kernel grids %s; vs undivided %.3g" % (plan[0], plan[1:7], plan[7:], relerr(u, one)))
    assert plan[0] in range(6)  # the two-wave form ran on the lists
    assert len(plan[7:]) >= 2   # ... in more than one launch
    assert relerr(u, one) < TOL_PARTITION
