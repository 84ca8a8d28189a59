"""One-sided LDG on the split fused stage.  With |ldg_beta| = 1/2 (the reference's default) one of the two weights 1/2 +- beta of
every interior pair is exactly 0.0: the common viscous flux is the projected flux Fn of ONE side.  The flux kernel that knows its
points' partners stores no Fn whose weight is zero, the pairwise kernels load the needed side alone, and the update kernel of a
low-storage scheme does not read the RK register in a stage whose RK_a is 0.0.  None of it may change a result: the fused stage
(called directly and through the deferred call sequence) is held against the per-method path, which computes every flux from the
gradients of both sides, within what tests/test_gpu_fused.py grants the fused stage against that path -- at beta = +-1/2, at a
beta that needs both sides, with boundary points, partition-face points and an LES closure in the flux kernel -- and the count of
needed points that hfx_fused_kernel_bytes reports is rebuilt from the face tables and the LDG switch in numpy."""
import ctypes as C
import os

import numpy as np
import pytest

import hfx
import hfx_host as H
import partition_util as PU
from test_gpu_deferred import calc_residual_calls, tag
from test_gpu_methods_vs_golden import GOLDEN, build, relerr

pytestmark = pytest.mark.gpu

# tests/test_gpu_fused.py: the fused stage against the per-method path (test_fused_public_arrays_after_a_step,
# test_fused_quads_vs_methods, test_split_paths_every_order_vs_methods); tests/test_gpu_partition.py: a partitioned run against the
# undivided one
TOL_FUSED, TOL_PARTITION = 1e-12, 1e-11


def fixture(name, **over):
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    for k, v in over.items():
        d[k] = np.array([v], dtype=np.float64)
    return d


def run_fixture(d, how, steps=1):
    """the state after `steps` time steps: how = "methods" (hfx_run_steps, one launch per reference method), "fused" (hfx_run_steps,
    fused 3) or "deferred" (the reference's call sequence, every stage a whole record)"""
    ctx = hfx.Context(0)
    if how == "deferred":
        ctx.set_option("deferred", 1)
    e, faces = build(ctx, d)
    if how == "deferred":
        tag(e, d)
        nstage, adv = int(d["sizes"][7]), int(np.ravel(d["adv_type"])[0])
        viscous = bool(int(np.ravel(d["viscous"])[0]))
        for _ in range(steps):
            for rk in range(nstage):
                calc_residual_calls([e], faces, viscous, rk)
                e.AdvanceSolution(rk, adv)
        u = e.download(hfx.DISU_UPTS0)
        nf, nr, why = ctx.deferred_stats()
        assert nf == steps * nstage and nr == 0, why  # (every stage ran as the fused stage)
    else:
        hfx.run_steps(e, faces, steps, fused=3 if how == "fused" else False)
        u = e.download(hfx.DISU_UPTS0)
    assert e.check_nan() == -1
    for f in faces:
        f.close()
    e.close()
    ctx.close()
    return u


_methods = {}


def methods_state(name, **over):
    """the per-method path's state, computed once per fixture and parameter set and left unchanged"""
    key = (name, tuple(sorted(over.items())))
    if key not in _methods:
        _methods[key] = run_fixture(fixture(name, **over), "methods")
        _methods[key].setflags(write=False)
    return _methods[key]


def check_fixture(name, hows=("fused",), **over):
    want = methods_state(name, **over)
    assert relerr(want, fixture(name)["u_init"]) > 1e-8  # (the state moved)
    for how in hows:
        err = relerr(run_fixture(fixture(name, **over), how), want)
        print("%s %s %s: %.3g against the per-method path" % (name, over, how, err))
        assert err < TOL_FUSED, (name, how)


@pytest.mark.parametrize("name", ["hex_p2_n3_deformed", "quad_p3_vortex", "quad_p3_integrals"])
def test_parity_at_the_default_beta(name):
    """beta = 1/2, the fixtures' default: a deformed hex mesh whose normals make the switch bit differ between faces, the inviscid
    2-D vortex (every path as before) and a viscous 2-D fixture; the stage called directly and through the deferred calls"""
    check_fixture(name, hows=("fused", "deferred"))


def test_negative_beta_flips_the_needed_side():
    check_fixture("hex_p2_n3_deformed", hows=("fused", "deferred"), ldg_beta=-0.5)


def test_every_point_needed_at_another_beta():
    """beta = 0.25, tau = 0.3: both weights are non-zero, every Fn is written and both sides are read"""
    d = fixture("hex_p1_ldg_tau")
    assert float(np.ravel(d["ldg_beta"])[0]) == 0.25 and float(np.ravel(d["ldg_tau"])[0]) == 0.3
    check_fixture("hex_p1_ldg_tau", hows=("fused", "deferred"))


def test_boundary_points_are_always_needed():
    check_fixture("hex_p2_bdy_walls")
    check_fixture("hex_p2_bdy_walls", ldg_beta=-0.5)


def test_les_closure_in_the_flux_kernel():
    """(the LES form of the flux kernel parks the viscous part of Fn and stores the sum behind its last phase)"""
    check_fixture("hex_p2_les_wale")


def test_partition_face_points_are_always_needed(tmp_path):
    """a block that is its own neighbour in x, y and z: every wrap-around point's Fn is packed and exchanged"""
    n = [4, 4, 4]
    cfg = dict(order=2, amp=0.05, riemann_solve_type=3)
    one = H.Case(n, **cfg)
    one.to_device(0)
    one.run_steps_lib(2, fused=3)
    one.sync_host()
    u1 = one.array("disu_upts0").copy()
    one.close()
    PU.spawn(PU.gpu_worker, 1, (n, [1, 1, 1], dict(cfg, self_partition=[1, 1, 1]), 2, str(tmp_path), "fused", "gloo", "rccl"))
    u = PU.assemble(str(tmp_path), "u", n, [1, 1, 1], u1.shape)
    err = relerr(u, u1)
    print("self-partitioned against undivided: %.3g" % err)
    assert err < TOL_PARTITION


WALLS = dict(bcs=[dict(type="isotherm_wall", T_static=310.0, u=3.0), dict(type="adiabat_wall", v=-2.0)], sides={"y-": 0, "y+": 1})


@pytest.mark.parametrize("order,kw", [(4, dict(ldg_beta=0.5)), (4, dict(ldg_beta=-0.5)), (2, dict(ldg_beta=0.5)), (4, dict(ldg_beta=0.5, **WALLS)),
                                      (4, dict(ldg_beta=0.25, ldg_tau=0.3))])
def test_affine_block_stores_only_the_needed_flux(order, kw):
    """The affine form of the flux kernel is the one that leaves the unneeded Fn unwritten and lets a wave without solution points
    (P4 hexes: flux points 128..149, all on one face) pass its flux-point physics when none of them is needed: periodic boxes at
    both signs of beta, walls in y (boundary points between interior ones), and a beta that needs every point."""
    n, out = [4, 3, 3], {}
    for fused in (False, 3):
        c = H.Case(n, order=order, amp=0.0, **kw)
        c.to_device(0)
        c.run_steps_lib(2, fused=fused)
        c.sync_host()
        out[fused] = c.array("disu_upts0").copy()
        if fused:
            names = (C.c_char * 256)()
            ms = (C.c_double * 8)()
            ctx, e, f, nb = c.handles()
            hfx.check(hfx.lib().hfx_time_fused_kernels(e, f, C.c_int(nb), C.c_int(1), ms, names))
            print("kernels:", names.value.decode())
            if order == 4 and "bcs" not in kw:  # (P2 on computed nodes: operators not bit-exactly tensor-product, dictionary rows)
                assert "affine_metrics" in names.value.decode()
        c.close()
    err = relerr(out[3], out[False])
    print("affine P%d %s: %.3g against the per-method path" % (order, {k: v for k, v in kw.items() if k.startswith("ldg")}, err))
    assert err < TOL_FUSED


def ldg_switch_flips(n):
    """the sign decision of inters::calc_ldg_switch on the left normals n (points, n_dims): exact zero tests"""
    s1 = n[:, 0] + n[:, 1]
    flip = (n[:, 0] < 0.0) | ((n[:, 0] == 0.0) & (s1 < 0.0))
    if n.shape[1] == 3:
        flip |= (n[:, 0] == 0.0) & (s1 == 0.0) & ((n[:, 0] + n[:, 2]) < 0.0)
    return flip


def needed_points(d):
    """(flux points whose Fn the stage needs, interior flux points, all flux points) from the fixture's face tables, normals and beta"""
    sz = [int(v) for v in d["sizes"]]
    ne, nfp, nd = sz[0], sz[2], sz[4]
    plane = nfp * ne
    beta = float(np.ravel(d["ldg_beta"])[0])
    viscous = bool(int(np.ravel(d["viscous"])[0]))
    norm = np.asarray(d["norm_fpts"], dtype=np.float64).reshape((plane, nd), order="F")
    needed = np.ones(plane, dtype=bool)  # boundary and partition-face points: always
    interior = 0
    for t in range(3):
        if "int%d_L" % t not in d:
            continue
        L = np.ravel(d["int%d_L" % t], order="F").astype(np.int64)
        R = np.ravel(d["int%d_R" % t], order="F").astype(np.int64)
        interior += 2 * L.size
        if not viscous or nd == 2:  # (quads: the 2-D stage writes and reads both sides, as before)
            continue
        b = np.where(ldg_switch_flips(norm[L]), -beta, beta)
        needed[L] = (0.5 + b) != 0.0
        needed[R] = (0.5 - b) != 0.0
    return int(needed.sum()), interior, plane


@pytest.mark.parametrize("name,over", [("hex_p2_n3_deformed", {}), ("hex_p2_n3_deformed", {"ldg_beta": -0.5}), ("quad_p3_integrals", {}),
                                       ("hex_p2_bdy_walls", {}), ("hex_p1_ldg_tau", {}), ("quad_p3_vortex", {})])
def test_needed_point_count(name, over):
    d = fixture(name, **over)
    want, interior, plane = needed_points(d)
    beta, viscous = float(np.ravel(d["ldg_beta"])[0]), bool(int(np.ravel(d["viscous"])[0]))
    if viscous and abs(beta) == 0.5 and int(d["sizes"][4]) == 3:
        assert want == interior // 2 + (plane - interior)
        if "bdy" not in name:
            assert interior == plane and want == plane // 2  # (periodic)
    else:
        assert want == plane  # beta = 0.25, and the quads
    ctx = hfx.Context(0)
    e, faces = build(ctx, d)
    hfx.run_steps(e, faces, 1, fused=3)  # builds the block's fused tables
    b = (C.c_double * 8)()
    hfx.check(hfx.lib().hfx_fused_kernel_bytes(e.h, b))
    print("%s %s: %d of %d flux points needed, libhfx reports %g, %g bytes per stage not moved" % (name, over, want, plane, b[5], b[6]))
    assert b[5] == want
    # (the face kernel's reads, and the flux kernel's writes where it knows its points' partners)
    idle_bytes = 8.0 * int(d["sizes"][3]) * (plane - want)
    assert b[6] in (idle_bytes, 2.0 * idle_bytes)
    for f in faces:
        f.close()
    e.close()
    ctx.close()


def test_low_storage_first_stage_does_not_need_the_register():
    """RK45 (adv_type 3), two full steps: the second step's first stage is entered with a used register and RK_a = 0.0"""
    out = {}
    for fused in (False, 3):
        c = H.Case([3, 3, 3], order=2, amp=0.1, adv_type=3)
        assert c.params().RK_a[0] == 0.0 and c.params().RK_a[1] != 0.0
        c.to_device(0)
        c.run_steps_lib(2, fused=fused)
        c.sync_host()
        out[fused] = c.array("disu_upts0").copy()
        c.close()
    err = relerr(out[3], out[False])
    print("RK45, two steps, fused 3 against the per-method path: %.3g" % err)
    assert err < TOL_FUSED
