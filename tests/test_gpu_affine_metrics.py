"""Affine element blocks (every element a parallelepiped) on the split fused stage: the detection when the fused tables are
made, the per-element metric record in place of the per-point metric arrays (option affine_metrics, default 1), and what
hfx_fused_kernel_bytes prices.  The bound of the detection is restated here in numpy and held against the host mirror's
metrics without a GPU; the GPU tests read the block's form from the names hfx_time_fused_kernels returns."""
import ctypes as C
import os

import numpy as np
import pytest

import hfx
import hfx_host as H
import partition_util as PU
from test_gpu_methods_vs_golden import build, relerr, GOLDEN

gpu = pytest.mark.gpu

# csrc/fused_hex.hip, affine_detect: tol = AFFINE_C eps (1 + (block volume / element volume)^(1/n_dims))
AFFINE_C = 1024.0
EPS = np.finfo(np.float64).eps
# what test_gpu_fused.py grants the fused stage against the per-method path (test_split_paths_every_order_vs_methods,
# test_fused_full_size_conservation, test_split3_variant_knobs_agree), and test_gpu_partition.py a partitioned run
TOL_FUSED, TOL_PARTITION = 1e-12, 1e-11
SHEAR = np.array([[1.0, 1.0, 0.0], [0.0, 1.0, 1.0], [0.0, 0.0, 1.0]])  # x + y, y + z, z: periodic images stay a period apart


def spread_and_tol(m):
    """(largest spread of an element's metrics about its representative, in units of the representative's scale) and the
    detection's bound, per element.  m: JGinv_upts (nd, nd, nu, ne), detjac_upts (nu, ne), JGinv_fpts (nd, nd, nfp, ne),
    detjac_fpts, tdA_fpts (nfp, ne), norm_fpts (nfp, ne, nd)"""
    ju, du, jf, df = m["JGinv_upts"], m["detjac_upts"], m["JGinv_fpts"], m["detjac_fpts"]
    td, nr = m["tdA_fpts"], m["norm_fpts"]
    nd = ju.shape[0]
    nfp, ne = td.shape
    npf = nfp // (2 * nd)
    jr, dr = ju[:, :, :1, :], du[:1, :]
    sj = np.abs(jr).max(axis=(0, 1, 2))
    w = np.abs(ju - jr).max(axis=(0, 1, 2)) / sj
    w = np.maximum(w, np.abs(jf - jr).max(axis=(0, 1, 2)) / sj)
    w = np.maximum(w, np.abs(du - dr).max(axis=0) / np.abs(dr[0]))
    w = np.maximum(w, np.abs(df - dr).max(axis=0) / np.abs(dr[0]))
    tf = td.reshape(2 * nd, npf, ne)
    w = np.maximum(w, (np.abs(tf - tf[:, :1, :]) / tf[:, :1, :]).max(axis=(0, 1)))
    nf = nr.reshape(2 * nd, npf, ne, nd)
    w = np.maximum(w, np.abs(nf - nf[:, :1]).max(axis=(0, 1, 3)))
    vol = np.abs(dr[0]).sum()
    tol = AFFINE_C * EPS * (1.0 + (vol / np.abs(dr[0])) ** (1.0 / nd))
    return w, tol


def metrics_of(case):
    return {k: case.array(k) for k in ("JGinv_upts", "detjac_upts", "JGinv_fpts", "detjac_fpts", "tdA_fpts", "norm_fpts")}


def fixture_metrics(name):
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    sz = [int(v) for v in d["sizes"]]
    ne, nu, nfp, nd = sz[0], sz[1], sz[2], sz[4]
    F = lambda k, shp: np.asarray(d[k], dtype=np.float64).reshape(shp, order="F")
    return {"JGinv_upts": F("JGinv_upts", (nd, nd, nu, ne)), "detjac_upts": F("detjac_upts", (nu, ne)),
            "JGinv_fpts": F("JGinv_fpts", (nd, nd, nfp, ne)), "detjac_fpts": F("detjac_fpts", (nfp, ne)),
            "tdA_fpts": F("tdA_fpts", (nfp, ne)), "norm_fpts": F("norm_fpts", (nfp, ne, nd))}


def box_xv(n, dims=3):
    """the box mesh's own vertices (hfx_host.h: xv[v + nv d], v = ix + (nx+1) (iy + (ny+1) iz))"""
    L = 6.2831853071795862
    idx = np.indices([k + 1 for k in n[:dims]][::-1])[::-1]
    return np.stack([L * (idx[d].ravel() / n[d]) for d in range(dims)], axis=1)


def sheared_xv(n, dims=3):
    return np.asfortranarray(box_xv(n, dims) @ SHEAR[:dims, :dims].T)


def displaced_xv(n):
    xv = np.asfortranarray(box_xv(n))
    xv[1 + (n[0] + 1) * (1 + (n[1] + 1) * 1), 0] += 0.05  # an interior vertex
    return xv


# ---- the bound, without a GPU -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,order", [(4, 1), (4, 4), (6, 2), (6, 5), (8, 4), (16, 4), (32, 4)])
def test_box_meshes_pass_the_bound_with_a_factor_4_to_spare(n, order):
    nodes = np.load(os.path.join(GOLDEN, "hex_p4_n32_tgv.npz"))["loc_1d_upts"] if order == 4 else None
    c = H.Case(n, order=order, loc_1d_upts=nodes)
    w, tol = spread_and_tol(metrics_of(c))
    c.close()
    print("box %d^3 P%d: largest spread %.3g, bound %.3g, margin %.3g" % (n, order, w.max(), tol.min(), (tol / np.maximum(w, 1e-300)).min()))
    assert np.all(4.0 * w <= tol)


def test_sheared_box_passes_the_bound():
    c = H.Case([4, 4, 4], xv=sheared_xv([4, 4, 4]), order=3)
    m = metrics_of(c)
    c.close()
    w, tol = spread_and_tol(m)
    print("sheared 4^3 P3: largest spread %.3g, bound %.3g" % (w.max(), tol.min()))
    assert np.all(4.0 * w <= tol)
    assert np.abs(m["JGinv_upts"][0, 1]).max() > 0.1 * np.abs(m["JGinv_upts"]).max()  # (the map is not diagonal)


@pytest.mark.parametrize("name", ["hex_p2_n3_deformed", "hex_p4_jet"])
def test_deformed_fixtures_fail_the_bound_by_orders_of_magnitude(name):
    w, tol = spread_and_tol(fixture_metrics(name))
    print("%s: largest spread %.3g, bound %.3g" % (name, w.max(), tol.max()))
    assert w.max() > 1e6 * tol.max()


def test_quad_p7_deformed_is_a_mesh_of_parallelograms():
    """The 2-D deformation of the fixtures moves x by a function of y and y by a function of x: every straight-sided quad of
    such a mesh is a parallelogram, so this "deformed" fixture IS affine element by element (measured: largest spread 8.1e-16
    against a bound of 9.1e-13; its detjac differs from element to element by 1.2e-2).  The detection must say so."""
    w, tol = spread_and_tol(fixture_metrics("quad_p7_deformed"))
    d = np.load(os.path.join(GOLDEN, "quad_p7_deformed.npz"))
    print("quad_p7_deformed: largest spread %.3g, bound %.3g" % (w.max(), tol.min()))
    assert np.all(4.0 * w <= tol)
    assert np.ptp(d["detjac_upts"]) > 1e-3


def test_one_displaced_vertex_fails_the_bound():
    c = H.Case([4, 4, 4], xv=displaced_xv([4, 4, 4]), order=2)
    w, tol = spread_and_tol(metrics_of(c))
    c.close()
    assert (w > 1e6 * tol).sum() == 8 and (4.0 * w <= tol).sum() == 64 - 8  # the vertex's eight elements


# ---- on the GPU ---------------------------------------------------------------------------------------------------------

class _Ctx:
    def __init__(self, h):
        self.h = h


def set_option(case, name, value):
    hfx.Context.set_option(_Ctx(case.handles()[0]), name, value)


def kernel_names(e, faces, nb):
    kt, names = (C.c_double * 8)(), (C.c_char * 256)()
    hfx.check(hfx.lib().hfx_time_fused_kernels(e, faces, C.c_int(nb), C.c_int(1), kt, names))
    return names.value.decode().split(",")


def case_is_affine(c, form=True):
    """form: the stage runs the affine form of its kernels ("affine_metrics" among the names); else: the block was found affine,
    whether its kernels have an affine form or not (then "affine_block": P5 hexes do not take the loader wave)"""
    ctx, e, f, nb = c.handles()
    names = kernel_names(e, f, nb)
    return "affine_metrics" in names or (not form and "affine_block" in names)


@gpu
@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("n", [4, 6])
def test_detection_box_is_affine(n, order):
    # (P4 with the benchmark's solution points, as bench.py builds the case)
    nodes = np.load(os.path.join(GOLDEN, "hex_p4_n32_tgv.npz"))["loc_1d_upts"] if order == 4 else None
    c = H.Case(n, order=order, loc_1d_upts=nodes)
    c.to_device(0)
    assert case_is_affine(c, form=False)
    # the affine form belongs to the loader-wave form of the sum-factorised flux kernel: P5 hexes do not take the loader wave, and
    # operators that are not bit-exactly tensor products run the dictionary-row kernel -- those keep the per-point metrics
    ctx, e, f, nb = c.handles()
    tensor = "split_flux_tensor_kernel" in kernel_names(e, f, nb)
    assert case_is_affine(c) == (order <= 4 and tensor)
    if order == 4:
        assert case_is_affine(c)
    set_option(c, "affine_metrics", 0)
    assert not case_is_affine(c) and case_is_affine(c, form=False)
    c.close()


@gpu
def test_detection_sheared_box_is_affine_and_a_displaced_vertex_is_not():
    for xv, want in ((sheared_xv([4, 4, 4]), True), (displaced_xv([4, 4, 4]), False)):
        c = H.Case([4, 4, 4], xv=xv, order=3)
        c.to_device(0)
        assert case_is_affine(c) == want and case_is_affine(c, form=False) == want
        c.close()


@gpu
@pytest.mark.parametrize("name", ["hex_p2_n3_deformed", "hex_p4_jet"])
def test_detection_deformed_fixtures_are_not_affine(name):
    ctx = hfx.Context(0)
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    e, faces = build(ctx, d)
    names = kernel_names(e.h, hfx._face_array(faces), len(faces))
    assert "affine_metrics" not in names and "affine_block" not in names
    for f in faces:
        f.close()
    e.close(); ctx.close()


@gpu
def test_detection_quad_p7_deformed_is_affine():
    """(parallelograms: test_quad_p7_deformed_is_a_mesh_of_parallelograms)"""
    ctx = hfx.Context(0)
    e, faces = build(ctx, dict(np.load(os.path.join(GOLDEN, "quad_p7_deformed.npz"))))
    names = kernel_names(e.h, hfx._face_array(faces), len(faces))
    assert "affine_metrics" in names or "affine_block" in names
    for f in faces:
        f.close()
    e.close(); ctx.close()


def _run(n, steps, fused, xv=None, order=4, opts=(), **kw):
    c = H.Case(n, xv=xv, order=order, **kw)
    c.to_device(0)
    for k, v in opts:
        set_option(c, k, v)
    c.run_steps_lib(steps, fused=fused)
    c.sync_host()
    u = c.array("disu_upts0").copy()
    c.close()
    return u


@gpu
@pytest.mark.parametrize("mesh", ["box", "sheared"])
@pytest.mark.parametrize("order", [2, 4])
def test_affine_stage_against_the_per_method_path_and_the_general_metrics(mesh, order):
    n = [4, 4, 4]
    xv = sheared_xv(n) if mesh == "sheared" else None
    want = _run(n, 3, False, xv, order)
    on = _run(n, 3, 3, xv, order)
    off = _run(n, 3, 3, xv, order, opts=[("affine_metrics", 0)])
    print("%s P%d: affine vs per-method %.3g, general vs per-method %.3g, affine vs general %.3g" %
          (mesh, order, relerr(on, want), relerr(off, want), relerr(on, off)))
    assert relerr(on, want) < TOL_FUSED
    assert relerr(on, off) < TOL_FUSED
    assert relerr(on, _run(n, 0, 3, xv, order)) > 1e-8  # (the state moved)


@gpu
def test_non_affine_block_is_bit_identical_with_the_option_on_and_off():
    n = [4, 4, 4]
    on = _run(n, 2, 3, amp=0.1)
    off = _run(n, 2, 3, amp=0.1, opts=[("affine_metrics", 0)])
    assert np.array_equal(on, off)


@gpu
def test_self_partitioned_affine_block_equals_the_undivided_one(tmp_path):
    n = [3, 4, 3]
    cfg = dict(order=3, amp=0.0, length=6.2831853071795862, T_c_ic=300.0, dt=1e-4, riemann_solve_type=3)
    c = H.Case(n, **cfg)
    c.to_device(0)
    assert case_is_affine(c)
    c.close()
    one = _run(n, 2, 3, **cfg)
    PU.spawn(PU.gpu_worker, 1, (n, [1, 1, 1], dict(cfg, self_partition=[1, 0, 1]), 2, str(tmp_path), "fused", "gloo", "rccl"))
    u = PU.assemble(str(tmp_path), "u", n, [1, 1, 1], one.shape)
    print("self-partitioned vs undivided: %.3g" % relerr(u, one))
    assert relerr(u, one) < TOL_PARTITION


@gpu
def test_kernel_bytes_price_the_metric_record():
    """An affine block (P4 hex): the flux kernel reads the 34-double record and JGinv at the solution points (1 125, the one
    per-point metric it keeps: it transforms the total flux, pressure included) in place of its 3 200 per-point metric doubles;
    the update kernel 1 in place of 125; the face kernel keeps its per-point normal and tdA.  A general block, and the option
    off: as before."""
    order = 4
    N = order + 1
    nu, nfp, nf, nd, ne = N ** 3, 6 * N ** 2, 5, 3, 64
    general = [0.0,
               ne * 8.0 * (nu * nf + nfp * nf + nu * (nd * nd + 1) + nfp * (nd * nd + 1) + nfp * nd + nu * nf + nfp * nf) + ne * 4.0 * nfp,
               ne * (8.0 * (nfp * nf + nfp * nf + 0.5 * nfp * nd + nfp + nfp * nf) + 4.0 * nfp),
               ne * 8.0 * (3 * nu * nf + nu + nfp * nf + 2 * nu * nf + nfp * nf)]
    for amp, opt, affine in ((0.0, 1, True), (0.0, 0, False), (0.1, 1, False)):
        c = H.Case([4, 4, 4], order=order, amp=amp)
        c.to_device(0)
        c.run_steps_lib(1, fused=3)  # builds the block's fused tables
        set_option(c, "affine_metrics", opt)
        b = (C.c_double * 8)()
        hfx.check(hfx.lib().hfx_fused_kernel_bytes(c.handles()[1], b))
        got = list(b)[:4]
        c.close()
        if not affine:
            assert got == general, (amp, opt)
            continue
        assert general[1] - got[1] == ne * 8.0 * (3200 - 34 - 1125)
        assert general[2] == got[2]
        assert general[3] - got[3] == ne * 8.0 * (125 - 1)
        assert got[0] == 0.0
