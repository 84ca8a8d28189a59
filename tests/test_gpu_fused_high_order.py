"""Hexahedra of orders 6 and 7 on the split fused stage: 343 / 512 solution points per element take the wide row entries of
variant 2 (csrc/split_common.hpp, Geo::WIDE), and a request for variant 3 -- whose flux kernel does not fit one such element
in LDS -- runs variant 2 (split_plan, csrc/fused_hex.hip).  Against the per-method path, the genuine reference's fixtures,
the host mirror's unchanged loop and the undivided block of a self-partitioned run."""
import ctypes as C
import os

import numpy as np
import pytest

import hfx
import hfx_host as H
import partition_util as PU
from test_gpu_methods_vs_golden import build, relerr, GOLDEN

pytestmark = pytest.mark.gpu

ORDERS = [6, 7]


def per_method_and_fused(n, modes, **kw):
    """one step of the per-method path and of every fused mode in `modes` on the same case"""
    out = {}
    for mode in (False,) + tuple(modes):
        c = H.Case(n, **kw)
        c.to_device(0)
        c.run_steps_lib(1, fused=mode)
        c.sync_host()
        out[mode] = c.array("disu_upts0").copy()
        c.close()
    return out


@pytest.mark.parametrize("order", ORDERS)
def test_split_paths_vs_methods(order):
    """the check test_gpu_fused.py::test_split_paths_every_order_vs_methods skips for hexes above P5"""
    u = per_method_and_fused([3, 3, 3], (2, 3), order=order, amp=0.1)
    for mode in (2, 3):
        assert relerr(u[mode], u[False]) < 1e-12, (mode, order)


def test_variant3_request_runs_variant2():
    """fused = 3 on a P6 hex block is routed to variant 2: the same bits, and a state that has moved"""
    u = per_method_and_fused([3, 3, 3], (2, 3), order=6, amp=0.1)
    assert np.array_equal(u[3], u[2])
    assert relerr(u[3], H.Case([3, 3, 3], order=6, amp=0.1).array("disu_upts0")) > 1e-8


@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("name", ["hex_p6_deformed", "hex_p7_deformed"])
def test_fused_vs_reference_fixture(name, mode):
    ctx = hfx.Context(0)
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    e, faces = build(ctx, d)
    hfx.run_steps(e, faces, 1, fused=mode)
    nstage = int(d["sizes"][7])
    assert relerr(e.download(hfx.DISU_UPTS0), d["u_step0_stage%d" % (nstage - 1)]) < 1e-11
    assert e.check_nan() == -1
    for f in faces:
        f.close()
    e.close()
    ctx.close()


def test_host_mirror_unchanged_loop_runs_fused():
    """the mirrored CalcResidual + AdvanceSolution loop on a deformed P6 box (the fixture's generator on three cells per
    direction, which the mirror's periodic matching needs) defers by default: every stage but the one pending at sync_host
    runs as the fused stage -- before, the block's fused tables were refused and every stage was replayed call by call --
    and the state equals the per-method path's"""
    ref = H.Case(3, order=6, amp=0.15)
    ref.to_device(0)
    ref.run_steps_lib(1, fused=False)
    ref.sync_host()
    want = ref.array("disu_upts0").copy()
    ref.close()
    c = H.Case(3, order=6, amp=0.15)
    c.to_device(0)
    ctx = c.handles()[0]
    c.run(1)
    c.sync_host()
    assert relerr(c.array("disu_upts0"), want) < 1e-11
    nf, nr, why = hfx.deferred_stats(ctx)
    assert (nf, nr) == (4, 1), why
    c.close()


WALLS = dict(bcs=[dict(type="isotherm_wall", T_static=310.0, u=3.0), dict(type="adiabat_wall", v=-2.0)],
             sides={"y-": 0, "y+": 1})


@pytest.mark.parametrize("what,kw", [
    ("walls", WALLS),
    ("wale", dict(LES=1, SGS_model=1, C_s=0.325, filter_ratio=1.0)),
    # s0 = 0: every element is filtered after every stage (dense filter + extrapolate_solution at this order)
    ("shock", dict(shock_cap=1, s0=0.0, expf_fac=36.0, expf_order=4, expf_cutoff=1, shock_det_field=0)),
])
def test_p6_ingredients_vs_methods(what, kw):
    u = per_method_and_fused([3, 3, 3], (3,), order=6, amp=0.1, riemann_solve_type=3, **kw)
    assert np.isfinite(u[3]).all()
    assert relerr(u[3], u[False]) < 1e-11, what


def _self_partition_worker(rank, world, port, outdir):
    import torch
    import hfx
    import hfx_host as H
    torch.cuda.set_device(0)
    kw = dict(order=6, amp=0.1, riemann_solve_type=3)
    c = H.Case([3, 3, 3], self_partition=[1, 0, 1], **kw)
    c.to_device(0)
    c.set_comm(hfx.comm_unique_id())
    c.run_partitioned(1)
    c.sync_host()
    part = c.array("disu_upts0").copy()
    c.close()
    one = H.Case([3, 3, 3], **kw)
    one.to_device(0)
    one.run_steps_lib(1, fused=3)
    one.sync_host()
    whole = one.array("disu_upts0").copy()
    one.close()
    np.save(outdir + "/part.npy", part)
    np.save(outdir + "/whole.npy", whole)


def test_self_partitioned_p6_block(tmp_path):
    """the wrap-around faces of x and z as partition faces whose neighbour is the rank itself (the library's RCCL transport,
    the partitioned fused stage of variant 2 with the corrected gradient on the wire) against the undivided block"""
    PU.spawn(_self_partition_worker, 1, (str(tmp_path),))
    part, whole = np.load(str(tmp_path / "part.npy")), np.load(str(tmp_path / "whole.npy"))
    assert np.isfinite(part).all()
    assert relerr(part, whole) < 1e-11


@pytest.mark.parametrize("order", ORDERS)
def test_kernel_bytes_are_variant2(order):
    """hfx_fused_kernel_bytes with the context's default (variant 3) counts the variant that runs: variant 2"""
    c = H.Case([3, 3, 3], order=order, amp=0.1)
    c.to_device(0)
    ctx, e = c.handles()[0], c.handles()[1]
    got = (C.c_double * 8)()
    for mode in (3, 2):
        hfx.check(hfx.lib().hfx_ctx_set_fused_mode(ctx, C.c_int(mode)))
        hfx.check(hfx.lib().hfx_fused_kernel_bytes(e, got))
        N = order + 1
        nu, nfp, nf, nd, ne = N ** 3, 6 * N ** 2, 5, 3, 27
        want = [ne * (8.0 * (2 * nfp * nf) + 4.0 * nfp + nfp * 0.5),
                ne * 8.0 * (nu * nf + nfp * nf + nu * (nd * nd + 1) + nfp * (nd * nd + 1) + nfp * nf * nd),
                ne * (8.0 * (nfp * nf + nfp * nf * nd + 0.5 * nfp * nd + nfp + nfp * nf) + 4.0 * nfp),
                ne * 8.0 * (nu * nf + nu * (nd * nd + 1) + nfp * nf + 3 * nu * nf + nfp * nf),
                0.0, 0.0, 0.0, 0.0]
        assert list(got) == want, mode
    c.close()
