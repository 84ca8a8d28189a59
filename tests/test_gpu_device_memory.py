"""Device memory of libhfx: every allocation has one owner (DevBuf), so registration calls may come in any order, a
create / destroy cycle gives back every byte and a failing registration leaves nothing behind.  The shared boxes make
the device-wide free memory noisy, so the tests read the library's own count of the bytes it holds
(hfx_live_device_bytes_internal)."""
import ctypes as C
import os

import numpy as np
import pytest

import hfx
import partition_util as PU
from test_gpu_methods_vs_golden import build, relerr, ALL, GOLDEN, RTOL1, RTOLD, RTOLS

pytestmark = pytest.mark.gpu

CYCLES = 3


def live_bytes():
    fn = hfx.lib().hfx_live_device_bytes_internal
    fn.restype = C.c_long
    return fn()


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def close(e, faces):
    for f in faces:
        f.close()
    e.close()


@pytest.mark.parametrize("name", [n for n in ALL if "_les_" in n and not n.startswith(("tet_", "pri_"))])
def test_set_h_ref_after_set_les(name):
    """hfx_eles_set_h_ref touches h_ref only: registered AFTER the LES closure it leaves wall_distance and Jacobian_fpts
    alone.  The per-method stage and the split fused stage then match the reference at the tolerances of
    test_les_intermediates, test_stage_states_vs_reference and test_fused_vs_reference."""
    d = load(name)
    nstage = int(d["sizes"][7])
    h_ref = d["h_ref"] if "h_ref" in d else np.ones(int(d["sizes"][0]))
    ctx = hfx.Context(0)
    e, faces = build(ctx, d)  # (registers the closure)
    e.set_h_ref(h_ref)
    if int(np.ravel(d["SGS_model"])[0]) >= 2:
        e.calc_sgs_terms()
    hfx.CalcResidual(e, faces)
    if "s0_sgsf_upts" in d:
        assert relerr(e.download(hfx.SGSF_UPTS), d["s0_sgsf_upts"]) < 1e-11
        assert relerr(e.download(hfx.SGSF_FPTS), d["s0_sgsf_fpts"]) < 1e-11
        assert relerr(e.download(hfx.TDISF_UPTS), d["s0_tdisf_upts"]) < RTOL1
    assert relerr(e.download(hfx.DIV_TCONF_UPTS), d["s0_div_tconf_upts"]) < RTOLD
    for fused, tol in ((0, RTOLS), (2, 1e-11), (3, 1e-11)):
        e.upload(hfx.DISU_UPTS0, d["u_init"])
        hfx.run_steps(e, faces, 1, fused=fused)
        assert relerr(e.download(hfx.DISU_UPTS0), d["u_step0_stage%d" % (nstage - 1)]) < tol, fused
    assert e.check_nan() == -1
    close(e, faces)
    ctx.close()


@pytest.mark.parametrize("name", ["hex_p2_les_smag", "hex_p2_les_wsm", "hex_p2_overint", "hex_p3_shock", "hex_p2_bdy_walls", "quad_p3_les_wale",
                                  "tet_p2_les_wale", "tet_p3_les_sim", "tet_p2_overint", "tet_p3_shock", "pri_p2_les_wale", "pri_p2_overint",
                                  "pri_p2_shock"])
def test_create_destroy_cycles_give_back_every_byte(name):
    """a context, an element block with what its fixture registers (an LES closure, over-integration, shock capturing) and
    its interior and boundary face blocks; one fused step with the flux kernel's time stamps on -- the split stage on
    hexahedra and quadrilaterals, the general stage on tetrahedra and prisms -- and one per-method stage; after the
    destroy the library holds exactly the bytes it held before the create, in every cycle"""
    d = load(name)
    fused = 4 if name.startswith(("tet_", "pri_")) else 3
    before = live_bytes()
    for cycle in range(CYCLES):
        ctx = hfx.Context(0)
        e, faces = build(ctx, d)
        e.set_h_ref(np.ones(e.n_eles))
        assert live_bytes() > before
        ctx.set_option("flux_stamps", 1)
        hfx.run_steps(e, faces, 1, fused=fused)
        hfx.CalcResidual(e, faces)
        ctx.synchronize()
        close(e, faces)
        ctx.close()
        assert live_bytes() - before == 0, cycle


def _partitioned_cycles_worker(rank, world, port, outdir):
    import torch
    import hfx_host as H
    torch.cuda.set_device(0)
    walls = dict(bcs=[dict(type="isotherm_wall", T_static=310.0, u=3.0), dict(type="adiabat_wall", v=-2.0)], sides={"y-": 0, "y+": 1})
    shock = dict(shock_cap=1, s0=1e-3, expf_fac=36.0, expf_order=4, expf_cutoff=1, shock_det_field=0)
    cfgs = [dict(order=3, amp=0.1, riemann_solve_type=3, LES=1, SGS_model=1, C_s=0.325, filter_ratio=1.0, **shock, **walls),
            dict(order=3, amp=0.1, riemann_solve_type=3, over_int=1, over_int_order=5, **shock, **walls)]
    left = []
    for cfg in cfgs:
        before = live_bytes()
        for cycle in range(CYCLES):
            c = H.Case([3, 4, 3], self_partition=[1, 0, 1], **cfg)
            c.to_device(0)
            hfx.check(hfx.lib().hfx_ctx_set_option(c.handles()[0], b"flux_stamps", C.c_int(1)))
            c.set_comm(hfx.comm_unique_id())
            held = live_bytes() - before
            c.run_partitioned(1)  # the partitioned split fused stage
            c.run(1)              # the mirrored per-method loop
            c.synchronize()
            c.close()
            left.append([held, live_bytes() - before])
    np.save(outdir + "/left.npy", np.array(left, dtype=np.int64))


def test_create_destroy_cycles_partitioned_blocks(tmp_path):
    """the same for a rank that is its own neighbour in x and z with walls in y: interior, boundary and partition-face blocks
    and the library's communicator; an LES closure with shock capturing, and over-integration with shock capturing (the
    split stage refuses a closure together with over-integration, so two blocks carry the three between them)"""
    PU.spawn(_partitioned_cycles_worker, 1, (str(tmp_path),))
    left = np.load(str(tmp_path / "left.npy"))
    assert left.shape == (2 * CYCLES, 2)
    assert np.all(left[:, 0] > 0)
    assert np.all(left[:, 1] == 0), left


def test_failing_registration_leaves_nothing_behind():
    """hfx_eles_create without opp_2_1 fails after the operators before it were made, hfx_int_inters_create with an entry of
    R out of range: the existing messages, and not a byte more held than before"""
    d = load("hex_p2_n3_deformed")
    ctx = hfx.Context(0)
    ctx.set_params(hfx.params_from(d))
    sz = [int(v) for v in d["sizes"]]
    before = live_bytes()
    less = {k: v for k, v in d.items() if k != "opp_2_1"}
    for _ in range(CYCLES):
        with pytest.raises(hfx.HfxError, match="hfx_eles_create: missing opp_1/opp_2"):
            hfx.Eles(ctx, sz[:5], less, ele_type=sz[6], order=sz[5])
        assert live_bytes() - before == 0
    e = hfx.Eles(ctx, sz[:5], d, ele_type=sz[6], order=sz[5])
    held = live_bytes()
    assert held > before
    R = np.array(d["int2_R"]).copy()
    R.flat[R.size // 2] = e.n_fpts * e.n_eles
    for _ in range(CYCLES):
        with pytest.raises(hfx.HfxError, match=r"face table R\[\d+\] = \d+ out of range"):
            hfx.IntInters(ctx, e, e, d["int2_L"], R)
        assert live_bytes() - held == 0
    e.close()
    assert live_bytes() - before == 0
    ctx.close()
