"""The history monitor on the device (hfx_ctx_set_history_monitor, hfx_eles_sample_history, hfx_eles_read_history) inside every
step loop and through the host mirror, against the genuine DRIVER's rows of history.plt (tests/golden/history_rows/hr_*.npz).

Bars (tests/history_rows_util.py): a residual column 1e-11 relative on the norm plus 1e-14 x max(1, |value|) for the printed
digits; force columns 1e-11 of their un-cancelled scale (in the loops: of the row's own size, which is no larger) plus the digits;
against hfx_eles_compute_res_upts 1e-13 relative (sums of non-negative terms in another order), bit-equal for the maximum; the force
columns bit-equal to hfx_eles_compute_wall_forces.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import bdy_util
import hfx
import hfx_host as H
import history_rows_util as HU
import integral_history_util as IU
import partition_util as PU
import wall_force_util as W
from test_gpu_methods_vs_golden import build
from test_wall_force_host import device_arrays, mirror_case, phys_of, ref_of

pytestmark = pytest.mark.gpu

HEXES = ["hr_hex_p2_rk45", "hr_hex_p2_euler", "hr_hex_p2_norm0", "hr_hex_p2_norm1", "hr_hex_p2_walls", "hr_hex_p2_forced"]
STALE_DIV = "div_tconf_upts was not stored by the fused stage that ran last"
ELE_AXIS = {"detjac_upts": 1, "JGinv_upts": 3, "detjac_fpts": 1, "JGinv_fpts": 3, "tdA_fpts": 1, "norm_fpts": 1, "pos_upts": 1,
            "vol_detjac_vol_cubpts": 1}


@pytest.fixture()
def ctx():
    c = hfx.Context(0)
    yield c
    c.close()


def close(e, faces):
    for f in faces:
        f.close()
    e.close()


@functools.lru_cache(maxsize=None)
def setup(name):
    """the fixture and, with calc_force, the wall faces the host mirror builds for it (no device); made once, left unchanged"""
    d = HU.load(name)
    s = dict(d=d, meta=HU.meta_of(d), forces=bool(int(d["calc_force"][0])), norm=int(d["res_norm_type"][0]),
             freq=int(d["monitor_res_freq"][0]), forced=bool("body_forcing" in d and int(d["body_forcing"][0])))
    if s["forced"]:
        s["F"] = HU.forcing_of(d)
    if s["forces"]:
        mc, _ = mirror_case(d)
        s.update(A=device_arrays(mc), phys=phys_of(mc), ref=ref_of(mc))
        mc.close()
    return s


def make(ctx, s):
    e, faces = build(ctx, s["d"])
    if s["forces"]:
        A = s["A"]
        ctx.set_force_reference(**s["ref"])
        e.set_wall_faces(A["face_ele"], A["face_inter"], A["face_flag"], A["opp"], A["weight"], A["detjac"], A["norm"])
    if s["forced"]:  # (the driver ran with body_forcing 1: the reference's hard-coded area and mass flux)
        s["F"].register(e, HU.FORCING_MDOT0)
    if s["d"]["hist_diag"].shape[1]:
        d = s["d"]
        e.set_volume_cubpts(d["opp_volume_cubpts"], d["weight_volume_cubpts"], d["vol_detjac_vol_cubpts"])
    return e, faces


def log_columns(norm, res, n_pts):
    return np.log10(HU.norm_residual(norm, res, n_pts))


def run_loop(e, faces, n, fused):
    if fused == 4:
        hfx.run_steps_blocks([e], faces, n, fused=4)
    else:
        hfx.run_steps(e, faces, n, fused=fused)


def force_columns_of(raw, nd):
    """(2 n_dims + 2) raw values -> F total per dimension, CL, CD"""
    return np.concatenate([raw[:nd] + raw[nd:2 * nd], raw[2 * nd:]])


# ---- 1. one sample ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [0, 1, 2])
@pytest.mark.parametrize("name", HU.HR)
def test_one_sample(ctx, name, norm):
    """one per-method step from the clock 0 takes the driver's row 1; a direct sample of the same arrays is that row bit for bit;
    every field agrees with hfx_eles_compute_res_upts, the force columns are hfx_eles_compute_wall_forces' bits"""
    s = setup(name)
    d = s["d"]
    e, faces = make(ctx, s)
    ctx.set_history_monitor(norm, s["forces"], monitor_res_freq=1, capacity=3)
    ctx.set_clock(0.0, 0)
    hfx.run_steps(e, faces, 1)
    assert e.history_count() == 1
    e.sample_history(0.5, 7)
    e.sample_history(0.75, 8)
    old = np.array([e.compute_res_upts(norm, f) for f in range(e.n_fields)])
    wf = e.compute_wall_forces(points=False) if s["forces"] else None
    times, steps, res, frc = e.read_history()
    assert list(steps) == [1, 7, 8] and list(times[1:]) == [0.5, 0.75] and e.history_count() == 0
    assert np.array_equal(res[:, 0], res[:, 1]) and np.array_equal(res[:, 0], res[:, 2])
    assert np.array_equal(frc[:, 0], frc[:, 1]) and np.array_equal(frc[:, 0], frc[:, 2])
    rel = np.abs(res[:, 0] - old) / np.abs(old)
    print("%s norm %d: against compute_res_upts %.3e" % (name, norm, rel.max()))
    assert np.all(rel <= 1e-13) and np.all(old > 0)
    if norm == 0:
        assert np.array_equal(res[:, 0], old)
    nd = e.n_dims
    if s["forces"]:
        raw = np.concatenate([wf["inv_force"], wf["vis_force"], [wf["cl"]], [wf["cd"]]])
        assert np.array_equal(frc[:, 0], raw) and np.any(raw[:nd] != 0) and np.any(raw[nd:2 * nd] != 0)
        miss = HU.value_miss(force_columns_of(frc[:, 0], nd), d["hist_force"][0],
                             HU.force_columns(W, s["A"], s["phys"], s["ref"], e.download(hfx.DISU_UPTS0), e.download(hfx.GRAD_DISU_UPTS))[1])
        print("%s: force columns against the driver's row 1: %.3f bars" % (name, miss))
        assert miss <= 1.0
    else:
        assert not np.any(frc)
    if norm == s["norm"]:
        miss = HU.log_miss(log_columns(norm, res[:, 0], e.n_upts * e.n_eles), d["hist_res"][0])
        print("%s norm %d: against the driver's row 1: %.3f bars" % (name, norm, miss))
        assert miss <= 1.0
    close(e, faces)


# ---- 2. past the first pass, unaligned planes ---------------------------------------------------------------------------------------
def tiled(d, n_eles):
    """the fixture's block without faces, its elements repeated up to n_eles"""
    sz = [int(v) for v in d["sizes"]]
    copies = -(-n_eles // sz[0])
    t = dict(d)
    for k, ax in ELE_AXIS.items():
        if k in d:
            t[k] = np.take(np.concatenate([d[k]] * copies, axis=ax), np.arange(n_eles), axis=ax)
    t["u_init"] = np.take(np.concatenate([d["u_init"]] * copies, axis=1), np.arange(n_eles), axis=1)
    sizes = np.array(d["sizes"]).copy()
    sizes[0] = n_eles
    t["sizes"] = sizes
    for k in [k for k in t if (k.startswith("int") and k[3].isdigit()) or k.startswith("bdy")]:
        del t[k]
    return t


@pytest.mark.parametrize("with_src", [False, True])
@pytest.mark.parametrize("name", ["hr_hex_p2_rk45", "hr_tet_p2_rk45"])
def test_past_the_first_pass(name, with_src):
    """caps 1, 2 and 3 on a block whose every workgroup walks more than three passes; the plane length is odd and no multiple of a
    lane's four points, so the odd fields' planes begin 8 bytes off a 16-byte boundary and the last item is not whole.  Against
    numpy and hfx_eles_compute_res_upts at 1e-13, capped against uncapped at 1e-13, two samples under one cap bit-equal."""
    d = HU.load(name)
    n_upts = int(d["sizes"][1])
    ppp = 1024
    n_eles = -(-(3 * 3 * ppp + 1) // n_upts)
    while (n_eles * n_upts) % 4 == 0 or (n_upts % 2 == 1 and (n_eles * n_upts) % 2 == 0):
        n_eles += 1
    t = tiled(d, n_eles)
    P = n_eles * n_upts
    rng = np.random.default_rng(20261020)
    rows = {}
    for cap in (0, 1, 2, 3):
        c = hfx.Context(0)
        if cap:
            c.set_option("persistent_grid_cap", cap)
        e, faces = build(c, t)
        n_fields = e.n_fields
        if cap == 0:
            div = rng.uniform(-1.0, 1.0, (n_upts, n_eles, n_fields))
            src = rng.uniform(-1.0, 1.0, (n_upts, n_eles, n_fields)) * 3.0 if with_src else None
        e.upload(hfx.DIV_TCONF_UPTS, div)
        if with_src:
            e.upload(hfx.SRC_UPTS, src)
        groups, per_pass = e.history_launch()
        assert per_pass == ppp and groups == (cap if cap else -(-(-(-P // 4)) // 256)) and (cap == 0 or P > 3 * cap * ppp)
        for norm in (0, 1, 2):
            c.set_history_monitor(norm, False, 1, 2)
            e.sample_history(0.0, 0)
            e.sample_history(0.0, 0)
            res = e.read_history()[2]
            assert np.array_equal(res[:, 0], res[:, 1])
            old = np.array([e.compute_res_upts(norm, f) for f in range(n_fields)])
            want = HU.res_upts(norm, div, t["detjac_upts"], src)
            assert np.all(np.abs(res[:, 0] - want) <= 1e-13 * np.abs(want)), (cap, norm)
            assert np.all(np.abs(res[:, 0] - old) <= 1e-13 * np.abs(old)), (cap, norm)
            if norm == 0:
                assert np.array_equal(res[:, 0], old)
            rows[cap, norm] = res[:, 0]
        close(e, faces)
        c.close()
    for cap in (1, 2, 3):
        for norm in (0, 1, 2):
            assert np.all(np.abs(rows[cap, norm] - rows[0, norm]) <= 1e-13 * np.abs(rows[0, norm]))
    if n_upts % 2 == 1:
        assert P % 2 == 1
    assert P % 4 != 0


@pytest.mark.parametrize("with_src", [False, True])
def test_unaligned_planes_on_the_fixture_itself(ctx, with_src):
    """the 3^3 P2 block: 729 points per plane"""
    d = HU.load("hr_hex_p2_rk45")
    e, faces = build(ctx, d)
    assert (e.n_upts * e.n_eles) % 2 == 1
    hfx.CalcResidual(e, faces)
    div = e.download(hfx.DIV_TCONF_UPTS)
    src = None
    if with_src:
        src = np.random.default_rng(7).uniform(-1.0, 1.0, div.shape) * np.abs(div / d["detjac_upts"][:, :, None]).max()
        e.upload(hfx.SRC_UPTS, src)
    for norm in (0, 1, 2):
        ctx.set_history_monitor(norm, False, 1, 1)
        e.sample_history(0.0, 0)
        res = e.read_history()[2][:, 0]
        want = HU.res_upts(norm, div, d["detjac_upts"], src)
        assert np.all(np.abs(res - want) <= 1e-13 * np.abs(want)), norm
    close(e, faces)


# ---- 3. in the loops, against the genuine driver ----------------------------------------------------------------------------------
def check_rows(s, e, times, steps, res, frc, what, diag=None):
    d = s["d"]
    assert list(steps) == [int(v) for v in d["hist_iter"]], what
    n_pts, nd = e.n_upts * e.n_eles, e.n_dims
    t = times * float(d["time_ref"][0])
    for k in range(len(steps)):
        miss = HU.log_miss(log_columns(s["norm"], res[:, k], n_pts), d["hist_res"][k])
        print("%s row at step %d: residual columns %.3f bars" % (what, steps[k], miss))
        assert miss <= 1.0, (what, k)
        assert abs(t[k] - d["hist_time"][k]) <= 1e-14 * d["hist_time"][k], (what, k)
        if s["forces"]:
            S = np.abs(d["hist_force"][k]).max()  # (the columns' own size: the un-cancelled scale is no smaller)
            miss = HU.value_miss(force_columns_of(frc[:, k], nd), d["hist_force"][k], S)
            print("%s row at step %d: force columns %.3f bars of the row's own size" % (what, steps[k], miss))
            assert miss <= 1.0, (what, k)
        if diag is not None:
            assert HU.value_miss(diag[:, k], d["hist_diag"][k], np.abs(d["hist_diag"][k]).max()) <= 1.0, (what, k)


LOOPS = [(n, f) for n in HEXES + ["hr_quad_p3_walls"] for f in (0, 2, 3)] + [("hr_tet_p2_rk45", 0), ("hr_tet_p2_rk45", 4)]


@pytest.mark.parametrize("name,fused", LOOPS)
def test_loop_rows_vs_the_driver(ctx, name, fused):
    """the clock at 0, the monitor as the fixture's input has it, ONE call of the fixture's steps: the loop takes the driver's rows;
    where the fixture has integral quantities that monitor runs beside this one, under the one monitor_res_freq"""
    s = setup(name)
    d = s["d"]
    e, faces = make(ctx, s)
    ctx.set_history_monitor(s["norm"], s["forces"], s["freq"], capacity=4)
    ids = [int(v) for v in np.ravel(d["integral_quantity_ids"])] if d["hist_diag"].shape[1] else []
    if ids:
        ctx.set_integral_monitor(ids, monitor_res_freq=s["freq"], capacity=4)
    ctx.set_clock(0.0, 0)
    n = s["meta"]["steps"]
    run_loop(e, faces, n, fused)
    assert ctx.get_clock()[1] == n
    times, steps, res, frc = e.read_history()
    diag = e.read_integral_history()[2] if ids else None
    check_rows(s, e, times, steps, res, frc, "%s fused %d" % (name, fused), diag)
    close(e, faces)


def test_fused_state_with_and_without_the_monitor():
    """fused 3: with residuals alone the loop launches what it launched before and the state is bit-equal; with viscous forces the
    sampled steps end call by call and the state agrees to 1e-12, the bound of the integral monitor"""
    s = setup("hr_quad_p3_walls")
    out = {}
    for what in ("none", "residuals", "forces"):
        c = hfx.Context(0)
        e, faces = make(c, s)
        if what != "none":
            c.set_history_monitor(s["norm"], what == "forces", s["freq"], capacity=4)
        c.set_clock(0.0, 0)
        hfx.run_steps(e, faces, s["meta"]["steps"], fused=3)
        out[what] = e.download(hfx.DISU_UPTS0)
        assert e.history_count() == (0 if what == "none" else len(s["d"]["hist_iter"]))
        close(e, faces)
        c.close()
    assert np.array_equal(out["residuals"], out["none"])
    err = np.abs(out["forces"] - out["none"]).max() / np.abs(out["none"]).max()
    print("hr_quad_p3_walls: state with viscous forces against without a monitor %.3e" % err)
    assert err <= 1e-12


# ---- 4. refusals, each before any launch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [0, 3])
def test_capacity_is_checked_before_the_first_launch(ctx, fused):
    s = setup("hr_hex_p2_euler")
    e, faces = make(ctx, s)
    ctx.set_history_monitor(2, False, 1, capacity=1)
    ctx.set_clock(0.0, 0)
    u0 = e.download(hfx.DISU_UPTS0)
    with pytest.raises(hfx.HfxError, match="take 2 rows"):
        hfx.run_steps(e, faces, 2, fused=fused)
    assert ctx.get_clock()[:2] == (0.0, 0) and e.history_count() == 0
    assert np.array_equal(e.download(hfx.DISU_UPTS0), u0)
    hfx.run_steps(e, faces, 1, fused=fused)
    with pytest.raises(hfx.HfxError, match="take 1 rows"):
        hfx.run_steps(e, faces, 1, fused=fused)
    assert list(e.read_history()[1]) == [1]
    close(e, faces)


def test_registration_refusals(ctx):
    s = setup("hr_quad_p3_walls")
    e, faces = build(ctx, s["d"])
    with pytest.raises(hfx.HfxError, match="no monitor"):
        e.sample_history(0.0, 0)
    with pytest.raises(hfx.HfxError, match="norm_type not recognized"):
        ctx.set_history_monitor(3, False, 1, 2)
    with pytest.raises(hfx.HfxError, match="hfx_ctx_set_force_reference"):
        ctx.set_history_monitor(2, True, 1, 2)
    with pytest.raises(hfx.HfxError, match="monitor_res_freq"):
        ctx.set_history_monitor(2, False, 0, 2)
    ctx.set_integral_monitor([0], monitor_res_freq=3, capacity=2)
    with pytest.raises(hfx.HfxError, match="monitor_res_freq 2.*registered with 3"):
        ctx.set_history_monitor(2, False, 2, 2)
    ctx.set_history_monitor(2, False, 3, 2)
    with pytest.raises(hfx.HfxError, match="monitor_res_freq 5.*registered with 3"):
        ctx.set_integral_monitor([0], monitor_res_freq=5, capacity=2)
    assert e.history_count() == 0
    # a full history; fewer than stored is refused and nothing is lost; capacity 0 drops the monitor and empties the histories
    hfx.CalcResidual(e, faces)
    e.sample_history(0.0, 0)
    e.sample_history(0.0, 1)
    with pytest.raises(hfx.HfxError, match="history is full"):
        e.sample_history(0.0, 2)
    t, st, r, n = np.zeros(2), np.zeros(2, dtype=np.int32), np.zeros(8), C.c_int(0)
    rc = hfx.lib().hfx_eles_read_history(e.h, C.c_int(1), t.ctypes.data_as(hfx.dp), st.ctypes.data_as(hfx.ip), r.ctypes.data_as(hfx.dp),
                                         None, C.byref(n))
    assert rc != 0 and e.history_count() == 2
    ctx.set_history_monitor(2, False, 3, 0)
    assert e.history_count() == 0
    close(e, faces)


def test_stale_arrays_are_refused(ctx):
    """a gradient a fused 3 loop kept on chip is refused, never read stale, and nothing is stored; residuals alone sample behind the
    same loop, whose last stage stored div_tconf_upts"""
    s = setup("hr_quad_p3_walls")
    e, faces = make(ctx, s)
    ctx.set_history_monitor(2, True, 1, 4)
    hfx.run_steps(e, faces, 1, fused=3)  # (no clock: the loop samples nothing and keeps the gradient on chip)
    assert e.history_count() == 0
    with pytest.raises(hfx.HfxError, match="was not materialised by the fused stage that ran last"):
        e.sample_history(0.0, 1)
    assert e.history_count() == 0
    ctx.set_history_monitor(2, False, 1, 4)  # residuals alone: div_tconf_upts of the last stage is there
    e.sample_history(0.0, 1)
    assert e.history_count() == 1
    close(e, faces)


def test_stale_div_tconf_is_refused():
    """deferred execution: an RK stage that is not the last of its step runs fused without storing div_tconf_upts when nothing asks for
    it; once another entry point has flushed it that way, a sample is refused"""
    from test_gpu_deferred import calc_residual_calls, tag
    s = setup("hr_hex_p2_rk45")
    d = s["d"]
    c = hfx.Context(0)
    c.set_option("deferred", 1)
    e, faces = build(c, d)
    tag(e, d)
    c.set_history_monitor(2, False, 1, 2)
    calc_residual_calls([e], faces, True, 0)
    e.AdvanceSolution(0, 3)
    e.download(hfx.DISU_UPTS0)  # (the state alone is asked for: the stage runs fused and stores no divergence)
    assert c.deferred_stats()[:2] == (1, 0)
    with pytest.raises(hfx.HfxError, match=STALE_DIV):
        e.sample_history(0.0, 0)
    assert e.history_count() == 0
    calc_residual_calls([e], faces, True, 1)
    e.AdvanceSolution(1, 3)
    e.sample_history(0.0, 0)  # (a pending stage: the need mask makes it store the divergence, still fused)
    assert e.history_count() == 1 and c.deferred_stats()[:2] == (2, 0)
    res = e.read_history()[2][:, 0]
    old = np.array([e.compute_res_upts(2, f) for f in range(e.n_fields)])
    assert np.all(np.abs(res - old) <= 1e-13 * old)
    close(e, faces)
    c.close()


# ---- 5. NaN ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [0, 1, 2])
def test_nan_residual(ctx, norm):
    """one solution value NaN before a one-step loop: the row's residuals are NaN whatever the norm (data only, no fault)"""
    s = setup("hr_hex_p2_euler")
    e, faces = build(ctx, s["d"])
    u = s["d"]["u_init"].copy(order="F")
    u[3, 5, 0] = np.nan
    e.upload(hfx.DISU_UPTS0, u)
    ctx.set_history_monitor(norm, False, 1, 1)
    ctx.set_clock(0.0, 0)
    hfx.run_steps(e, faces, 1, fused=0)
    res = e.read_history()[2]
    assert np.all(np.isnan(res[:, 0]))
    close(e, faces)


def test_nan_through_the_mirror():
    d = HU.load("hr_hex_p2_euler")
    c, meta = bdy_util.case_from_fixture(d)
    c.set_monitor_res_freq(1, 0)
    c.set_history(0, 2)
    c.to_device(0)
    ctx, e = c.handles()[:2]
    u = np.asfortranarray(d["u_init"].copy(order="F"))
    u[3, 5, 0] = np.nan
    hfx.check(hfx.lib().hfx_eles_upload(e, C.c_int(hfx.DISU_UPTS0), u.ctypes.data_as(hfx.dp)))
    c.run(1)
    with pytest.raises(hfx.HfxError, match="NaN residual encountered. Exiting"):
        c.read_history()
    c.close()


# ---- 6. through the host mirror -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [True, False])
@pytest.mark.parametrize("name", ["hr_hex_p2_rk45", "hr_hex_p2_euler", "hr_hex_p2_norm0", "hr_hex_p2_norm1", "hr_quad_p3_walls",
                                  "hr_hex_p2_walls", "hr_hex_p2_forced"])
def test_mirror_rows_vs_the_driver(name, deferred):
    """hfxh_case_run with deferred execution on and off: hfxh_case_read_history gives every column of every row of the driver"""
    s = setup(name)
    d = s["d"]
    c, meta = mirror_case(d, **(dict(body_forcing=1) if s["forced"] else {})) if s["forces"] else bdy_util.case_from_fixture(d)
    n_diag = d["hist_diag"].shape[1]
    if n_diag:
        c.set_integral_quantities([IU.NAMES[int(i)] for i in np.ravel(d["integral_quantity_ids"])])
    c.set_monitor_res_freq(s["freq"], 4 if n_diag else 0)
    c.set_history(s["norm"], 4)
    c.set_deferred(deferred)
    c.to_device(0)
    # (more rows than the histories hold: refused before the first launch, by the integral monitor's check where both are registered)
    with pytest.raises(hfx.HfxError, match="%s monitor: 400 steps" % ("integral" if n_diag else "history")):
        c.run(400)
    assert c.history_count() == 0
    c.run(meta["steps"])
    assert c.history_count() == len(d["hist_iter"])
    steps, rows = c.read_history()
    nf, nd = c.n_fields, c.n_dims
    nq = nd + 2 if s["forces"] else 0
    assert rows.shape == (nf + nq + n_diag + 1, len(d["hist_iter"])) and list(steps) == [int(v) for v in d["hist_iter"]]
    assert c.history_count() == 0 and (not n_diag or c.integral_count() == 0)
    for k in range(len(steps)):
        what = "%s mirror deferred %d row at step %d" % (name, deferred, steps[k])
        miss = HU.log_miss(rows[:nf, k], d["hist_res"][k])
        print("%s: residual columns %.3f bars" % (what, miss))
        assert miss <= 1.0, what
        if nq:
            miss = HU.value_miss(rows[nf:nf + nq, k], d["hist_force"][k], np.abs(d["hist_force"][k]).max())
            print("%s: force columns %.3f bars of the row's own size" % (what, miss))
            assert miss <= 1.0, what
        if n_diag:
            assert HU.value_miss(rows[nf + nq:nf + nq + n_diag, k], d["hist_diag"][k], np.abs(d["hist_diag"][k]).max()) <= 1.0, what
        assert abs(rows[-1, k] - d["hist_time"][k]) <= 1e-14 * d["hist_time"][k], what
    c.close()


@pytest.mark.parametrize("name", ["hr_hex_p2_norm0", "hr_hex_p2_norm1", "hr_hex_p2_rk45", "hr_hex_p2_forced"])
def test_mirror_CalcNormResidual(name):
    """hfxh_case_CalcNormResidual behind one step -- eles::compute_res_upts per class and field, the max or the sums, the finish --
    is the driver's row 1 for res_norm_type 0, 1 and 2 and with a source term; hfxh_case_sample_history then stores the loop's row
    again, bit for bit"""
    s = setup(name)
    d = s["d"]
    c, meta = mirror_case(d, **(dict(body_forcing=1) if s["forced"] else {})) if s["forces"] else bdy_util.case_from_fixture(d)
    c.set_monitor_res_freq(1, 0)
    c.set_history(s["norm"], 3)
    c.set_deferred(False)
    c.to_device(0)
    with pytest.raises(hfx.HfxError, match="history is full|no residual"):
        for _ in range(4):
            c.sample_history()
    c.set_history(s["norm"], 3)  # (registering again empties the histories)
    assert c.history_count() == 0
    c.run(1)
    norm = c.CalcNormResidual()
    miss = HU.log_miss(np.log10(norm), d["hist_res"][0])
    print("%s: CalcNormResidual against the driver's row 1: %.3f bars" % (name, miss))
    assert miss <= 1.0
    c.sample_history()
    steps, rows = c.read_history()
    assert list(steps) == [1, 1] and np.array_equal(rows[:, 0], rows[:, 1])
    assert HU.log_miss(rows[:c.n_fields, 0], np.log10(norm)) <= 1.0
    c.close()


@pytest.mark.parametrize("norm", [0, 1, 2])
def test_mirror_CalcNormResidual_nan(norm):
    d = HU.load("hr_hex_p2_euler")
    c, meta = bdy_util.case_from_fixture(d)
    c.set_history(norm, 0)
    c.set_deferred(False)
    c.to_device(0)
    e = c.handles()[1]
    u = np.asfortranarray(d["u_init"].copy(order="F"))
    u[3, 5, 0] = np.nan
    hfx.check(hfx.lib().hfx_eles_upload(e, C.c_int(hfx.DISU_UPTS0), u.ctypes.data_as(hfx.dp)))
    c.run(1)
    with pytest.raises(hfx.HfxError, match="NaN residual encountered. Exiting"):
        c.CalcNormResidual()
    c.close()


# ---- 7. partitioned -------------------------------------------------------------------------------------------------------------------
WALLS = dict(bcs=[dict(type="isotherm_wall", T_static=310.0, u=3.0)], sides={"y-": 0, "y+": 0})
MIRROR_CFG = dict(order=2, amp=0.05, T_c_ic=300.0, dt=1e-4, riemann_solve_type=3)


def _partitioned_worker(rank, world, port, outdir):
    import faulthandler
    faulthandler.enable()
    import torch
    torch.cuda.set_device(0)
    dist = PU.init_pg(rank, world, port, "gloo")
    try:
        for tag, part, walls in (("one_res", False, False), ("part_res", True, False), ("one_frc", False, True), ("part_frc", True, True),
                                 ("one_max", False, False), ("part_max", True, False)):
            kw = dict(self_partition=[1, 0, 0]) if part else {}
            if walls:
                kw.update(WALLS, calc_force=1, area_ref=1.0)
            c = H.Case([4, 4, 4], length=6.2831853071795862, **kw, **MIRROR_CFG)
            c.set_monitor_res_freq(2, 0)
            c.set_history(0 if tag.endswith("max") else 2, 4)  # (norm 0: the MAX reduction over the communicator's ranks)
            c.to_device(0)
            if not part:
                c.run(5)
            else:
                c.set_comm(hfx.comm_unique_id())
                if walls:
                    # a variant-3 plan keeps the gradient on chip: refused before the first launch, the case as it was
                    ctx, e = c.handles()[:2]
                    u0 = np.zeros((c.n_upts, c.n_eles, c.n_fields), order="F")
                    hfx.check(hfx.lib().hfx_eles_download(e, C.c_int(hfx.DISU_UPTS0), u0.ctypes.data_as(hfx.dp)))
                    try:
                        c.run_partitioned(5)
                        msg = ""
                    except hfx.HfxError as err:
                        msg = str(err)
                    u1 = np.zeros_like(u0)
                    hfx.check(hfx.lib().hfx_eles_download(e, C.c_int(hfx.DISU_UPTS0), u1.ctypes.data_as(hfx.dp)))
                    np.save(os.path.join(outdir, "refused.npy"), np.array([("fused mode 2" in msg) and ("residuals alone" in msg),
                                                                          np.array_equal(u0, u1), c.history_count() == 0]))
                    hfx.check(hfx.lib().hfx_ctx_set_fused_mode(ctx, C.c_int(2)))  # (variant 2 writes the gradient in every stage)
                c.run_partitioned(5)
            st, rows = c.read_history()
            np.save(os.path.join(outdir, tag + "_s.npy"), st)
            np.save(os.path.join(outdir, tag + "_v.npy"), rows)
            c.close()
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_partitioned_loop(tmp_path):
    """one self-partitioned rank through hfx_run_steps_partitioned (RCCL loop-back), as tests/test_gpu_integral_history.py does:
    with residuals alone the rows of the undivided case; with viscous wall forces a variant-3 plan is refused before its first
    launch and fused mode 2 gives the undivided rows.  log10 columns to 1e-11 on the norm, forces to 1e-11 of the row's largest."""
    from test_gpu_time_average import spawn_with_time_limit
    spawn_with_time_limit(_partitioned_worker, (str(tmp_path),), 240)
    get = lambda tag, k: np.load(str(tmp_path / ("%s_%s.npy" % (tag, k))))
    assert list(np.load(str(tmp_path / "refused.npy"))) == [True, True, True]
    for kind in ("res", "frc", "max"):
        one, part = get("one_" + kind, "v"), get("part_" + kind, "v")
        assert list(get("one_" + kind, "s")) == [1, 2, 4] == list(get("part_" + kind, "s")) and one.shape == part.shape
        assert np.array_equal(one[-1], part[-1])  # the times
        assert HU.log_miss(part[:5], one[:5]) <= 1.0
        if kind == "frc":
            assert one.shape[0] == 5 + 5 + 1 and np.all(np.abs(part[5:10] - one[5:10]) <= 1e-11 * np.abs(one[5:10]).max(axis=0))
            assert np.any(one[5:8] != 0)
