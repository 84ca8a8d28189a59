"""The plot monitor on the device (hfx_ctx_set_plot_monitor, hfx_eles_sample_plot, hfx_eles_read_plot_snapshots,
hfx_eles_calc_plot_fields) inside every step loop, against the genuine DRIVER's Tecplot rows (tests/golden/plot_rows/pr_*.npz;
tools/capture_plot_rows.py).  Bars: those of tests/plot_rows_util.py -- 1e-11 of the column's un-cancelled scale plus 1e-14 of the
value for the printed digits (scaled_q_criterion: plot_rows_util.bars); the scales come from the numpy restatement through the
oracle, stepped once per fixture on the CPU."""
import json

import numpy as np
import pytest

import hfx
import plot_rows_util as PU
from test_gpu_methods_vs_golden import build
from test_plot_rows_host import snapshots

pytestmark = pytest.mark.gpu

STALE = "was not materialised by the fused stage that ran last"


@pytest.fixture()
def ctx():
    c = hfx.Context(0)
    yield c
    c.close()


def close(e, faces):
    for f in faces:
        f.close()
    e.close()


def n_steps_of(d):
    return json.loads(bytes(d["meta_json"]).decode())["steps"]


def setup(ctx, d, diag=None, capacity=4, clock=True):
    """the fixture's block with its plot points, average fields and monitor"""
    e, faces = build(ctx, d)
    e.set_opp_p(d["opp_p"])
    avg = PU.names_of(d, "average_fields")
    if avg:
        e.set_average_fields(avg)
    if diag is not False:
        ctx.set_plot_monitor(PU.names_of(d, "diagnostic_fields") if diag is None else diag, plot_freq=int(d["plot_freq"][0]), capacity=capacity)
    if clock:
        ctx.set_clock(0.0, 0)
    return e, faces


def run_loop(e, faces, n, fused):
    if fused == 4:
        hfx.run_steps_blocks([e], faces, n, fused=4)
    else:
        hfx.run_steps(e, faces, n, fused=fused)


def check_rows(name, steps, values, what):
    """the snapshots against the driver's rows behind the position; prints the largest miss per column in bars"""
    d, diag, avg, snaps = snapshots(name)
    n_dims = int(d["sizes"][4])
    assert list(steps) == [int(v) for v in d["plot_iter"]], what
    worst = np.zeros(values.shape[2])
    for k in range(len(steps)):
        worst = np.maximum(worst, PU.miss(PU.rows_of(values[..., k]), d["plot_rows"][k][:, n_dims:], snaps[k][1]))
    print("%s: %s bars" % (what, np.array2string(worst, precision=3)))
    assert np.all(worst <= PU.bars(d)), (what, worst)


LOOPS = [(n, f) for n in PU.PR[:5] for f in (0, 2, 3)] + [("pr_tet_p2_rk45", 0), ("pr_tet_p2_rk45", 4)]


@pytest.mark.parametrize("name,fused", LOOPS)
def test_loop_rows_vs_the_driver(ctx, name, fused):
    """the clock set to 0, the monitor with the fixture's fields and plot_freq, ONE call of the fixture's steps: the loop takes the
    driver's rows.  On a plan that keeps the gradient on chip (fused 3, 4) the last stage of a sampled step runs call by call when a
    field reads the gradient; whichever way the last stage ran, the gradient is marked accordingly when the loop returns."""
    d = PU.load(name)
    e, faces = setup(ctx, d)
    n = n_steps_of(d)
    run_loop(e, faces, n, fused)
    assert ctx.get_clock()[1] == n and e.plot_count() == len(d["plot_iter"])
    times, steps, values = e.read_plot_snapshots()
    assert np.allclose(times, PU.scalar(d, "dt") * np.array(steps), rtol=1e-14, atol=0)
    check_rows(name, steps, values, "%s fused %d" % (name, fused))
    reads = PU.reads_gradient(PU.names_of(d, "diagnostic_fields"))
    last_sampled = int(d["plot_iter"][-1]) == n
    if fused in (3, 4) and reads and not last_sampled:
        # pr_hex_p2_rk45 ends on step 5, which is not sampled: its gradient stayed on chip, and is refused, never read stale
        with pytest.raises(hfx.HfxError, match=STALE):
            e.sample_plot(0.0, n)
        with pytest.raises(hfx.HfxError, match=STALE):
            e.calc_plot_fields()
    else:
        # the same kernel on demand: bit for bit the in-loop snapshot of the same step
        again = e.calc_plot_fields()
        if last_sampled:
            assert np.array_equal(again, values[..., -1])
        e.sample_plot(0.0, n)
        e.sample_plot(0.0, n)
        _, _, twice = e.read_plot_snapshots()
        assert np.array_equal(twice[..., 0], again) and np.array_equal(twice[..., 1], again)
    close(e, faces)


@pytest.mark.parametrize("name", ["pr_hex_p2_rk45", "pr_quad_p3_walls"])
def test_fused_state_with_and_without_the_monitor(name):
    """with gradient-free fields a fused 3 loop launches what it launched before: the state is bit-equal to the unmonitored loop's;
    with a gradient field the sampled steps end call by call and the state stays within 1e-12, the bar the integral monitor's tests
    grant the same rule"""
    d = PU.load(name)
    out = {}
    for what, diag in (("none", False), ("free", ["u", "mach", "pressure", "energy"]), ("all", None)):
        c = hfx.Context(0)
        e, faces = setup(c, d, diag=diag)
        hfx.run_steps(e, faces, n_steps_of(d), fused=3)
        out[what] = e.download(hfx.DISU_UPTS0)
        assert e.plot_count() == (0 if diag is False else len(d["plot_iter"]))
        if what == "free":  # (the gradient was never materialised, and never asked for)
            e.sample_plot(0.0, 0)
        close(e, faces)
        c.close()
    assert np.array_equal(out["free"], out["none"])
    err = np.abs(out["all"] - out["none"]).max() / np.abs(out["none"]).max()
    print("%s: state with the monitor against without %.3e" % (name, err))
    assert err <= 1e-12


@pytest.mark.parametrize("fused", [0, 3])
def test_capacity_is_checked_before_the_first_launch(ctx, fused):
    d = PU.load("pr_hex_p2_pres5")
    e, faces = setup(ctx, d, capacity=1)
    u0 = e.download(hfx.DISU_UPTS0)
    with pytest.raises(hfx.HfxError, match="take 2 snapshots"):
        hfx.run_steps(e, faces, 2, fused=fused)
    assert ctx.get_clock()[:2] == (0.0, 0) and e.plot_count() == 0
    assert np.array_equal(e.download(hfx.DISU_UPTS0), u0)
    hfx.run_steps(e, faces, 1, fused=fused)
    with pytest.raises(hfx.HfxError, match="take 1 snapshots"):
        hfx.run_steps(e, faces, 1, fused=fused)
    _, steps, values = e.read_plot_snapshots()
    assert list(steps) == [1] and e.plot_count() == 0
    dd, _, _, snaps = snapshots("pr_hex_p2_pres5")
    assert np.all(PU.miss(PU.rows_of(values[..., 0]), dd["plot_rows"][0][:, 3:], snaps[0][1]) <= PU.bars(dd))
    close(e, faces)


def test_on_chip_gradient_is_refused_after_a_fused_stage(ctx):
    """without the library's clock the loop takes no snapshot and fused 3 keeps the gradient on chip: a monitor with a gradient field
    is refused, one with gradient-free fields samples"""
    d = PU.load("pr_hex_p2_rk45")
    e, faces = setup(ctx, d, clock=False)
    hfx.run_steps(e, faces, 2, fused=3)
    assert e.plot_count() == 0
    with pytest.raises(hfx.HfxError, match=STALE):
        e.sample_plot(0.0, 2)
    assert e.plot_count() == 0
    ctx.set_plot_monitor(["mach", "sensor"], plot_freq=1, capacity=1)
    e.sample_plot(0.0, 2)
    assert e.plot_count() == 1
    close(e, faces)


# ---- through the host mirror ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [True, False])
@pytest.mark.parametrize("name", PU.PR[:5])
def test_mirror_rows_vs_the_driver(name, deferred):
    """hfxh_case_run on the fixture's mesh and input with deferred execution on and off: the rows of hfxh_case_read_plot_rows are the
    driver's, position (eles::calc_pos_ppts) included.  Deferred, the sample's need mask makes the pending last stage run call by
    call where a field reads the gradient, and only that stage; with gradient-free fields every stage runs fused."""
    import bdy_util
    d = PU.load(name)
    diag, avg = PU.names_of(d, "diagnostic_fields"), PU.names_of(d, "average_fields")
    c, meta = bdy_util.case_from_fixture(d, p_res=int(d["p_res"][0]))
    if avg:
        c.set_average_fields(avg)
    c.set_diagnostic_fields([n.upper() for n in diag])  # (lower-cased as src/input.cpp:125-129 does)
    c.set_plot(int(d["plot_freq"][0]), 4)
    c.set_deferred(deferred)
    bars = PU.mirror_bars(name, d, c)  # (1, but for scaled_q_criterion: measured on the CPU with the mirror's own arrays)
    c.to_device(0)
    c.sync_host()
    assert np.abs(c.array("disu_upts0") - d["u_init"]).max() <= 1e-13 * np.abs(d["u_init"]).max()  # (the mirror's initial state is the fixture's)
    with pytest.raises(hfx.HfxError, match="plot monitor: 400 steps"):
        c.run(400)  # (more snapshots than the history holds: refused before the first launch)
    assert c.plot_count() == 0
    c.run(meta["steps"])
    assert c.plot_count() == len(d["plot_iter"])
    times, steps, rows = c.read_plot_rows()
    n_dims = int(d["sizes"][4])
    _, _, _, snaps = snapshots(name)
    assert list(steps) == [int(v) for v in d["plot_iter"]] and c.plot_count() == 0
    for k in range(len(steps)):
        drv = d["plot_rows"][k]
        m = PU.miss(rows[k][:, n_dims:], drv[:, n_dims:], snaps[k][1])
        pos = np.abs(rows[k][:, :n_dims] - drv[:, :n_dims]).max() / np.abs(drv[:, :n_dims]).max()
        print("%s mirror deferred %d file %d: %s bars, position %.2e" % (name, deferred, steps[k], np.array2string(m, precision=3), pos))
        assert np.all(m <= bars), (k, m, bars)
        assert pos <= 1e-13 + 1e-14  # (the mirror's shape functions against the reference's, and the printed digits)
        assert abs(times[k] - PU.scalar(d, "dt") * steps[k]) <= 1e-14 * times[k]
    if deferred:
        c.synchronize()
        n_fused, n_replayed, why = hfx.deferred_stats(c.handles()[0])
        print("%s: %d stages fused, %d replayed (%s)" % (name, n_fused, n_replayed, why))
        n_stages = int(d["sizes"][7]) * meta["steps"]
        if not PU.reads_gradient(diag):
            assert n_replayed == 0 and n_fused == n_stages, why
        elif name == "pr_hex_p2_rk45":  # (periodic: nothing else asks for a replay -- only the sampled steps' last stages)
            assert (n_fused, n_replayed) == (n_stages - len(steps), len(steps)), why
        else:
            assert n_replayed >= len(steps)
    c.close()


def test_mirror_reports_a_nan_as_the_reference_does():
    import bdy_util
    d = PU.load("pr_quad_p3_walls")
    c, meta = bdy_util.case_from_fixture(d, p_res=2)
    c.set_diagnostic_fields(["pressure", "mach"])
    c.set_plot(1, 2)
    with pytest.raises(hfx.HfxError, match="plot_quantity not recognized"):
        c.set_diagnostic_fields(["pressure", "enstrophy"])
    c.to_device(0)
    with pytest.raises(hfx.HfxError, match="Q criterion Not implemented in 2D"):
        c.set_diagnostic_fields(["q_criterion"])
        c.sample_plot()
    c.set_diagnostic_fields(["pressure", "mach"])
    ctx, e = c.handles()[:2]
    u = np.array(c.array("disu_upts0"), order="F")
    u[:, 2, 3] = -1.0  # a negative energy in element 2: a negative pressure, the Mach number a NaN
    hfx.check(hfx.lib().hfx_eles_upload(e, hfx.DISU_UPTS0, u.ctypes.data_as(hfx.dp)))
    c.sample_plot()
    with pytest.raises(hfx.HfxError, match="plot_quantitiy mach: NaN"):
        c.read_plot_rows()
    c.close()


# ---- partitioned ----------------------------------------------------------------------------------------------------------------------
MIRROR_CFG = dict(order=2, amp=0.05, T_c_ic=300.0, dt=1e-4, riemann_solve_type=3)
PART_FIELDS = ["u", "pressure", "vorticity", "q_criterion"]


def _partitioned_worker(rank, world, port, outdir):
    import ctypes as C
    import faulthandler
    import os
    faulthandler.enable()
    import torch
    import hfx_host as H
    import partition_util
    torch.cuda.set_device(0)
    dist = partition_util.init_pg(rank, world, port, "gloo")
    try:
        for tag, part in (("one", False), ("part", True)):
            kw = dict(self_partition=[1, 0, 0]) if part else {}
            c = H.Case([4, 4, 4], length=6.2831853071795862, **kw, **MIRROR_CFG)
            c.set_diagnostic_fields(PART_FIELDS)
            c.set_plot(2, 4)
            c.to_device(0)
            if not part:
                c.run(5)
            else:
                c.set_comm(hfx.comm_unique_id())
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
                np.save(os.path.join(outdir, "refused.npy"), np.array([("fused mode 2" in msg) and ("plot monitor" in msg),
                                                                      np.array_equal(u0, u1), c.plot_count() == 0]))
                hfx.check(hfx.lib().hfx_ctx_set_fused_mode(ctx, C.c_int(2)))  # (variant 2 writes the gradient in every stage)
                c.run_partitioned(5)
            t, s, rows = c.read_plot_rows()
            np.save(os.path.join(outdir, tag + "_t.npy"), t)
            np.save(os.path.join(outdir, tag + "_s.npy"), s)
            np.save(os.path.join(outdir, tag + "_rows.npy"), rows)
            c.close()
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_partitioned_loop(tmp_path):
    """one self-partitioned rank through hfx_run_steps_partitioned (RCCL loop-back), as tests/test_gpu_integral_history.py does: with a
    gradient field a variant-3 plan is refused before its first launch and names the remedy; fused mode 2 gives the undivided case's
    rows within 1e-11 of every column's largest value"""
    from test_gpu_time_average import spawn_with_time_limit
    spawn_with_time_limit(_partitioned_worker, (str(tmp_path),), 240)
    get = lambda tag, k: np.load(str(tmp_path / ("%s_%s.npy" % (tag, k))))
    assert list(np.load(str(tmp_path / "refused.npy"))) == [True, True, True]
    one, part = get("one", "rows"), get("part", "rows")
    assert list(get("one", "s")) == [2, 4] == list(get("part", "s"))
    assert np.array_equal(get("one", "t"), get("part", "t"))
    assert one.shape == part.shape == (2, 64 * 8, 3 + 5 + len(PART_FIELDS))
    err = np.abs(part - one).max(axis=(0, 1)) / np.abs(one).max(axis=(0, 1))
    print("partitioned against undivided, per column: %s" % np.array2string(err, precision=2))
    assert np.all(err <= 1e-11)
