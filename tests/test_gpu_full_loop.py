"""Every per-step duty at once in every step loop: the body force, the time averages, the probes, the integral quantities, the
history rows and the plot snapshots registered TOGETHER on one context whose clock starts at (0, 0), history and plot monitor at
different frequencies, against what the genuine driver wrote in one such run (tests/golden/full_loop/fl_*.npz;
tools/capture_full_loop.py) and the numpy restatements in lockstep (tests/full_loop_util.py).  Never against another device path,
except where two device runs must be bit-equal.

Bars, all from the existing utilities: a residual column 1e-11 on the norm plus the printed digits (history_rows_util.log_miss); force
columns 1e-11 of their un-cancelled scale, the integral columns 1e-11 of the row's largest (value_miss); plot columns 1e-11 of the
column's un-cancelled scale (plot_rows_util.miss, bars); probes 1e-11 of the field's largest magnitude over the probes
(full_loop_util); the controller 1e-7 of the driver's printed 8 digits; the averages 1e-11 of each plane's largest value; the state
1e-11 of its largest value.  What each run prints: the worst of each in units of its bar.

Triangles (fl_tri_p3_walls, fl_tri_p3_shock: 40 P3 triangles, one whole group of the fused 2-D simplex stage and a ragged one) run the
per-method loop and fused 4; every fused-4 run asserts hfx_simplex2d_plan, the shock case that the filter is folded.  Their probes sit
at plot points, so a sample on the step of a plot file is also held against the driver's rows there ("probes on plot rows").

The plan of a P2 block reports neither folded faces nor the two-wave flux kernel (both are forms of P4 hexahedra on affine blocks,
tests/test_gpu_folded_faces.py, tests/test_gpu_flux_two_wave.py): the legs with fold_faces 0 and flux_two_wave 0 are left out.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import full_loop_util as FU
import hfx
import history_rows_util as HU
import plot_rows_util as PU
from test_gpu_deferred_interleaved import is_current
from test_gpu_methods_vs_golden import build

pytestmark = pytest.mark.gpu

HEX, DRIVEN, QUAD, TET, TRI, TRI_SHOCK = FU.FL
HISTORIES = ["probes", "integral", "history", "plot"]
G_P3 = 32  # (elements per group of the fused 2-D simplex stage at P3: the 40 triangles are one whole group and a ragged one of 8)


@functools.lru_cache(maxsize=None)
def setup(name):
    """the fixture, the lockstep walk, the wall faces and inflow faces the host mirror builds (no device), the probes; made once,
    left unchanged"""
    d, w = FU.reference(name)
    s = dict(name=name, d=d, w=w, meta=FU.meta_of(d), steps=FU.meta_of(d)["steps"], F=FU.force_setup(d), P=FU.probes(name),
             norm=int(d["res_norm_type"][0]), freq=int(d["monitor_res_freq"][0]), plot_freq=int(d["plot_freq"][0]),
             ids=[int(v) for v in np.ravel(d["integral_quantity_ids"])], diag=PU.names_of(d, "diagnostic_fields"),
             avg=PU.names_of(d, "average_fields"), forcing=HU.forcing_of(d) if FU.forced(d) else None,
             probe_steps=FU.expected_probes(name)[0], probe_values=FU.expected_probes(name)[1])
    s["need"] = dict(probes=len(s["probe_steps"]), integral=len(d["hist_iter"]), history=len(d["hist_iter"]), plot=len(d["plot_iter"]))
    s["free_diag"] = [n for n in s["diag"] if n not in PU.GRADIENT]
    s["tri"], s["shock"] = int(d["sizes"][6]) == FU.TRIANGLES, FU.shock(d)
    return s


def register(ctx, e, s, monitors="all", caps=None):
    """every duty of the case; monitors "free": the subset that reads no gradient -- residuals without forces, kinetic energy alone,
    the plot fields without vorticity and Q; "none": averages, probes and the body force alone stay off too"""
    d, P = s["d"], s["P"]
    caps = dict(s["need"], **(caps or {}))
    e.set_opp_p(d["opp_p"])
    if s["F"] is not None:
        A = s["F"]["A"]
        ctx.set_force_reference(**s["F"]["ref"])
        e.set_wall_faces(A["face_ele"], A["face_inter"], A["face_flag"], A["opp"], A["weight"], A["detjac"], A["norm"])
    if s["forcing"] is not None:  # (the driver ran with body_forcing 1: the reference's hard-coded area and mass flux)
        s["forcing"].register(e, HU.FORCING_MDOT0)
    e.set_volume_cubpts(d["opp_volume_cubpts"], d["weight_volume_cubpts"], d["vol_detjac_vol_cubpts"])
    if monitors != "none":
        free = monitors == "free"
        if s["avg"]:
            e.set_average_fields(s["avg"])
        ctx.set_history_monitor(s["norm"], s["F"] is not None and not free, s["freq"], capacity=caps["history"])
        ctx.set_integral_monitor([0] if free else s["ids"], monitor_res_freq=s["freq"], capacity=caps["integral"])
        ctx.set_plot_monitor(s["free_diag"] if free else s["diag"], plot_freq=s["plot_freq"], capacity=caps["plot"])
        ctx.set_probes(P["names"], probe_freq=FU.PROBE_FREQ[s["name"]], capacity=caps["probes"])
        e.set_probes(P["ele"][P["perm"]], P["opp"][:, P["perm"]])  # (a scrambled order)
    ctx.set_clock(0.0, 0)


def make(ctx, s, monitors="all", caps=None):
    e, faces = build(ctx, s["d"])
    e.triangles, e.folds_shock, e.fixture = s["tri"], s["shock"], s["d"]
    register(ctx, e, s, monitors, caps)
    return e, faces


def assert_simplex_stage(e):
    """a block of triangles behind a fused-4 call: the 2-D simplex stage prepared it (the query is refused otherwise), and where the
    block has shock capturing the filter is folded into its update kernel -- a silent per-method loop cannot pass"""
    from test_gpu_tris import expected_plan
    plan, want = e.simplex2d_plan(), expected_plan(e.fixture)
    assert plan["group"] == G_P3 and e.n_eles == G_P3 + 8
    assert all(plan[k] == want[k] for k in ("size_class", "group", "waves", "gather", "element_lds")), plan
    if e.folds_shock:
        assert e.simplex2d_shock_plan()["folded"] == 1
    else:
        assert plan == want, plan


def close(e, faces, ctx=None):
    for f in faces:
        f.close()
    e.close()
    if ctx is not None:
        ctx.close()


def run_loop(e, faces, n, fused):
    if fused == 4:
        hfx.run_steps_blocks([e], faces, n, fused=4)
        if getattr(e, "triangles", False):
            assert_simplex_stage(e)
    else:
        hfx.run_steps(e, faces, n, fused=fused)


def counts(e):
    return dict(probes=e.probe_count()[0], integral=e.integral_count(), history=e.history_count(), plot=e.plot_count())


def collect(ctx, e, s):
    """every history read once, the averages, the controller's rows, the state, the clock: in the form check() takes"""
    d = s["d"]
    nd, n_pts = e.n_dims, e.n_upts * e.n_eles
    t, st, res, frc = e.read_history()
    out = dict(hist_steps=st, hist_time=t * float(d["time_ref"][0]), hist_res=np.log10(HU.norm_residual(s["norm"], res, n_pts)),
               hist_force=np.concatenate([frc[:nd] + frc[nd:2 * nd], frc[2 * nd:]]))
    out["integ_time"], out["integ_steps"], out["integ"] = e.read_integral_history()
    out["plot_time"], out["plot_steps"], values = e.read_plot_snapshots()
    out["plot_rows"] = np.stack([PU.rows_of(values[..., k]) for k in range(values.shape[3])]) if values.shape[3] else np.zeros((0, 0, 0))
    out["probe_time"], out["probe_steps"], v = e.read_probes()
    out["probes"] = v[:, np.argsort(s["P"]["perm"]), :]  # (back from the order of registration)
    out["avg"] = e.download_average() if s["avg"] else None
    out["ctl"] = e.body_force_history()[:, [0, 2]] if s["forcing"] is not None else None
    out["u"] = e.download(hfx.DISU_UPTS0)
    out["clock"] = ctx.get_clock()
    return out


def check(s, got, what, free=False):
    """a run's results against the fixture and the lockstep restatements at the existing bars; free: the gradient-free subset of
    the monitors ran.  Prints and returns the worst miss of each kind in units of its bar"""
    d, w = s["d"], s["w"]
    nd, nf = int(d["sizes"][4]), int(d["sizes"][3])
    dt = w["dt"]
    worst = {}
    # history rows and their times
    assert list(got["hist_steps"]) == [int(v) for v in d["hist_iter"]], what
    for k, r in enumerate(w["hist"]):
        worst["residual"] = max(worst.get("residual", 0.0), HU.log_miss(got["hist_res"][:, k], d["hist_res"][k]))
        assert abs(got["hist_time"][k] - d["hist_time"][k]) <= 1e-14 * d["hist_time"][k], (what, k)
        if "force" in r and not free:
            worst["force"] = max(worst.get("force", 0.0), HU.value_miss(got["hist_force"][:, k], d["hist_force"][k], r["force_scale"]))
    # integral columns
    assert list(got["integ_steps"]) == [int(v) for v in d["hist_iter"]], what
    for k in range(len(w["hist"])):
        want = d["hist_diag"][k][[s["ids"].index(0)]] if free else d["hist_diag"][k]
        worst["integral"] = max(worst.get("integral", 0.0), HU.value_miss(got["integ"][:, k], want, np.abs(want).max()))
    # plot rows, average columns included
    assert list(got["plot_steps"]) == [int(v) for v in d["plot_iter"]], what
    cols = np.arange(len(w["plot"][0]["scales"]))
    if free:
        head = nf + len(s["avg"])
        cols = np.array(list(range(head)) + [head + i for i, n in enumerate(s["diag"]) if n not in PU.GRADIENT])
    for k, snap in enumerate(w["plot"]):
        m = PU.miss(got["plot_rows"][k], d["plot_rows"][k][:, nd:][:, cols], snap["scales"][cols]) / PU.bars(d)[cols]
        worst["plot"] = max(worst.get("plot", 0.0), float(m.max()))
        assert abs(got["plot_time"][k] - dt * snap["step"]) <= 1e-14 * got["plot_time"][k], (what, k)
    # probe samples and their steps
    assert list(got["probe_steps"]) == s["probe_steps"], what
    assert np.allclose(got["probe_time"], dt * np.array(s["probe_steps"]), rtol=1e-14, atol=0)
    worst["probes"] = max(FU.probe_miss(got["probes"], s["probe_values"])) / 1e-11
    # triangles: the probes sit at plot points, and where a probe sample and a plot file fall on one step the conserved state of the
    # samples is the DRIVER's rows at those points, at the plot bar
    on_rows = FU.probes_against_plot_rows(s["name"], got["probe_steps"], got["probes"])
    assert (on_rows is not None) == s["tri"], what
    if on_rows is not None:
        worst["probes on plot rows"] = on_rows
    # the controller against the lines the driver printed before every step (8 decimals)
    if got["ctl"] is not None:
        drv = d["driver_controller"][:, 3:]
        assert got["ctl"].shape == drv.shape, what
        worst["controller"] = float((np.abs(got["ctl"] - drv) / (1e-7 * np.abs(drv).max(axis=0) + 6e-9)).max())
    # the final averages, the final state
    if got["avg"] is not None:
        a = w["average"]
        worst["average"] = float(max(np.abs(got["avg"][:, :, i] - a[:, :, i]).max() / np.abs(a[:, :, i]).max() for i in range(a.shape[2]))) / 1e-11
    worst["state"] = float(np.abs(got["u"] - w["states"][-1]).max() / np.abs(w["states"][-1]).max()) / 1e-11
    # (i_steps counts from 1; the spinup latch is the time of step 1)
    assert got["clock"][1] == s["steps"] and abs(got["clock"][2] - dt) <= 1e-14 * dt, what
    print("%s: worst miss in bars: %s" % (what, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
    for k, v in worst.items():
        assert v <= 1.0, (what, k, v)
    return worst


def one_call(name, fused, monitors="all"):
    s = setup(name)
    ctx = hfx.Context(0)
    e, faces = make(ctx, s, monitors)
    run_loop(e, faces, s["steps"], fused)
    got = collect(ctx, e, s) if monitors != "none" else dict(u=e.download(hfx.DISU_UPTS0))
    close(e, faces, ctx)
    return got


@functools.lru_cache(maxsize=None)
def per_method_run(name):
    """the one-call fused 0 run the cuts are compared with bit for bit; made once, left unchanged"""
    return one_call(name, 0)


def same_bits(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]) for k in a if k != "clock") and a["clock"] == b["clock"]


# ---- 1. through the C ABI, one call of all steps ------------------------------------------------------------------------------
ONE_CALL = [(n, f) for n in (HEX, DRIVEN, QUAD) for f in (0, 2, 3)] + [(HEX, 4), (TET, 0), (TET, 4)] + \
    [(n, f) for n in (TRI, TRI_SHOCK) for f in (0, 4)]


@pytest.mark.parametrize("name,fused", ONE_CALL)
def test_one_call(name, fused):
    check(setup(name), per_method_run(name) if fused == 0 else one_call(name, fused), "%s fused %d, one call" % (name, fused))


# ---- 2. cut into calls -----------------------------------------------------------------------------------------------------------
CUTS = [(HEX, (2, 1, 4)), (HEX, (1,) * 7), (QUAD, (1, 4)), (DRIVEN, (1, 1))]


CUT_LEGS = [(n, c, f) for n, c in CUTS for f in (0, 3)] + [(TRI, c, f) for c in ((2, 3), (1,) * 5) for f in (0, 4)] + [(TRI_SHOCK, (1,) * 5, 4)]


@pytest.mark.parametrize("name,cut,fused", CUT_LEGS, ids=["%s-%s-%d" % (n, "+".join(map(str, c)), f) for n, c, f in CUT_LEGS])
def test_cut_into_calls(name, cut, fused):
    """i_steps carries across the calls and "step 1" happens once; the histories are read once at the end.  fused 0: every device
    result is the one-call run's, bit for bit (the per-method loop launches the same kernels either way).  fused 3, and fused 4 on the
    triangles: the fixture at the bars; in a cut into single steps the library's own report shows which form the step's last stage
    took.  On the triangles with shock capturing every step but the last ends call by call -- the per-method filter and a fresh
    extrapolation -- between stages of the folded kernel"""
    s = setup(name)
    ctx = hfx.Context(0)
    e, faces = make(ctx, s)
    by_calls = [c for _, _, c in FU.schedule(s["d"])]
    done = 0
    for n in cut:
        run_loop(e, faces, n, fused)
        done += n
        assert ctx.get_clock()[1] == done
        if fused in (3, 4) and n == 1:
            # behind a step whose last stage ran call by call the gradient is in memory; behind a fused one it stayed on chip, and a
            # download is refused.  A loop that quietly ran everything call by call would report 1 throughout
            assert is_current(e, hfx.GRAD_DISU_UPTS) == int(by_calls[done - 1]), (name, done)
            if not by_calls[done - 1]:
                with pytest.raises(hfx.HfxError):
                    e.download(hfx.GRAD_DISU_UPTS)
    if fused == 3 and name == HEX and set(cut) == {1}:
        assert [i + 1 for i, c in enumerate(by_calls) if c] == [1, 2, 3, 4, 6]
    got = collect(ctx, e, s)
    close(e, faces, ctx)
    what = "%s fused %d, calls of %s" % (name, fused, "+".join(map(str, cut)))
    if fused == 0:
        assert same_bits(got, per_method_run(name)), what
    check(s, got, what)


# ---- 3. against no monitors --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fused", [(HEX, 3), (QUAD, 3), (TRI, 4)], ids=[HEX, QUAD, TRI])
def test_state_with_and_without_the_duties(name, fused):
    """fused 3, and fused 4 on the triangles: with the monitors that read no gradient the loop launches what it launched before and
    the final state is bit-equal to a run without any; with the full set the sampled steps end call by call and the state agrees to
    1e-12, the bound of DESIGN 6i.  (Not the triangles with shock capturing: a sensor at its threshold may legitimately flip)"""
    s = setup(name)
    none, free, full = one_call(name, fused, "none"), one_call(name, fused, "free"), one_call(name, fused)
    check(s, free, "%s fused %d, gradient-free monitors" % (name, fused), free=True)
    assert np.array_equal(free["u"], none["u"])
    err = np.abs(full["u"] - none["u"]).max() / np.abs(none["u"]).max()
    print("%s: state with every duty against none %.3e" % (name, err))
    assert err <= 1e-12


# ---- 4. atomic refusal -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [0, 3, 4])
def test_a_call_one_history_refuses_leaves_everything_untouched(fused):
    """every history has room for the whole run but one, each in turn: the call is refused before any launch -- the clock, all four
    counts and the state are as they were -- and once that history has room the same context runs and meets the fixture.  fused 4: on
    the triangles"""
    name = TRI if fused == 4 else HEX
    s = setup(name)
    for which in HISTORIES:
        ctx = hfx.Context(0)
        e, faces = make(ctx, s, caps={which: s["need"][which] - 1} if s["need"][which] > 1 else None)
        if s["need"][which] == 1:
            # (one sample in the whole run: a capacity of 0 would drop the monitor; fill the history's only place by hand instead)
            assert which == "probes" or (name == TRI and which == "plot")
            if which == "probes":
                e.sample_probes(0.0, 0)
            else:  # (the triangles' one plot file; its vorticity reads a gradient: a residual of the initial state leaves one)
                hfx.CalcResidual(e, faces)
                e.sample_plot(0.0, 0)
        u0 = e.download(hfx.DISU_UPTS0)
        before = counts(e)
        with pytest.raises(hfx.HfxError):
            run_loop(e, faces, s["steps"], fused)
        assert ctx.get_clock()[:2] == (0.0, 0) and counts(e) == before, which
        assert np.array_equal(e.download(hfx.DISU_UPTS0), u0), which
        if s["avg"]:
            assert not e.download_average().any(), which
        # room for the whole run: registering a monitor again empties its history
        register(ctx, e, s)
        assert counts(e) == dict.fromkeys(HISTORIES, 0)
        run_loop(e, faces, s["steps"], fused)
        check(s, collect(ctx, e, s), "%s fused %d after a refusal by the %s history" % (name, fused, which))
        close(e, faces, ctx)


@pytest.mark.parametrize("fused", [0, 3, 4])
def test_a_refused_call_leaves_the_controller_untouched(fused):
    """the driven channel after its two steps, nothing read: a further call finds each history full in turn (the others read empty) and
    is refused before the controller evaluates -- its record, the clock, the counts, src_upts and the state are as they were.
    fused 4: the triangles after their five steps.  There is no driven triangle case (the reference's body force is three-dimensional,
    tools/capture_full_loop.py), so that leg has no controller: the clock, the counts, the averages and the state"""
    s = setup(TRI if fused == 4 else DRIVEN)
    driven = s["forcing"] is not None
    assert driven == (fused != 4)
    for which in HISTORIES:
        ctx = hfx.Context(0)
        e, faces = make(ctx, s)
        run_loop(e, faces, s["steps"], fused)
        for other in HISTORIES:
            if other != which:
                dict(probes=e.read_probes, integral=e.read_integral_history, history=e.read_history, plot=e.read_plot_snapshots)[other]()
        before, clock = counts(e), ctx.get_clock()
        u0, avg0 = e.download(hfx.DISU_UPTS0), e.download_average()
        if driven:
            state, src0, rows0 = e.body_force_state(), e.download(hfx.SRC_UPTS), e.body_force_history()
        assert before == {k: (s["need"][k] if k == which else 0) for k in HISTORIES}
        with pytest.raises(hfx.HfxError):
            run_loop(e, faces, 2, fused)  # (the next two steps: every monitor samples, and would have room had it been read)
        assert ctx.get_clock() == clock and counts(e) == before, which
        if driven:
            after = e.body_force_state()
            assert all(np.array_equal(state[k], after[k]) for k in state), which
            assert np.array_equal(e.body_force_history(), rows0) and np.array_equal(e.download(hfx.SRC_UPTS), src0), which
        assert np.array_equal(e.download(hfx.DISU_UPTS0), u0) and np.array_equal(e.download_average(), avg0), which
        close(e, faces, ctx)


# ---- 5. reading empties one history only -------------------------------------------------------------------------------------------
def test_reading_the_plot_snapshots_mid_run_leaves_the_other_histories():
    s = setup(HEX)
    ctx = hfx.Context(0)
    e, faces = make(ctx, s)
    run_loop(e, faces, 2, 3)
    run_loop(e, faces, 1, 3)
    before = counts(e)
    assert before == dict(probes=0, integral=2, history=2, plot=1)
    t0, s0, v0 = e.read_plot_snapshots()
    assert counts(e) == dict(before, plot=0) and list(s0) == [2]
    run_loop(e, faces, 4, 3)
    got = collect(ctx, e, s)
    got["plot_time"], got["plot_steps"] = np.concatenate([t0, got["plot_time"]]), np.concatenate([s0, got["plot_steps"]])
    got["plot_rows"] = np.concatenate([PU.rows_of(v0[..., 0])[None], got["plot_rows"]])
    close(e, faces, ctx)
    check(s, got, "%s fused 3, 2 + 1 + 4 with the plot snapshots read after 2 + 1" % HEX)


# ---- 6. through the host mirror ------------------------------------------------------------------------------------------------------
def mirror(s, monitors="all", **over):
    """the fixture's case through the host mirror with every duty of its input registered (no device yet)"""
    from test_wall_force_host import mirror_case
    d, P = s["d"], s["P"]
    free = monitors == "free"
    kw = dict(p_res=int(d["p_res"][0]), **over)
    if free:
        kw["calc_force"] = 0  # (the mirror's history row carries the wall forces whenever the case has calc_force)
    if s["forcing"] is not None:
        kw["body_forcing"] = 1
    c, _ = mirror_case(d, **kw)
    if s["avg"]:
        c.set_average_fields(s["avg"])
    c.set_diagnostic_fields(s["free_diag"] if free else s["diag"])
    c.set_plot(s["plot_freq"], s["need"]["plot"])
    import integral_history_util as IU
    c.set_integral_quantities([IU.NAMES[0]] if free else [IU.NAMES[i] for i in s["ids"]])
    c.set_monitor_res_freq(s["freq"], s["need"]["integral"])
    c.set_history(s["norm"], s["need"]["history"])
    c.set_probes(P["pos"][:, P["perm"]], P["names"], probe_freq=FU.PROBE_FREQ[s["name"]], capacity=s["need"]["probes"])
    return c


def collect_mirror(c, s, free=False):
    """hfxh_case_read_history, hfxh_case_read_plot_rows, the probe and average readers: in the form check() takes"""
    nf, nd = c.n_fields, c.n_dims
    nq = 0 if free else nd + 2
    st, rows = c.read_history()
    n_diag = 1 if free else len(s["ids"])
    assert rows.shape[0] == nf + nq + n_diag + 1
    out = dict(hist_steps=st, hist_res=rows[:nf], hist_force=rows[nf:nf + nq], integ=rows[nf + nq:nf + nq + n_diag], integ_steps=st,
               hist_time=rows[-1])
    out["plot_time"], out["plot_steps"], prow = c.read_plot_rows()
    out["plot_rows"], out["plot_pos"] = prow[:, :, nd:], prow[:, :, :nd]
    gi = c.probes()["global_index"]
    assert np.array_equal(c.probes()["p2c"], s["P"]["ele"][s["P"]["perm"]][gi])
    out["probe_time"], out["probe_steps"], v = c.read_probes()
    canon = np.zeros_like(v)
    canon[:, s["P"]["perm"][gi], :] = v  # (located probe j is the gi[j]-th registered, which is probe perm[gi[j]])
    out["probes"] = canon
    out["avg"] = c.averages() if s["avg"] else None
    out["ctl"] = c.body_force_history()[:, [0, 2]] if s["forcing"] is not None else None
    u = np.zeros((c.n_upts, c.n_eles, c.n_fields), order="F")
    hfx.check(hfx.lib().hfx_eles_download(c.handles()[1], C.c_int(hfx.DISU_UPTS0), u.ctypes.data_as(hfx.dp)))
    out["u"] = u
    out["clock"] = c.clock()
    return out


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("name", [HEX, DRIVEN, QUAD])
def test_host_mirror(name, deferred):
    """hfxh_case_run (RunSteps) with deferred execution off and on: the last stage of a step stays pending while five readers want it.
    Deferred, every stage runs fused but the last stage of each step a gradient-reading monitor samples, which is replayed call by
    call: the mirror announces the step's samples (hfx_flush_for_samples) before the averages and the probes, which read the state
    alone, make the pending stage run"""
    s = setup(name)
    c = mirror(s)
    c.set_deferred(deferred)
    c.to_device(0)
    c.run(s["steps"])
    got = collect_mirror(c, s)
    d = s["d"]
    pos = np.abs(got["plot_pos"] - d["plot_rows"][:, :, :c.n_dims]).max() / np.abs(d["plot_rows"][:, :, :c.n_dims]).max()
    assert pos <= 1e-13 + 1e-14  # (the mirror's shape functions against the reference's, and the printed digits)
    if deferred:
        c.synchronize()
        n_fused, n_replayed, why = hfx.deferred_stats(c.handles()[0])
        n_by_calls = sum(1 for _, _, b in FU.schedule(d) if b)
        print("%s mirror deferred: %d stages fused, %d records replayed (%s); %d steps end call by call"
              % (name, n_fused, n_replayed, why, n_by_calls))
        # (replays only where the one-stage rule asks for them: the last stage of every step that ends call by call, no other record)
        n_stages = int(d["sizes"][7]) * s["steps"]
        assert n_fused > 0 and (n_fused, n_replayed) == (n_stages - n_by_calls, n_by_calls), why
    c.close()
    check(s, got, "%s mirror deferred %d" % (name, deferred))


@pytest.mark.parametrize("announce", [False, True])
def test_the_first_reader_decides_how_a_pending_stage_runs(announce):
    """deferred execution through the C ABI, the calls of one RK45 step recorded: the time averages read the state alone, and behind
    them the pending last stage has run fused -- the integral sample of the same step is refused, never served an older gradient.
    With the step's samples announced first (hfx_flush_for_samples) that one stage is replayed call by call and the row is the driver's
    row of step 1"""
    from test_gpu_deferred import calc_residual_calls, tag
    s = setup(HEX)
    d, w = s["d"], s["w"]
    ctx = hfx.Context(0)
    ctx.set_option("deferred", 1)
    e, faces = make(ctx, s)
    tag(e, d)
    n_stages = int(d["sizes"][7])
    for rk in range(n_stages):
        calc_residual_calls([e], faces, True, rk)
        e.AdvanceSolution(rk, 3)
    dt = w["dt"]
    if announce:
        hfx.flush_for_samples([e], integrals=True, history=True, plot=True)
    e.CalcTimeAverageQuantities(dt, dt)
    if not announce:
        assert ctx.deferred_stats()[:2] == (n_stages, 0)
        with pytest.raises(hfx.HfxError, match="was not materialised by the fused stage that ran last"):
            e.sample_integral_quantities(dt, 1)
        assert e.integral_count() == 0
    else:
        e.sample_integral_quantities(dt, 1)
        e.sample_history(dt, 1)
        e.sample_plot(dt, 1)
        assert ctx.deferred_stats()[:2] == (n_stages - 1, 1), ctx.deferred_stats()[2]
        nd, r = e.n_dims, w["hist"][0]
        _, _, res, frc = e.read_history()
        log = np.log10(HU.norm_residual(s["norm"], res[:, 0], e.n_upts * e.n_eles))
        force = np.concatenate([frc[:nd, 0] + frc[nd:2 * nd, 0], frc[2 * nd:, 0]])
        integ = e.read_integral_history()[2][:, 0]
        miss = (HU.log_miss(log, d["hist_res"][0]), HU.value_miss(force, d["hist_force"][0], r["force_scale"]),
                HU.value_miss(integ, d["hist_diag"][0], np.abs(d["hist_diag"][0]).max()))
        print("row of step 1 behind the announced flush: residual %.3g, force %.3g, integral %.3g bars" % miss)
        assert max(miss) <= 1.0
        assert np.array_equal(e.download_average()[:, :, 0], e.download(hfx.DISU_UPTS0)[:, :, 0])  # (step 1: a = 0, b = 1)
    close(e, faces, ctx)


@pytest.mark.parametrize("announce", [False, True])
def test_the_first_reader_decides_how_a_pending_triangle_stage_runs(announce):
    """the triangle counterpart: the calls of one RK45 step on fl_tri_p3_walls with `deferred` 1, every whole stage planned as the 2-D
    simplex stage.  A probe sample and the time averages read the state alone: behind them the pending last stage has run fused, and
    the integral sample of the same step is refused, never served an older gradient.  With the step's samples announced first that
    one stage is replayed call by call, and the history row, the integral row and the wall forces are the driver's row of step 1.
    Either way the state is the lockstep's after step 1 and the probes are its probes"""
    from test_gpu_deferred import calc_residual_calls, tag
    s = setup(TRI)
    d, w = s["d"], s["w"]
    ctx = hfx.Context(0)
    ctx.set_option("deferred", 1)
    e, faces = make(ctx, s)
    tag(e, d)
    n_stages = int(d["sizes"][7])
    for rk in range(n_stages):
        calc_residual_calls([e], faces, True, rk)
        e.AdvanceSolution(rk, 3)
    dt = w["dt"]
    if announce:
        hfx.flush_for_samples([e], integrals=True, history=True, plot=True)
    e.sample_probes(dt, 1)
    e.CalcTimeAverageQuantities(dt, dt)
    if not announce:
        assert ctx.deferred_stats()[:2] == (n_stages, 0), ctx.deferred_stats()[2]
        with pytest.raises(hfx.HfxError, match="was not materialised by the fused stage that ran last"):
            e.sample_integral_quantities(dt, 1)
        with pytest.raises(hfx.HfxError):  # (the viscous wall forces read the same gradient)
            e.sample_history(dt, 1)
        assert e.integral_count() == 0 and e.history_count() == 0
    else:
        e.sample_integral_quantities(dt, 1)
        e.sample_history(dt, 1)
        e.sample_plot(dt, 1)
        assert ctx.deferred_stats()[:2] == (n_stages - 1, 1), ctx.deferred_stats()[2]
        nd, r = e.n_dims, w["hist"][0]
        _, _, res, frc = e.read_history()
        log = np.log10(HU.norm_residual(s["norm"], res[:, 0], e.n_upts * e.n_eles))
        force = np.concatenate([frc[:nd, 0] + frc[nd:2 * nd, 0], frc[2 * nd:, 0]])
        integ = e.read_integral_history()[2][:, 0]
        miss = (HU.log_miss(log, d["hist_res"][0]), HU.value_miss(force, d["hist_force"][0], r["force_scale"]),
                HU.value_miss(integ, d["hist_diag"][0], np.abs(d["hist_diag"][0]).max()))
        print("triangles, row of step 1 behind the announced flush: residual %.3g, force %.3g, integral %.3g bars" % miss)
        assert max(miss) <= 1.0
    assert_simplex_stage(e)
    assert np.array_equal(e.download_average()[:, :, 0], e.download(hfx.DISU_UPTS0)[:, :, 0])  # (step 1: a = 0, b = 1)
    probes = e.read_probes()[2][:, np.argsort(s["P"]["perm"]), :]
    assert s["probe_steps"][0] == 1
    miss = (max(FU.probe_miss(probes, s["probe_values"][:, :, :1])) / 1e-11,
            float(np.abs(e.download(hfx.DISU_UPTS0) - w["states"][0]).max() / np.abs(w["states"][0]).max()) / 1e-11)
    print("triangles deferred, announce %d: probes %.3g, state %.3g bars" % ((announce,) + miss))
    assert max(miss) <= 1.0
    close(e, faces, ctx)


# ---- 7. partitioned ---------------------------------------------------------------------------------------------------------------------
def _partitioned_worker(rank, world, port, outdir):
    import faulthandler
    faulthandler.enable()
    import torch
    import partition_util
    torch.cuda.set_device(0)
    dist = partition_util.init_pg(rank, world, port, "gloo")
    try:
        s = setup(HEX)
        for tag, monitors, mode in (("refused", "all", 3), ("free", "free", 3), ("full", "all", 2)):
            c = mirror(s, monitors, self_partition=[1, 0, 0])
            c.to_device(0)
            c.set_comm(hfx.comm_unique_id())
            ctx, e = c.handles()[:2]
            hfx.check(hfx.lib().hfx_ctx_set_fused_mode(ctx, C.c_int(mode)))
            if tag == "refused":
                # a variant-3 plan keeps the gradient on chip: refused before the first launch, the case as it was
                u0 = np.zeros((c.n_upts, c.n_eles, c.n_fields), order="F")
                hfx.check(hfx.lib().hfx_eles_download(e, C.c_int(hfx.DISU_UPTS0), u0.ctypes.data_as(hfx.dp)))
                try:
                    c.run_partitioned(s["steps"])
                    msg = ""
                except hfx.HfxError as err:
                    msg = str(err)
                u1 = np.zeros_like(u0)
                hfx.check(hfx.lib().hfx_eles_download(e, C.c_int(hfx.DISU_UPTS0), u1.ctypes.data_as(hfx.dp)))
                np.save(os.path.join(outdir, "refused.npy"),
                        np.array(["fused mode 2" in msg, np.array_equal(u0, u1), c.history_count() == 0, c.plot_count() == 0,
                                  c.integral_count() == 0, c.probe_count()[0] == 0, c.clock()[1] == 0]))
            else:
                c.run_partitioned(s["steps"])
                got = collect_mirror(c, s, free=monitors == "free")
                got["clock"] = np.array(got["clock"])
                np.savez(os.path.join(outdir, tag + ".npz"), **{k: v for k, v in got.items() if v is not None})
            c.close()
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_partitioned(tmp_path):
    """one self-partitioned rank through hfx_run_steps_partitioned (RCCL loop-back; the body-force-free channel cut at its x wrap-around
    faces): fused mode 2, the only mode in which the partitioned loops take gradient fields, meets the fixture's rows at the same
    bars; at fused mode 3 the gradient-reading monitors are refused before the loop starts and the gradient-free subset runs and
    meets its rows"""
    from test_gpu_time_average import spawn_with_time_limit
    s = setup(HEX)
    spawn_with_time_limit(_partitioned_worker, (str(tmp_path),), 240)
    assert list(np.load(str(tmp_path / "refused.npy"))) == [True] * 7
    for tag in ("free", "full"):
        got = dict(np.load(str(tmp_path / (tag + ".npz"))))
        got["clock"] = tuple(got["clock"])
        got.setdefault("ctl", None)
        got.setdefault("avg", None)
        check(s, got, "%s partitioned, %s" % (HEX, "fused mode 3, gradient-free monitors" if tag == "free" else "fused mode 2"),
              free=tag == "free")


REFUSALS = ["the history monitor samples the viscous wall forces", "the plot monitor has a field that reads grad_disu_upts",
            "the integral monitor has a quantity that reads grad_disu_upts"]


def test_partitioned_triangles():
    """fl_tri_p3_walls cut into three virtual parts of one rank (FU.TRI_PARTS: one partition group, one interior group) through
    hfx_run_steps_partitioned_blocks, whose stages keep the gradient on chip.  With the full monitor set the call is refused before the
    first launch, for the history monitor's wall forces first, then -- that monitor on the residuals alone -- for the plot monitor's
    vorticity, then for the integral monitor's enstrophy; each time the state, the clock, the averages and all four counts are as they
    were.  The gradient-free set then runs on the same blocks and meets the driver's rows"""
    from test_tris_partition_oracle import grow_parts, virtual_tables
    s = setup(TRI)
    d = s["d"]
    reg, L, Rlut, seg = virtual_tables(d, grow_parts(d, *FU.TRI_PARTS))
    ctx = hfx.Context(0)
    e, faces = build(ctx, reg)
    m = hfx.MpiInters(ctx, e, L, Rlut)
    m.set_neighbours(seg)
    comm = hfx.Comm(ctx.h, hfx.comm_unique_id(), 1, 0)
    register(ctx, e, s)
    u0 = e.download(hfx.DISU_UPTS0)
    for k, words in enumerate(REFUSALS):
        if k == 1:
            ctx.set_history_monitor(s["norm"], False, s["freq"], capacity=s["need"]["history"])
        if k == 2:
            ctx.set_plot_monitor(s["free_diag"], plot_freq=s["plot_freq"], capacity=s["need"]["plot"])
        with pytest.raises(hfx.HfxError, match=words):
            hfx.run_steps_partitioned_blocks([e], faces, [m], comm, s["steps"])
        assert ctx.get_clock()[:2] == (0.0, 0) and counts(e) == dict.fromkeys(HISTORIES, 0), words
        assert np.array_equal(e.download(hfx.DISU_UPTS0), u0) and not e.download_average().any(), words
    register(ctx, e, s, "free")
    hfx.run_steps_partitioned_blocks([e], faces, [m], comm, s["steps"])
    pp = e.simplex2d_partition_plan()
    assert (pp["partition_groups"], pp["interior_groups"]) == (1, 1), pp
    assert e.simplex2d_plan()["group"] == G_P3
    got = collect(ctx, e, s)
    comm.close()
    close(e, faces + [m], ctx)
    check(s, got, "%s partitioned, three virtual parts, gradient-free monitors" % TRI, free=True)
