"""The full-loop fixtures (tests/golden/full_loop/fl_*.npz; tools/capture_full_loop.py) on the CPU: conditions 2 and 3 of the capture
are proved again from the committed files, so that a stale or hand-edited fixture fails here, and the sampling schedule the fixtures
pin is the one hfx_integral_monitor_samples and hfx_plot_monitor_samples count, for the whole span and for every cut of it into two
and three calls.  No GPU.  Bars: tests/history_rows_util.py and tests/plot_rows_util.py; see tests/full_loop_util.py."""
import numpy as np
import pytest

import full_loop_util as FU
import hfx
import history_rows_util as HU
import integral_history_util as IU
import plot_rows_util as PU

# history rows and plot files per case, as the issue of this family states them
ROWS = {"fl_hex_p2_channel": ([1, 3, 6], [2, 4, 6]), "fl_hex_p2_forced": ([1], [2]), "fl_quad_p3_walls": ([1, 2, 4], [3]),
        "fl_tet_p2_euler": ([1, 4], [3, 6]), "fl_tri_p3_walls": ([1, 2, 4], [3]), "fl_tri_p3_shock": ([1, 2, 4], [3])}
BY_CALLS = {"fl_hex_p2_channel": [1, 2, 3, 4, 6], "fl_hex_p2_forced": [1, 2], "fl_quad_p3_walls": [1, 2, 3, 4], "fl_tet_p2_euler": [1, 3, 4, 6],
            "fl_tri_p3_walls": [1, 2, 3, 4], "fl_tri_p3_shock": [1, 2, 3, 4]}
TRI = ["fl_tri_p3_walls", "fl_tri_p3_shock"]


@pytest.mark.parametrize("name", FU.FL)
def test_every_row_the_driver_wrote_is_met(name):
    """condition 2: the oracle in lockstep -- the state after the step with the corrected gradient of the last stage's input --
    meets every column of every history row and every plot file; the bars the capture recorded are the ones found now"""
    d, w = FU.reference(name)
    sz = [int(v) for v in d["sizes"]]
    diag, avg = PU.names_of(d, "diagnostic_fields"), PU.names_of(d, "average_fields")
    assert [r["step"] for r in w["hist"]] == [int(v) for v in d["hist_iter"]] == ROWS[name][0]
    assert [s["step"] for s in w["plot"]] == [int(v) for v in d["plot_iter"]] == ROWS[name][1]
    assert d["plot_rows"].shape == (len(w["plot"]), sz[0] * d["opp_p"].shape[0], sz[4] + sz[3] + len(avg) + len(diag))
    for k, r in enumerate(w["hist"]):
        bars = {key: r[key] for key in ("res_bars", "force_bars", "diag_bars") if key in r}
        print("%s history row at step %d: %s (forces in units of the row's own size: %s)" % (name, r["step"], bars, r.get("force_row_size")))
        assert max(bars.values()) <= 1.0, (name, r["step"], bars)
        assert ("force_bars" in r) == bool(int(d["calc_force"][0])) and ("diag_bars" in r) == bool(d["hist_diag"].shape[1])
        assert abs(r["step"] * w["dt"] * float(d["time_ref"][0]) - d["hist_time"][k]) <= 1e-13 * d["hist_time"][k]
    for s in w["plot"]:
        print("%s plot file %d: %s bars" % (name, s["step"], np.array2string(s["bars"], precision=2)))
        assert np.all(s["bars"] <= PU.bars(d)), (name, s["step"], s["bars"])
    assert FU.worst_bars(w) <= 1.0
    assert np.all(np.array([s["bars"] for s in w["plot"]]).max(axis=0) <= d["rows_paired_bars"] + 1e-9)
    # the harness's own last state: the two runs of the capture are one (on the forced case: the run without the force; on the
    # triangle case with shock capturing: the run without the filter)
    free = FU.harness_state(d, w)
    assert np.abs(free - d["u_last_harness"]).max() <= 1e-11 * np.abs(d["u_last_harness"]).max()


@pytest.mark.parametrize("name", FU.FL)
def test_the_fixture_tells_right_from_subtly_wrong(name):
    """condition 3: every sensitivity number exceeds 1e-6 in every row or file it is formed for, and is the one the capture stored"""
    d, w = FU.reference(name)
    formed = {"own_gradient_force": bool(int(d["calc_force"][0])) * len(d["hist_iter"]), "own_gradient_vorticity": len(d["plot_iter"]),
              "previous_state_row": len(d["plot_iter"]), "unforced_state": int(FU.forced(d)),
              "spinup_zero_average": len(d["plot_iter"]) if PU.names_of(d, "average_fields") else 0}
    for key in FU.SENSITIVITY:
        got, stored = np.array(w["sens"][key]), d["sens_" + key]
        print("%s %s: %s" % (name, key, np.array2string(got, precision=2)))
        assert len(got) == len(stored) == formed[key], key
        assert np.all(got > FU.MARGIN), key
        assert np.all(np.abs(got - stored) <= 1e-6 * got), key


@pytest.mark.parametrize("name", FU.FL)
def test_a_changed_digit_is_noticed(name):
    """a stored row changed in its 9th significant digit misses its bar: one value of every kind of row, the largest of its column
    (history) or of its file's column (plot), multiplied by 1 + 1e-9"""
    d, w = FU.reference(name)
    n_dims, n_fields = int(d["sizes"][4]), int(d["sizes"][3])
    bump = 1.0 + 1e-9
    r = w["hist"][-1]
    # residual columns are log10: the 9th digit of the printed value
    res = d["hist_res"][-1].copy()
    res[0] *= bump
    assert HU.log_miss(r["res"], res) > 1.0
    if "force" in r:
        # (the bar is 1e-11 of the UN-CANCELLED scale: a column that cancels below 1e-2 of it keeps fewer than 9 digits at that bar)
        frc = d["hist_force"][-1].copy()
        i = int(np.argmax(np.abs(frc) / r["force_scale"]))
        if abs(frc[i]) >= 1e-2 * r["force_scale"][i]:
            frc[i] *= bump
            assert HU.value_miss(r["force"], frc, r["force_scale"]) > 1.0
    if "diag" in r:
        dg = d["hist_diag"][-1].copy()
        i = int(np.argmax(np.abs(dg)))
        dg[i] *= bump
        assert HU.value_miss(r["diag"], dg, np.abs(d["hist_diag"][-1]).max()) > 1.0
    s = w["plot"][-1]
    for col in range(len(s["scales"])):
        rows = d["plot_rows"][-1][:, n_dims:].copy()
        i = int(np.argmax(np.abs(rows[:, col])))
        if abs(rows[i, col]) < 1e-2 * s["scales"][col]:
            continue  # (a column whose values all lie far below its un-cancelled scale: the bar is of the scale, not of the digits)
        rows[i, col] *= bump
        assert PU.miss(s["rows"], rows, s["scales"])[col] > 1.0, col


def test_the_controller_is_the_drivers():
    """fl_hex_p2_forced: the lockstep controller meets the lines the driver printed before every step (8 digits) at 1e-7, with the
    reference's hard-coded target and a force in every step; fl_hex_p2_channel is the same channel without the force"""
    d, w = FU.reference("fl_hex_p2_forced")
    drv = d["driver_controller"]
    assert drv.shape == (FU.meta_of(d)["steps"], 5) and np.all(drv[:, 1] == HU.FORCING_MDOT0) and np.all(drv[:, 4] != 0)
    tie = FU.controller_tie(d, w)
    print("controller tie %.2e" % tie)
    assert tie <= 1e-7
    assert not FU.forced(FU.reference("fl_hex_p2_channel")[0])


@pytest.mark.parametrize("name", FU.FL)
def test_sampling_schedule(name):
    """the rows the fixtures hold are the steps the library's own rules count, from clock 0 over the whole span and over every cut
    of the span into two and three calls; the steps whose last stage runs call by call are the union of the monitors' samples that
    read the gradient"""
    d, _ = FU.reference(name)
    n = FU.meta_of(d)["steps"]
    freq, pf = int(d["monitor_res_freq"][0]), int(d["plot_freq"][0])
    hist, plot = ROWS[name]
    assert freq != pf
    assert IU.sample_steps(0, n, freq) == hist and PU.sample_steps(0, n, pf) == plot
    assert hfx.integral_monitor_samples(0, n, freq) == len(hist) and hfx.plot_monitor_samples(0, n, pf) == len(plot)
    sched = FU.schedule(d)
    assert [s + 1 for s, (h, p, c) in enumerate(sched) if h] == hist and [s + 1 for s, (h, p, c) in enumerate(sched) if p] == plot
    assert [s + 1 for s, (h, p, c) in enumerate(sched) if c] == BY_CALLS[name]
    for parts in (2, 3):
        if parts > n:
            continue
        for cut in FU.cuts(n, parts):
            assert sum(cut) == n and min(cut) >= 1
            at, nh, npl = 0, 0, 0
            for k in cut:
                a, b = hfx.integral_monitor_samples(at, k, freq), hfx.plot_monitor_samples(at, k, pf)
                assert a == len([s for s in hist if at < s <= at + k]), (cut, at)
                assert b == len([s for s in plot if at < s <= at + k]), (cut, at)
                nh, npl, at = nh + a, npl + b, at + k
            assert (nh, npl) == (len(hist), len(plot)), cut
    assert len(FU.cuts(7, 3)) == 15 and [2, 1, 4] in FU.cuts(7, 3)


@pytest.mark.parametrize("name", FU.FL)
def test_probes_are_located_and_expected(name):
    """the 8 probes lie in the elements their positions were formed in, the operator rows reproduce a linear field exactly enough
    (their sum is 1), and the expected samples fall on the steps the probe frequency gives"""
    d, _ = FU.reference(name)
    P = FU.probes(name)
    assert P["opp"].shape == (int(d["sizes"][1]), FU.N_PROBES) and sorted(P["perm"]) == list(range(FU.N_PROBES))
    assert np.all(np.abs(P["opp"].sum(axis=0) - 1.0) <= 1e-12)
    steps, values = FU.expected_probes(name)
    n = FU.meta_of(d)["steps"]
    assert steps == [s for s in range(1, n + 1) if s % FU.PROBE_FREQ[name] == 0] and len(steps) >= 1
    assert values.shape == (len(P["names"]), FU.N_PROBES, len(steps)) and np.all(np.isfinite(values))
    if name == "fl_hex_p2_channel":
        assert steps == [5]  # (behind a fused step between two steps that end call by call)


# ---- triangles: what the host mirror does not build comes from the fixture ---------------------------------------------------------
@pytest.mark.parametrize("name", TRI)
def test_triangle_wall_faces_and_surface_cubature(name):
    """the wall list derived from the boundary tables and the surface cubature the harness dumped: 4 faces on either wall of the
    4 x 5 box, the isothermal ones on y-, every local face among them (the node lists are rotated), 4 points per face; weights that
    sum to the reference side's length 2, unit normals that point down on y- and up on y+, face Jacobians that sum to the wall's
    length within the deformation; an element without a face in any boundary group carries zeros"""
    import wall_force_util as W
    d, _ = FU.reference(name)
    n_eles, n_upts, order = int(d["sizes"][0]), int(d["sizes"][1]), int(d["sizes"][5])
    assert int(d["sizes"][6]) == FU.TRIANGLES and n_eles == 40
    F = FU.force_setup(d)
    A = F["A"]
    assert len(A["face_ele"]) == 8 and sorted(A["face_flag"].tolist()) == [W.ISOTHERM_WALL] * 4 + [W.ADIABAT_WALL] * 4
    assert np.all(np.diff(A["face_ele"]) > 0) and set(A["face_inter"].tolist()) == {0, 1, 2}
    assert len(A["opp"]) == 3 and F["phys"]["viscous"] == 1 and F["ref"]["area_ref"] > 0
    length = {W.ISOTHERM_WALL: 0.0, W.ADIABAT_WALL: 0.0}
    for f, (e, l, flag) in enumerate(zip(A["face_ele"], A["face_inter"], A["face_flag"])):
        assert A["opp"][l].shape == (order + 1, n_upts) and np.all(np.abs(A["opp"][l].sum(axis=1) - 1.0) <= 1e-12)
        nm = A["norm"][f]
        assert nm.shape == (order + 1, 2) and np.all(np.abs((nm * nm).sum(axis=1) - 1.0) <= 1e-13)
        assert np.all(nm[:, 1] < -0.9) if flag == W.ISOTHERM_WALL else np.all(nm[:, 1] > 0.9)
        assert np.all(A["detjac"][f] > 0)
        length[int(flag)] += float((A["weight"][l] * A["detjac"][f]).sum())
    for v in length.values():  # (a wall is the deformed image of a side of 2 pi)
        assert 2.0 * np.pi - 1e-12 <= v <= 1.1 * 2.0 * np.pi
    walls = set(A["face_ele"].tolist())
    for l in range(3):
        dj = np.asarray(d["inter_detjac_inters_cubpts_%d" % l])
        assert dj.shape == (order + 1, n_eles) and np.asarray(d["norm_inters_cubpts_%d" % l]).shape == (order + 1, n_eles, 2)
        # the reference forms them for every element with a face in ANY group, the cyclic ones included (bdy_ele2ele): 4 + 4 on the
        # walls, 5 + 5 on the x sides, two corner triangles counted twice
        has = dj.all(axis=0)
        assert np.array_equal(has, dj.any(axis=0)) and has.sum() == 16 and has[sorted(walls)].all()


@pytest.mark.parametrize("name", TRI)
def test_triangle_probes_sit_at_interior_plot_points_and_meet_the_plot_file(name):
    """the 8 probes are plot points strictly inside their elements, spread over the usual element choices; at the step both a probe
    sample and a plot file fall on, the lockstep's probe samples give the DRIVER's conserved plot rows at those points at the plot
    bar -- and the samples of the neighbouring steps do not (the check can tell the step)"""
    d, w = FU.reference(name)
    P = FU.probes(name)
    n = int(d["sizes"][0])
    assert P["ele"].tolist() == [0, 1, n // 3, n // 2, n // 2, (2 * n) // 3, n - 2, n - 1] and P["perm"].tolist() == FU.PROBE_PERM
    loc = np.asarray(d["loc_ppts"])[:, P["ppt"]]
    assert np.all(loc > -1 + 1e-3) and np.all(loc.sum(axis=0) < -1e-3)
    steps, values = FU.expected_probes(name)
    worst = FU.probes_against_plot_rows(name, steps, values)
    print("%s: probes against the driver's plot rows %.3g bars" % (name, worst))
    assert worst is not None and worst <= 1.0
    assert FU.probes_against_plot_rows(name, steps, np.roll(values, 1, axis=2)) > 1e3


def test_triangle_virtual_parts_offer_both_kinds_of_group():
    """FU.TRI_PARTS on fl_tri_p3_walls: three virtual parts, six directed segments, every flux point in exactly one face table, and of
    the two groups of the fused 2-D simplex stage (32 + 8 elements at P3) one has partition faces and one has none"""
    from test_tris_partition_oracle import grow_parts, group_census, virtual_tables
    d, _ = FU.reference("fl_tri_p3_walls")
    reg, L, Rlut, seg = virtual_tables(d, grow_parts(d, *FU.TRI_PARTS))
    ne, nfp = int(d["sizes"][0]), int(d["sizes"][2])
    assert len(seg) == 6 and L.shape[1] > 0 and np.array_equal(reg["bdy0_L"], d["bdy0_L"])
    seen = [np.ravel(L)] + [np.ravel(reg[k]) for k in reg if k.startswith(("int", "bdy")) and k.endswith(("_L", "_R"))]
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(nfp * ne))
    assert group_census(reg, L) == (1, 1, True, False)


def test_triangle_shock_filter_counts():
    """fl_tri_p3_shock: in every step the filter takes at least one element and not all, no sensor value of any stage lies within
    tri_shock_util.MARGIN of s0, and the counts are the ones the capture stored; without the filter the run ends elsewhere"""
    import tri_shock_util as TS
    d, w = FU.reference("fl_tri_p3_shock")
    n = int(d["sizes"][0])
    per_stage, per_step, gap = FU.filtered_counts(d)
    print("filtered per stage %s, per step %s of %d, closest %.1e" % (per_stage.tolist(), per_step.tolist(), n, gap))
    assert np.all((per_step >= 1) & (per_step <= n - 1)) and gap > TS.MARGIN
    assert np.array_equal(per_stage, d["filtered_per_stage"]) and np.array_equal(per_step, d["filtered_per_step"])
    assert "sensor" in PU.names_of(d, "diagnostic_fields") and FU.shock(d) and not FU.shock(FU.reference("fl_tri_p3_walls")[0])
    moved = np.abs(w["unfiltered"] - w["states"][-1]).max() / np.abs(w["states"][-1]).max()
    print("the filter moves the final state by %.2e" % moved)
    assert moved > FU.MARGIN
