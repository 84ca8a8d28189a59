"""The rows of history.plt against the GENUINE driver, without a GPU: the fixtures of tools/capture_history_rows.py hold every
column of every row the reference's main loop wrote (tests/golden/history_rows/hr_*.npz).  The oracle (tests/oracle_py.py) steps the
fixture's case; the numpy restatement of eles::compute_res_upts and output::CalcNormResidual (tests/history_rows_util.py) gives
the residual columns, tests/wall_force_util.py the force columns, tests/integral_history_util.py the diagnostics.

Bars: 1e-11 relative on a norm (log10(1 + 1e-11) on the printed log10) plus 1e-14 x max(1, |value|) for the 15 printed digits; the
forces and diagnostics 1e-11 of their un-cancelled scale (of the row's largest diagnostic) plus the same digits.

The host mirror's own arithmetic (csrc/host: res_norm_type, hfxh_norm_residual, the sampling rule) is checked on a CPU case.
"""
import functools

import numpy as np
import pytest

import hfx
import hfx_host as H
import history_rows_util as HU
import integral_history_util as IU
import wall_force_util as W
from test_wall_force_host import device_arrays, mirror_case, phys_of, ref_of


@functools.lru_cache(maxsize=None)
def oracle_rows(name):
    """the fixture and, per row of the driver, what the oracle holds behind that step: div_tconf_upts of the last stage, the state,
    the last stage's gradient; on the pairing case the sampled state's own gradient too.  Computed once, left unchanged."""
    d = HU.load(name)
    meta = HU.meta_of(d)
    run = HU.oracle_run(d)
    want = [int(v) for v in d["hist_iter"]]
    rows = []
    for s in range(1, meta["steps"] + 1):
        run.step()
        if s in want:
            a = run.case.arr
            src = run.src.copy(order="F") if hasattr(run, "src") else None  # (the driven channel: what the controller has added so far)
            rows.append(dict(div=a["div_tconf_upts"].copy(order="F"), u=run.u.copy(order="F"), grad=run.grad.copy(order="F"), src=src,
                             own=run.own_gradient() if "viscous_force_own_gradient" in d else None))
    forces = None
    if int(d["calc_force"][0]):
        mc, _ = mirror_case(d)
        forces = dict(A=device_arrays(mc), phys=phys_of(mc), ref=ref_of(mc))
        mc.close()
    return d, rows, run.case.arr["detjac_upts"], forces


def columns(d, row, detjac, norm_type=None, root_inside=False):
    nt = int(d["res_norm_type"][0]) if norm_type is None else norm_type
    return np.log10(HU.norm_residual(nt, HU.res_upts(nt, row["div"], detjac, row["src"]), detjac.size, root_inside))


@pytest.mark.parametrize("name", HU.HR)
def test_residual_columns_vs_the_driver(name):
    d, rows, detjac, _ = oracle_rows(name)
    assert len(rows) == len(d["hist_iter"]) == len(IU.sample_steps(0, HU.meta_of(d)["steps"], int(d["monitor_res_freq"][0])))
    nt = int(d["res_norm_type"][0])
    for k, row in enumerate(rows):
        got = columns(d, row, detjac)
        miss = HU.log_miss(got, d["hist_res"][k])
        print("%s row at step %d: residual columns %.3f bars" % (name, d["hist_iter"][k], miss))
        assert miss <= 1.0, (name, k)
        # the mirror's finish is the restatement's
        mine = np.log10(H.norm_residual(nt, HU.res_upts(nt, row["div"], detjac, row["src"]), detjac.size))
        assert HU.log_miss(mine, d["hist_res"][k]) <= 1.0


@pytest.mark.parametrize("name", ["hr_quad_p3_walls", "hr_hex_p2_walls", "hr_hex_p2_forced"])
def test_force_and_diagnostic_columns_vs_the_driver(name):
    d, rows, _, F = oracle_rows(name)
    for k, row in enumerate(rows):
        got, S = HU.force_columns(W, F["A"], F["phys"], F["ref"], row["u"], row["grad"])
        miss = HU.value_miss(got, d["hist_force"][k], S)
        print("%s row at step %d: force columns %.3f bars" % (name, d["hist_iter"][k], miss))
        assert miss <= 1.0
        if d["hist_diag"].shape[1]:
            q = IU.fixture_quantities(d, row["u"], row["grad"])
            miss = HU.value_miss(q, d["hist_diag"][k], np.abs(d["hist_diag"][k]).max())
            print("%s row at step %d: diagnostics %.3f bars" % (name, d["hist_iter"][k], miss))
            assert miss <= 1.0


def test_force_pairing_is_visible():
    """with the sampled state's own (refreshed) gradient the viscous force misses the driver's rows by more than the 1e-6 the
    capture tool recorded, in every row"""
    d, rows, _, F = oracle_rows("hr_quad_p3_walls")
    nd = 2
    assert np.all(d["viscous_force_own_gradient"] > 1e-6)
    for k, row in enumerate(rows):
        paired, S = HU.force_columns(W, F["A"], F["phys"], F["ref"], row["u"], row["grad"])
        own, _ = HU.force_columns(W, F["A"], F["phys"], F["ref"], row["u"], row["own"])
        inv, _ = HU.force_columns(W, F["A"], dict(F["phys"], viscous=0), F["ref"], row["u"], None)
        row_vis = d["hist_force"][k] - inv
        rel = np.abs((own - inv)[:nd] - row_vis[:nd]).max() / np.abs(row_vis[:nd]).max()
        print("row at step %d: own-gradient viscous force misses by %.3e (recorded %.3e)" % (d["hist_iter"][k], rel,
                                                                                             d["viscous_force_own_gradient"][k]))
        assert rel > 1e-6
        assert HU.value_miss(own, d["hist_force"][k], S) > 1.0  # and the row's bar is missed


def test_source_term_is_in_the_driven_channels_rows():
    """hr_hex_p2_forced: the driver ran with body_forcing 1; without the - src_upts term every row is missed, and the controller in
    lockstep is the driver's own (its printed mass flux and force, 8 digits)"""
    d, rows, detjac, _ = oracle_rows("hr_hex_p2_forced")
    for k, row in enumerate(rows):
        assert np.abs(row["src"][:, :, 1]).max() > 0 and not row["src"][:, :, [0, 2, 3]].any()
        assert HU.log_miss(columns(d, dict(row, src=None), detjac), d["hist_res"][k]) > 1e6
    run = HU.oracle_run(d)
    for _ in range(HU.meta_of(d)["steps"]):
        run.step()
    drv = d["driver_controller"]
    got = np.array(run.rows)
    assert np.all(np.abs(got - drv[:, 3:]) <= 1e-7 * np.abs(drv[:, 3:]).max(axis=0) + 6e-9)  # (8 printed decimals)
    assert np.all(drv[:, 1] == HU.FORCING_MDOT0) and drv[0, 2] == HU.FORCING_MDOT0


def test_l2_norm_divides_the_root_by_n_upts():
    """sqrt(sum / n_upts) in place of the reference's sqrt(sum) / n_upts misses every row"""
    d, rows, detjac, _ = oracle_rows("hr_hex_p2_rk45")
    assert int(d["res_norm_type"][0]) == 2
    for k, row in enumerate(rows):
        assert HU.log_miss(columns(d, row, detjac, root_inside=True), d["hist_res"][k]) > 1e6
        assert HU.log_miss(columns(d, row, detjac), d["hist_res"][k]) <= 1.0


@pytest.mark.parametrize("name", ["hr_hex_p2_norm0", "hr_hex_p2_norm1", "hr_hex_p2_rk45"])
def test_the_three_norms_differ(name):
    """each fixture's rows are met by its own norm type alone"""
    d, rows, detjac, _ = oracle_rows(name)
    nt = int(d["res_norm_type"][0])
    for other in {0, 1, 2} - {nt}:
        assert HU.log_miss(columns(d, rows[0], detjac, norm_type=other), d["hist_res"][0]) > 1e6


@pytest.mark.parametrize("name", HU.WF)
def test_wall_force_fixtures_residual_columns(name):
    """hist_res of the wall-force fixtures (step 1, one Euler stage, res_norm_type 1): the harness's L1 sums of the first residual
    through the mirror's finish (those files hold neither div_tconf_upts nor the operators: the sums themselves cannot be formed)"""
    d = HU.load(name)
    sz = [int(v) for v in d["sizes"]]
    n_upts = sz[0] * sz[1]
    sums = d["s0_res_sums"][:, 0]
    got = np.log10(H.norm_residual(1, sums, n_upts))
    assert np.array_equal(got, np.log10(HU.norm_residual(1, sums, n_upts)))
    miss = HU.log_miss(got, d["hist_res"])
    print("%s: residual columns %.3f bars" % (name, miss))
    assert miss <= 1.0


# ---- the host mirror's arithmetic on a CPU case --------------------------------------------------------------------------------
def test_mirror_input_and_norms():
    c = H.Case([3, 3, 3], order=2)
    n_fields = 5
    assert c.history() == (2, 0, n_fields + 1)  # res_norm_type 2 (src/input.cpp:108), no monitor, residuals and the time
    with pytest.raises(hfx.HfxError, match="norm_type not recognized"):
        c.set_history(3, 4)
    with pytest.raises(hfx.HfxError, match="at least 0"):
        c.set_history(1, -1)
    assert c.history()[:2] == (2, 0)  # (a refusal leaves the case as it was)
    c.set_history(0, 7)
    assert c.history()[:2] == (0, 7)
    c.set_integral_quantities(["kineticenergy", "enstropy"])
    c.set_monitor_res_freq(3, 7)
    assert c.history()[2] == n_fields + 2 + 1
    c.close()
    sums = np.array([4.0, 9.0, 16.0, 25.0, 36.0])
    assert np.array_equal(H.norm_residual(0, sums, 10), sums)
    assert np.array_equal(H.norm_residual(1, sums, 10), sums / 10)
    assert np.array_equal(H.norm_residual(2, sums, 10), np.sqrt(sums) / 10)
    with pytest.raises(hfx.HfxError, match="norm_type not recognized"):
        H.norm_residual(3, sums, 10)
    for nt in (0, 1, 2):
        bad = sums.copy()
        bad[3] = np.nan
        with pytest.raises(hfx.HfxError, match="NaN residual encountered. Exiting"):
            H.norm_residual(nt, bad, 10)


def test_sampling_steps():
    """the rows of a call: step 1 and the multiples of monitor_res_freq, as the fixtures' iteration columns"""
    for name in HU.HR:
        d = HU.load(name)
        freq, steps = int(d["monitor_res_freq"][0]), HU.meta_of(d)["steps"]
        assert [int(v) for v in d["hist_iter"]] == IU.sample_steps(0, steps, freq)
        assert hfx.integral_monitor_samples(0, steps, freq) == len(d["hist_iter"])
    d = HU.load("hr_quad_p3_walls")  # neither 1 nor a divisor of the step count
    assert int(d["monitor_res_freq"][0]) == 3 and HU.meta_of(d)["steps"] == 4 and list(d["hist_iter"]) == [1, 3]
