"""The plot-row fixtures (tests/golden/plot_rows/pr_*.npz; tools/capture_plot_rows.py) on the CPU: the numpy restatement of a row
(tests/plot_rows_util.py) through the oracle reproduces every row the genuine driver wrote, and the pairing the rows pin is visible
-- the diagnostic fields are formed from the state after the step and the gradient the step's last RK stage left.  No GPU."""
import json

import numpy as np
import pytest

import plot_rows_util as PU

_RUNS = {}


def snapshots(name):
    """the oracle stepped once per fixture: per plot file the restated columns, their scales, and (pairing case) the vorticity
    column formed with the sampled state's own gradient"""
    if name not in _RUNS:
        d = PU.load(name)
        steps = json.loads(bytes(d["meta_json"]).decode())["steps"]
        diag, avg = PU.names_of(d, "diagnostic_fields"), PU.names_of(d, "average_fields")
        run = PU.Run(d, avg)
        out = []
        for s in range(1, steps + 1):
            run.step()
            if s in list(d["plot_iter"]):
                got, scales = PU.fixture_fields(d, run)
                own = PU.fixture_fields(d, run, grad=run.own_gradient())[0] if "vorticity_own_gradient" in d else None
                out.append((PU.rows_of(got), scales, None if own is None else PU.rows_of(own)))
        _RUNS[name] = (d, diag, avg, out)
    return _RUNS[name]


@pytest.mark.parametrize("name", PU.PR)
def test_restatement_reproduces_the_driver(name):
    d, diag, avg, snaps = snapshots(name)
    sz = [int(v) for v in d["sizes"]]
    n_dims, n_fields = sz[4], sz[3]
    assert list(d["plot_iter"]) == PU.sample_steps(0, json.loads(bytes(d["meta_json"]).decode())["steps"], int(d["plot_freq"][0]))
    assert d["plot_rows"].shape == (len(snaps), sz[0] * d["opp_p"].shape[0], n_dims + n_fields + len(avg) + len(diag))
    for k, (got, scales, _) in enumerate(snaps):
        m = PU.miss(got, d["plot_rows"][k][:, n_dims:], scales)
        print("%s file %d: %s bars" % (name, int(d["plot_iter"][k]), np.array2string(m, precision=2)))
        assert np.all(m <= 1.0), (k, m)


def test_a_refreshed_gradient_is_not_what_the_reference_plots():
    """condition 3 of the capture: the vorticity of the sampled state's OWN gradient misses the driver's column by more than 1e-6 of
    its largest value in every file, the last stage's gradient meets it; the numbers are those the capture recorded"""
    d, diag, avg, snaps = snapshots("pr_hex_p2_rk45")
    n_dims, n_fields = int(d["sizes"][4]), int(d["sizes"][3])
    col = n_fields + len(avg) + diag.index("vorticity")
    for k, (got, scales, own) in enumerate(snaps):
        drv = d["plot_rows"][k][:, n_dims + col]
        big = np.abs(drv).max()
        own_miss, paired_miss = np.abs(own[:, col] - drv).max() / big, np.abs(got[:, col] - drv).max() / big
        print("file %d: own gradient %.2e, last stage's %.2e of the column's largest value" % (int(d["plot_iter"][k]), own_miss, paired_miss))
        assert own_miss > 1e-6 and paired_miss < 1e-11
        assert abs(own_miss - d["vorticity_own_gradient"][k]) <= 1e-6 * own_miss


def test_each_selected_field_moves_its_column():
    """the columns follow the caller's order: every name gives a column of its own, a name listed twice the same column twice"""
    d, diag, avg, snaps = snapshots("pr_hex_p2_rk45")
    run = PU.Run(d)
    run.step()
    names = [n for n in PU.NAMES if n != "sensor"] + ["sensor"]
    every, _ = PU.fields(names, d["opp_p"], run.u, run.grad, PU.scalar(d, "gamma"), sensor=run.sensor)
    nf = run.u.shape[2]
    for i in range(len(names)):
        for j in range(i):
            assert not np.array_equal(every[..., nf + i], every[..., nf + j]), (names[i], names[j])
    for i, n in enumerate(names):
        one, _ = PU.fields([n, "pressure", n], d["opp_p"], run.u, run.grad, PU.scalar(d, "gamma"), sensor=run.sensor)
        assert np.array_equal(one[..., nf], every[..., nf + i]) and np.array_equal(one[..., nf + 2], every[..., nf + i])
        assert np.array_equal(one[..., nf + 1], every[..., nf + names.index("pressure")])


def test_refusals_of_the_restatement():
    """the reference's messages (src/eles.cpp:3933, :3988, :3994)"""
    d, diag, avg, snaps = snapshots("pr_quad_p3_walls")
    run = PU.Run(d)
    run.step()
    g = PU.scalar(d, "gamma")
    with pytest.raises(ValueError, match="Q criterion Not implemented in 2D"):
        PU.fields(["q_criterion"], d["opp_p"], run.u, run.grad, g)
    with pytest.raises(ValueError, match="Sensor unavailable"):
        PU.fields(["sensor"], d["opp_p"], run.u, run.grad, g)
    with pytest.raises(ValueError, match="plot_quantity not recognized"):
        PU.fields(["enstrophy"], d["opp_p"], run.u, run.grad, g)
    two, _ = PU.fields(["w", "vorticity"], d["opp_p"], run.u, run.grad, g)
    assert np.all(two[..., 4] == 0.0) and np.all(two[..., 5] >= 0.0)


@pytest.mark.parametrize("n_dims", [2, 3])
def test_the_kernels_point_formulas_on_the_host(n_dims):
    """csrc/plot_point.hpp, which the kernel evaluates at every plot point, through hfx_plot_point_fields on the host (no device): a
    seeded random state and gradient at 200 points against the numpy restatement, whose interpolation is the identity here.  Bars as
    everywhere; the two share nothing but the reference"""
    import hfx
    rng = np.random.default_rng(20261020 + n_dims)
    nf, n = n_dims + 2, 200
    names = [m for m in PU.NAMES if n_dims == 3 or "q_criterion" not in m]
    u = np.zeros((1, n, nf))
    u[0, :, 0] = rng.uniform(0.8, 1.2, n)
    u[0, :, 1:nf - 1] = rng.uniform(-0.3, 0.3, (n, n_dims))
    u[0, :, nf - 1] = rng.uniform(2.4, 2.6, n)
    grad = rng.uniform(-1.0, 1.0, (1, n, nf, n_dims))
    sensor = rng.uniform(0.0, 1.0, n)
    want, scales = PU.fields(names, np.eye(1), u, grad, 1.4, sensor=sensor)
    got = np.array([hfx.plot_point_fields(names, u[0, i], grad[0, i], 1.4, sensor[i]) for i in range(n)])
    m = PU.miss(got, want[0][:, nf:], scales[nf:])
    print("%d-D: %s bars" % (n_dims, np.array2string(m, precision=3)))
    assert np.all(m <= 1.0), m
    if n_dims == 2:
        assert np.all(got[:, names.index("w")] == 0.0)
        with pytest.raises(hfx.HfxError, match="Q criterion Not implemented in 2D"):
            hfx.plot_point_fields(["q_criterion"], u[0, 0], grad[0, 0], 1.4)
    with pytest.raises(hfx.HfxError, match="plot_quantity not recognized"):
        hfx.plot_point_fields([10], u[0, 0], grad[0, 0], 1.4)
    # gradient-free fields never touch the gradient
    assert np.array_equal(hfx.plot_point_fields(names[:6], u[0, 0], None, 1.4), got[0, :6])
