"""The lane mapping of the plot-field kernel (hfx_eles_sample_plot, hfx_eles_calc_plot_fields), independent of any fixture: a
seeded random opp_p, state, gradient, averages and sensor on blocks that no residual ever runs on, against the numpy restatement
(tests/plot_rows_util.py).  hfx_eles_plot_launch says which path a case took: several elements per pass with a partial last pass,
one element per pass, an element's plot points in several passes of the lanes, workgroups that loop.  Bars: those of
plot_rows_util, 1e-11 of the column's un-cancelled scale plus 1e-14 of the value."""
import os

import numpy as np
import pytest

import hfx
import plot_rows_util as PU

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL_3D = ["u", "v", "w", "energy", "mach", "pressure", "vorticity", "q_criterion", "scaled_q_criterion", "sensor"]
ALL_2D = ["u", "v", "w", "energy", "mach", "pressure", "vorticity", "sensor"]
THREADS = 256  # lanes of a workgroup of the kernel


@pytest.fixture()
def ctx():
    c = hfx.Context(0)
    yield c
    c.close()


def random_block(ctx, n_dims, n_eles, n_upts, rng):
    """a block of random operators and metrics: nothing here runs a residual"""
    params = hfx.params_from(dict(np.load(os.path.join(GOLDEN, "hex_p2_integrals.npz" if n_dims == 3 else "quad_p3_integrals.npz"))))
    ctx.set_params(params)
    nfp, nf = 6, n_dims + 2
    r = lambda *s: rng.uniform(-1.0, 1.0, s)
    data = dict(opp_0=r(nfp, n_upts), opp_3=r(n_upts, nfp), opp_6=r(nfp, n_upts), detjac_upts=r(n_upts, n_eles) + 2.0,
                JGinv_upts=r(n_dims, n_dims, n_upts, n_eles), detjac_fpts=r(nfp, n_eles) + 2.0, JGinv_fpts=r(n_dims, n_dims, nfp, n_eles),
                tdA_fpts=r(nfp, n_eles), norm_fpts=r(nfp, n_eles, n_dims))
    for i in range(n_dims):
        data.update({"opp_1_%d" % i: r(nfp, n_upts), "opp_2_%d" % i: r(n_upts, n_upts), "opp_4_%d" % i: r(n_upts, n_upts),
                     "opp_5_%d" % i: r(n_upts, nfp)})
    e = hfx.Eles(ctx, [n_eles, n_upts, nfp, nf, n_dims], data, ele_type=4 if n_dims == 3 else 1, order=2 if n_dims == 3 else 3)
    # a physical state: density and energy well above the kinetic energy
    u = np.zeros((n_upts, n_eles, nf), order="F")
    u[..., 0] = rng.uniform(0.8, 1.2, (n_upts, n_eles))
    for m in range(n_dims):
        u[..., 1 + m] = rng.uniform(-0.3, 0.3, (n_upts, n_eles))
    u[..., nf - 1] = rng.uniform(2.4, 2.6, (n_upts, n_eles))
    grad = np.asfortranarray(rng.uniform(-1.0, 1.0, (n_upts, n_eles, nf, n_dims)))
    e.upload(hfx.DISU_UPTS0, u)
    e.upload(hfx.GRAD_DISU_UPTS, grad)
    return e, u, grad, params.gamma


def interpolation(n_ppts, n_upts, rng):
    """rows that sum to one with positive weights, as an interpolation has: the interpolated state stays physical"""
    opp = rng.uniform(0.0, 1.0, (n_ppts, n_upts))
    return np.asfortranarray(opp / opp.sum(axis=1)[:, None])


CASES = [(3, ne, npp) for ne in (1, 5, 33) for npp in (4, 64, 65, 125, 729)] + [(2, 33, 4), (2, 5, 65)]


@pytest.mark.parametrize("n_dims,n_eles,n_ppts", CASES)
def test_lane_mapping(ctx, n_dims, n_eles, n_ppts):
    """every field, two average fields and the sensor; the grid held to 2 workgroups so that 33 elements make a workgroup loop"""
    rng = np.random.default_rng(20261020 + 1000 * n_eles + n_ppts)
    n_upts = 27 if n_dims == 3 else 16
    ctx.set_option("persistent_grid_cap", 2)
    e, u, grad, gamma = random_block(ctx, n_dims, n_eles, n_upts, rng)
    opp = interpolation(n_ppts, n_upts, rng)
    e.set_opp_p(opp)
    # (with 65 plot points more average fields than the block has fields: two slabs of them)
    e.set_average_fields(["rho_average", "e_average"] + (["u_average", "v_average", "e_average", "rho_average"] if n_ppts == 65 else []))
    n_avg = e.n_average_fields
    avg = np.asfortranarray(rng.uniform(-1.0, 1.0, (n_upts, n_eles, n_avg)))
    e.upload_average(avg)
    sensor = np.asfortranarray(rng.uniform(0.0, 1.0, n_eles))
    e.upload(hfx.SENSOR, sensor)
    names = ALL_3D if n_dims == 3 else ALL_2D
    # (the sensor needs shock capturing on the block: asked for below, where it is refused first)
    with pytest.raises(hfx.HfxError, match="Sensor unavailable"):
        ctx.set_plot_monitor(names, plot_freq=1, capacity=2)
        e.calc_plot_fields()
    modes = max(1, n_upts // 3)
    e.set_shock_capture(np.eye(n_upts), np.eye(n_upts), rng.uniform(0.5, 1.0, n_upts), np.arange(n_upts) >= n_upts - modes, 1e9, 0)
    e.upload(hfx.SENSOR, sensor)
    ctx.set_plot_monitor(names, plot_freq=1, capacity=2)

    groups, epp, ppp = e.plot_launch()
    assert groups <= 2 and ppp == min(n_ppts, THREADS)
    if n_ppts > THREADS:
        assert epp == 1 and n_ppts > 2 * ppp  # several passes of the lanes, the last one partial
    else:
        assert epp == min(THREADS // n_ppts, 32768 // (8 * n_upts * (n_dims + 2)))
    if (n_eles, n_ppts) == (33, 64):
        assert epp == 4 and n_eles % epp != 0 and -(-n_eles // epp) > 2 * groups  # a partial last pass; every workgroup loops
    if (n_eles, n_ppts) == (5, 4):
        assert epp > n_eles  # one pass, not full

    got = e.calc_plot_fields()
    want, scales = PU.fields(names, opp, u, grad, gamma, average=avg, sensor=sensor)
    assert got.shape == want.shape == (n_ppts, n_eles, n_dims + 2 + n_avg + len(names))
    m = PU.miss(got, want, scales)
    print("%d-D, %d elements, %d plot points (%d per pass of %d elements): largest miss %.3f bars" % (n_dims, n_eles, n_ppts, ppp, epp, m.max()))
    assert np.all(m <= 1.0), m
    # the interpolated state is that of hfx_eles_calc_disu_ppts to rounding, the sensor the element's, bit for bit
    old = e.calc_disu_ppts()
    assert np.abs(got[..., :n_dims + 2] - old).max() <= 1e-14 * np.abs(old).max()
    assert np.array_equal(got[..., -1], np.broadcast_to(sensor[None, :], (n_ppts, n_eles)))
    # two samples of one state and the on-demand snapshot: equal bit for bit
    e.sample_plot(0.25, 1)
    e.sample_plot(0.5, 2)
    assert e.plot_count() == 2
    times, steps, values = e.read_plot_snapshots()
    assert list(times) == [0.25, 0.5] and list(steps) == [1, 2] and e.plot_count() == 0
    assert values.shape == got.shape + (2,)
    assert np.array_equal(values[..., 0], got) and np.array_equal(values[..., 1], got)
    e.close()


def test_each_selected_field_moves_its_column(ctx):
    """the fields in the caller's order, one listed twice; n_diag = 0 is the conserved fields alone"""
    rng = np.random.default_rng(7)
    e, u, grad, gamma = random_block(ctx, 3, 5, 27, rng)
    opp = interpolation(27, 27, rng)
    e.set_opp_p(opp)
    order = ["pressure", "q_criterion", "u", "pressure", "vorticity"]
    ctx.set_plot_monitor(order, plot_freq=1, capacity=1)
    got = e.calc_plot_fields()
    want, scales = PU.fields(order, opp, u, grad, gamma)
    assert np.all(PU.miss(got, want, scales) <= 1.0)
    assert np.array_equal(got[..., 5], got[..., 8]) and not np.array_equal(got[..., 5], got[..., 7])
    ctx.set_plot_monitor([], plot_freq=1, capacity=1)
    bare = e.calc_plot_fields()
    assert bare.shape == (27, 5, 5) and np.array_equal(bare, got[..., :5])
    e.close()


def test_a_nan_is_stored(ctx):
    rng = np.random.default_rng(8)
    e, u, grad, gamma = random_block(ctx, 3, 5, 27, rng)
    u[:, 3, 4] = -50.0  # a negative pressure in element 3: its Mach number is the square root of a negative number
    e.upload(hfx.DISU_UPTS0, u)
    e.set_opp_p(interpolation(8, 27, rng))
    ctx.set_plot_monitor(["mach"], plot_freq=1, capacity=1)
    got = e.calc_plot_fields()
    assert np.all(np.isnan(got[:, 3, 5])) and not np.any(np.isnan(np.delete(got, 3, axis=1)))
    e.close()


def test_refusals(ctx):
    rng = np.random.default_rng(9)
    e, u, grad, gamma = random_block(ctx, 2, 5, 16, rng)
    with pytest.raises(hfx.HfxError, match="no monitor"):
        e.sample_plot(0.0, 0)
    with pytest.raises(hfx.HfxError, match="plot_quantity not recognized"):
        ctx.set_plot_monitor([0, 10], plot_freq=1, capacity=1)
    with pytest.raises(hfx.HfxError, match="plot_freq"):
        ctx.set_plot_monitor(["u"], plot_freq=0, capacity=1)
    with pytest.raises(hfx.HfxError, match="at least 1"):
        ctx.set_plot_monitor(["u"], plot_freq=1, capacity=-1)
    ctx.set_plot_monitor(["u"], plot_freq=1, capacity=1)
    with pytest.raises(hfx.HfxError, match="hfx_eles_set_opp_p"):
        e.sample_plot(0.0, 0)
    e.set_opp_p(interpolation(4, 16, rng))
    ctx.set_plot_monitor(["u", "q_criterion"], plot_freq=1, capacity=1)
    with pytest.raises(hfx.HfxError, match="Q criterion Not implemented in 2D"):
        e.sample_plot(0.0, 0)
    ctx.set_plot_monitor(["sensor"], plot_freq=1, capacity=1)
    with pytest.raises(hfx.HfxError, match="Sensor unavailable"):
        e.sample_plot(0.0, 0)
    assert e.plot_count() == 0
    ctx.set_plot_monitor(["vorticity"], plot_freq=1, capacity=1)
    e.sample_plot(0.0, 0)
    with pytest.raises(hfx.HfxError, match="history is full"):
        e.sample_plot(0.0, 1)
    first = e.read_plot_snapshots()[2]
    # registering again empties the histories; capacity 0 drops the monitor
    e.sample_plot(0.0, 0)
    ctx.set_plot_monitor(["vorticity"], plot_freq=1, capacity=2)
    assert e.plot_count() == 0
    e.sample_plot(0.0, 0)
    assert np.array_equal(e.read_plot_snapshots()[2], first)
    e.sample_plot(0.0, 0)
    ctx.set_plot_monitor([], capacity=0)
    assert e.plot_count() == 0
    with pytest.raises(hfx.HfxError, match="no monitor"):
        e.sample_plot(0.0, 0)
    # an inviscid context has no grad_disu_upts: the reference's words
    p = ctx.params
    p.viscous = 0
    ctx.set_params(p)
    with pytest.raises(hfx.HfxError, match="only supported by viscous simualtion"):
        ctx.set_plot_monitor(["pressure", "vorticity"], plot_freq=1, capacity=1)
    ctx.set_plot_monitor(["pressure"], plot_freq=1, capacity=1)
    e.sample_plot(0.0, 0)
    assert e.plot_count() == 1
    assert hfx.plot_monitor_samples(0, 5, 2) == 2 and hfx.plot_monitor_samples(1, 1, 2) == 1 and hfx.plot_monitor_samples(2, 1, 2) == 0
    e.close()
