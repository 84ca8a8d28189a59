"""Point probes sampled on the device (hfx_ctx_set_probes, hfx_eles_set_probes, hfx_eles_sample_probes, hfx_eles_read_probes),
inside every step loop and through the host mirror (hfxh_case_set_probes).

The yardstick is the genuine reference's plot-point data: every plot point of every element of the four *_plot fixtures is a
probe whose operator row (a row of opp_p) and whose interpolated state (disu_ppts) the reference recorded.  The expected
fields are the numpy statement of src/output.cpp:1479-1538 on that disu_ppts (tests/probe_util.py); tests/test_probes_host.py
shows that they move by less than 1e-13 when the contraction is summed in another order.  Bars: 1e-12 of each field's
largest magnitude over the probes -- the project's 1e-13 for this contraction on the device times ten for the one cancelling
difference in the pressure (E / p is about 2.5 on these fixtures) -- and 1e-13 for rho, which has no derived arithmetic.
"""
import ctypes as C
import os

import numpy as np
import pytest

import hfx
import hfx_host as H
import partition_util as PU
import probe_util as U
from test_gpu_methods_vs_golden import build

pytestmark = pytest.mark.gpu

TIME0 = 0.25  # FlowSol.time before the first step


def close(e, faces, ctx=None):
    for f in faces:
        f.close()
    e.close()
    if ctx is not None:
        ctx.close()


def block(ctx, name):
    """a device block of the fixture's mesh and order: from the fixture itself, from the fixture of the same mesh that holds the
    operators, or (quad_p2_plot, which has no such sibling) from the host mirror's registration"""
    d = U.load(name)
    if "opp_0" in d:
        return build(ctx, d)
    if name in U.BLOCK_OF:
        b = U.load(U.BLOCK_OF[name])
        assert [int(v) for v in d["sizes"][:7]] == [int(v) for v in b["sizes"][:7]]
        return build(ctx, b)
    m, _, _ = U.mirror(name)
    reg = m.registration()
    m.close()
    assert [int(v) for v in d["sizes"][:7]] == [int(v) for v in reg["sizes"][:7]]
    return build(ctx, reg)


def check_fields(got, want, names, what):
    rel = U.field_rel(got, want)
    for f, r in zip(names, rel):
        print("%s %s: %.3e" % (what, f, r))
    for f, r in zip(names, rel):
        assert r <= (1e-13 if f == "rho" else 1e-12), (what, f, r)


# ---- 1. against the genuine reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.PLOT_FIXTURES)
def test_every_plot_point_as_a_probe_vs_reference(name):
    d = U.load(name)
    n_ppts, n_eles, n_fields = d["disu_ppts"].shape
    names = U.field_names(n_fields - 2)
    ctx = hfx.Context(0)
    e, faces = block(ctx, name)
    e.upload(hfx.DISU_UPTS0, d["u_init"])
    ctx.set_probes(names, probe_freq=1, capacity=2)
    ele = np.repeat(np.arange(n_eles), n_ppts)  # probe e * n_ppts + j: plot point j of element e
    e.set_probes(ele, np.tile(d["opp_p"].T, (1, n_eles)))
    e.sample_probes(1.5, 3)
    assert e.probe_count() == (1, n_eles * n_ppts)
    times, steps, values = e.read_probes()
    assert list(times) == [1.5] and list(steps) == [3] and values.shape == (len(names), n_eles * n_ppts, 1)
    want = U.probe_fields(d["disu_ppts"].transpose(1, 0, 2).reshape(-1, n_fields), names, ctx.params.gamma)
    check_fields(values[:, :, 0], want, names, name)
    close(e, faces, ctx)


# ---- 2. shapes ---------------------------------------------------------------------------------------------------------------
_rows = {}


def mirror_rows(order, n, seed):
    """operator rows of the mirror's set_opp_probe for a hexahedron of this order at n seeded random locations: (n_upts, n)"""
    if order not in _rows:
        _rows[order] = H.Case([3, 3, 3], order=order)
    loc = np.random.default_rng(seed).uniform(-1.0, 1.0, (3, n)).copy(order="F")
    return _rows[order].opp_probe(loc)


@pytest.mark.parametrize("n_probes", [1, 7, 64, 257])
@pytest.mark.parametrize("name,n_upts", [("hex_p2_n3_deformed", 27), ("hex_p3_plot", 64), ("hex_p4_jet", 125)])
def test_shapes(name, n_upts, n_probes):
    """n_upts below, equal to and above a wave with a remainder; probe counts that do and do not fill the last workgroup (four
    probes each); probes spread over the elements, all in one element, all in the last element"""
    ctx = hfx.Context(0)
    e, faces = block(ctx, name)
    assert e.n_upts == n_upts
    u = e.download(hfx.DISU_UPTS0)
    names = U.field_names(3)
    ctx.set_probes(names, probe_freq=1, capacity=1)
    opp = mirror_rows(e_order(n_upts), n_probes, seed=n_upts + n_probes)
    rng = np.random.default_rng(n_probes)
    for what, ele in (("spread", rng.integers(0, e.n_eles, n_probes)), ("one element", np.full(n_probes, e.n_eles // 2)),
                      ("last element", np.full(n_probes, e.n_eles - 1))):
        e.set_probes(ele, opp)
        e.sample_probes(0.0, 0)
        _, _, values = e.read_probes()
        want = U.probe_fields(U.interpolate(opp, np.asarray(ele), u), names, ctx.params.gamma)
        check_fields(values[:, :, 0], want, names, "%s %d probes, %s" % (name, n_probes, what))
    close(e, faces, ctx)


def e_order(n_upts):
    return int(round(n_upts ** (1.0 / 3.0))) - 1


def test_a_block_without_probes_is_accepted():
    ctx = hfx.Context(0)
    e, faces = block(ctx, "hex_p2_n3_deformed")
    ctx.set_probes(["rho"], probe_freq=1, capacity=3)
    e.set_probes([], np.zeros((e.n_upts, 0)))
    ctx.set_clock(TIME0, 0)
    hfx.run_steps(e, faces, 2, fused=3)
    assert e.probe_count() == (0, 0)
    assert e.read_probes()[2].shape == (1, 0, 0)
    close(e, faces, ctx)


# ---- 3. determinism ------------------------------------------------------------------------------------------------------------
def test_samples_are_reproducible_bit_for_bit_and_do_not_depend_on_the_order_of_registration():
    ctx = hfx.Context(0)
    e, faces = block(ctx, "hex_p4_jet")
    names = U.field_names(3)
    ctx.set_probes(names, probe_freq=1, capacity=2)
    n = 257
    opp = mirror_rows(4, n, seed=5)
    ele = np.random.default_rng(5).integers(0, e.n_eles, n)
    e.set_probes(ele, opp)
    e.sample_probes(0.0, 0)
    e.sample_probes(0.0, 0)
    _, _, v = e.read_probes()
    assert np.array_equal(v[:, :, 0], v[:, :, 1])
    perm = np.random.default_rng(6).permutation(n)
    e.set_probes(ele[perm], opp[:, perm])
    e.sample_probes(0.0, 0)
    _, _, w = e.read_probes()
    assert np.array_equal(w[:, :, 0], v[:, perm, 0])
    close(e, faces, ctx)


# ---- 4. in the loops -----------------------------------------------------------------------------------------------------------
LOOPS = {"per_method": ("hex_p2_n3_deformed", 0), "split_fused": ("hex_p2_n3_deformed", 3), "general_fused": ("tet_p2_n2_deformed", 4)}


def loop_probes(e):
    """a few probes in the first, a middle and the last element, rows of plausible magnitude (seeded)"""
    n = 9
    rng = np.random.default_rng(e.n_upts)
    opp = rng.uniform(-0.5, 1.0, (e.n_upts, n))
    ele = np.array([0, 0, e.n_eles // 2, e.n_eles - 1, 1, 2, e.n_eles - 1, 3, 4])
    return ele, opp


def run_loop(e, faces, n, fused):
    if fused == 4:
        hfx.run_steps_blocks([e], faces, n, fused=4)
    else:
        hfx.run_steps(e, faces, n, fused=fused)


def library_loop(name, fused, calls, names):
    """the clock set, probe_freq 2: the loop samples itself"""
    ctx = hfx.Context(0)
    e, faces = block(ctx, name)
    ctx.set_probes(names, probe_freq=2, capacity=4)
    e.set_probes(*loop_probes(e))
    ctx.set_clock(TIME0, 0)
    for n in calls:
        run_loop(e, faces, n, fused)
    out = e.read_probes()
    u = e.download(hfx.DISU_UPTS0)
    clock = ctx.get_clock()
    close(e, faces, ctx)
    return out, u, clock


@pytest.mark.parametrize("path", sorted(LOOPS))
def test_loop_samples_at_steps_2_and_4(path):
    """Five steps in one call with the clock set and probe_freq 2: exactly two samples, at steps 2 and 4, with the loop's own
    times; bitwise equal to one step per call (no clock) with hfx_eles_sample_probes by hand after steps 2 and 4, and to two
    calls of two and three steps."""
    name, fused = LOOPS[path]
    names = U.field_names(3)
    (times, steps, values), u5, clock = library_loop(name, fused, [5], names)
    assert list(steps) == [2, 4] and values.shape[2] == 2 and clock[1] == 5
    # by hand
    ctx = hfx.Context(0)
    e, faces = block(ctx, name)
    ctx.set_probes(names, probe_freq=2, capacity=4)
    e.set_probes(*loop_probes(e))
    time = TIME0
    for s in range(1, 6):
        run_loop(e, faces, 1, fused)
        time += ctx.get_dt()
        if s % 2 == 0:
            e.sample_probes(time, s)
    assert e.probe_count()[0] == 2  # (no clock: the loop itself took none)
    t_hand, s_hand, v_hand = e.read_probes()
    close(e, faces, ctx)
    (t23, s23, v23), _, _ = library_loop(name, fused, [2, 3], names)
    for i, f in enumerate(names):
        for k in range(2):
            scale = np.abs(v_hand[i, :, k]).max() or 1.0
            print("%s %s sample %d: one call of five against by hand %.3e, against calls of two and three %.3e (relative)"
                  % (path, f, k, np.abs(values[i, :, k] - v_hand[i, :, k]).max() / scale, np.abs(values[i, :, k] - v23[i, :, k]).max() / scale))
    assert list(times) == list(t_hand) and list(s_hand) == [2, 4]
    assert list(t23) == list(times) and list(s23) == [2, 4]
    assert np.array_equal(values, v_hand)
    assert np.array_equal(values, v23)


MIRROR_CFG = dict(order=2, amp=0.05, T_c_ic=300.0, dt=1e-4, riemann_solve_type=3)


def mirror_probe_positions(c):
    locs = np.random.default_rng(12).uniform(-0.6, 0.6, (3, 6)).copy(order="F")
    return c.calc_pos([0, 5, 5, c.n_eles - 1, 9, 20], locs)


def test_deferred_mirrored_loop_samples_at_steps_2_and_4():
    """the host mirror's RunSteps with deferred execution on, probe_freq 2, five steps: two samples, at steps 2 and 4 with the
    mirror's times; bitwise equal to five calls of one step with a sample by hand after the second and the fourth, and to calls
    of two and three steps.  Every stage still runs fused."""
    names = U.field_names(3)
    out = []
    for freq, calls in ((2, [5]), (1000, [1] * 5), (2, [2, 3])):
        c = H.Case([3, 3, 3], **MIRROR_CFG)
        c.set_probes(mirror_probe_positions(c), names, probe_freq=freq, capacity=4)
        c.to_device(0)
        done = 0
        for n in calls:
            c.run(n)
            done += n
            if freq == 1000 and done % 2 == 0:
                c.sample_probes()
        out.append(c.read_probes())
        dt = c.params().dt  # (the mirror's non-dimensional time step)
        n_fused, n_replayed, why = hfx.deferred_stats(c.handles()[0])
        assert n_replayed == 0, why
        c.close()
    (t5, s5, v5), (t1, s1, v1), (t23, s23, v23) = out
    assert list(s5) == [2, 4] and list(t5) == [0.0 + dt + dt, 0.0 + dt + dt + dt + dt]
    assert list(s1) == [2, 4] and list(t1) == list(t5) and list(s23) == [2, 4]
    assert v5.shape == (len(names), 6, 2)
    assert np.array_equal(v5, v1)
    assert np.array_equal(v5, v23)


def _partitioned_worker(rank, world, port, outdir):
    import faulthandler
    faulthandler.enable()
    import torch
    torch.cuda.set_device(0)
    dist = PU.init_pg(rank, world, port, "gloo")
    try:
        names = U.field_names(3)
        for tag, freq, calls in (("five", 2, [5]), ("hand", 1000, [1] * 5), ("two_three", 2, [2, 3])):
            c = H.Case([4, 4, 4], self_partition=[1, 0, 0], length=6.2831853071795862, **MIRROR_CFG)
            c.set_probes(mirror_probe_positions(c), names, probe_freq=freq, capacity=4)
            c.to_device(0)
            c.set_comm(hfx.comm_unique_id())
            done = 0
            for n in calls:
                c.run_partitioned(n)  # hfx_run_steps_partitioned: the clock handed to the library, which samples
                done += n
                if freq == 1000 and done % 2 == 0:
                    c.sample_probes()
            t, s, v = c.read_probes()
            np.save(os.path.join(outdir, tag + "_t.npy"), t)
            np.save(os.path.join(outdir, tag + "_s.npy"), s)
            np.save(os.path.join(outdir, tag + "_v.npy"), v)
            np.save(os.path.join(outdir, "dt.npy"), np.array([c.params().dt]))
            c.close()
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_partitioned_loop_samples_at_steps_2_and_4(tmp_path):
    """one self-partitioned rank through hfx_run_steps_partitioned (RCCL loop-back), as tests/test_gpu_time_average.py does"""
    from test_gpu_time_average import spawn_with_time_limit
    spawn_with_time_limit(_partitioned_worker, (str(tmp_path),), 240)
    get = lambda tag, k: np.load(str(tmp_path / ("%s_%s.npy" % (tag, k))))
    dt = float(np.load(str(tmp_path / "dt.npy"))[0])
    for tag in ("five", "hand", "two_three"):
        assert list(get(tag, "s")) == [2, 4], tag
        assert list(get(tag, "t")) == [dt + dt, dt + dt + dt + dt], tag
    v5, v1, v23 = get("five", "v"), get("hand", "v"), get("two_three", "v")
    assert v5.shape == (6, 6, 2) and np.abs(v5).max() > 0
    for i in range(6):
        scale = np.abs(v1[i]).max() or 1.0
        print("partitioned field %d: five against by hand %.3e, against two and three %.3e (relative)"
              % (i, np.abs(v5[i] - v1[i]).max() / scale, np.abs(v5[i] - v23[i]).max() / scale))
    assert np.array_equal(v5, v1)
    assert np.array_equal(v5, v23)


# ---- 5. nothing else moves -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", sorted(LOOPS))
def test_state_is_bit_identical_with_and_without_probes(path):
    name, fused = LOOPS[path]
    ctx = hfx.Context(0)
    e, faces = block(ctx, name)
    ctx.set_clock(TIME0, 0)
    run_loop(e, faces, 5, fused)
    plain = [e.download(i) for i in (hfx.DISU_UPTS0, hfx.DISU_UPTS1, hfx.DIV_TCONF_UPTS)]
    close(e, faces, ctx)
    (times, steps, values), u, clock = library_loop(name, fused, [5], U.field_names(3))
    assert values.shape[2] == 2 and np.abs(values).max() > 0
    assert np.array_equal(u, plain[0])
    ctx = hfx.Context(0)
    e, faces = block(ctx, name)
    ctx.set_probes(["pressure"], probe_freq=1, capacity=8)
    e.set_probes(*loop_probes(e))
    ctx.set_clock(TIME0, 0)
    run_loop(e, faces, 5, fused)
    for i, p in zip((hfx.DISU_UPTS0, hfx.DISU_UPTS1, hfx.DIV_TCONF_UPTS), plain):
        assert np.array_equal(e.download(i), p)
    assert e.probe_count()[0] == 5
    close(e, faces, ctx)


def test_mirror_state_and_deferred_stats_with_and_without_probes():
    """a case without probes runs exactly the stages it ran before -- every one fused, none replayed, the same state bit for
    bit -- and so does a case with them: a sample makes the pending stage run (fused) and adds its own launch, nothing else"""
    out = []
    for with_probes in (False, True):
        c = H.Case([3, 3, 3], **MIRROR_CFG)
        if with_probes:
            c.set_probes(mirror_probe_positions(c), ["rho", "pressure"], probe_freq=1, capacity=8)
        c.to_device(0)
        c.run(3)
        c.synchronize()
        ctx, e, f, nb = c.handles()
        u = np.zeros((c.n_upts, c.n_eles, c.n_fields), order="F")
        hfx.check(hfx.lib().hfx_eles_download(e, C.c_int(hfx.DISU_UPTS0), u.ctypes.data_as(hfx.dp)))
        out.append((u, hfx.deferred_stats(ctx)[:2], hfx.probe_count_of(e)))
        c.close()
    assert np.array_equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1] == (3 * 5, 0)
    assert out[0][2] == (0, 0) and out[1][2] == (3, 6)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def live_bytes():
    fn = hfx.lib().hfx_live_device_bytes_internal
    fn.restype = C.c_long
    return fn()


def test_refusals_and_the_history():
    ctx = hfx.Context(0)
    e, faces = block(ctx, "hex_p2_n3_deformed")
    ele, opp = loop_probes(e)
    with pytest.raises(hfx.HfxError, match="probe_freq"):
        ctx.set_probes(["rho"], probe_freq=0, capacity=2)
    with pytest.raises(hfx.HfxError, match="unknown probe field"):
        ctx.set_probes([6], probe_freq=1, capacity=2)
    with pytest.raises(hfx.HfxError, match="no probe fields"):
        e.sample_probes(0.0, 0)
    ctx.set_probes(["rho", "u"], probe_freq=2, capacity=2)
    for bad in (-1, e.n_eles):
        b = ele.copy()
        b[3] = bad
        with pytest.raises(hfx.HfxError, match="lies in element"):
            e.set_probes(b, opp)
    assert e.probe_count() == (0, 0)  # (a failed registration leaves nothing behind)
    e.set_probes(ele, opp)
    # a loop call whose samples exceed the free capacity: refused before any step
    ctx.set_clock(TIME0, 0)
    u0 = e.download(hfx.DISU_UPTS0)
    for fused in (0, 3):
        with pytest.raises(hfx.HfxError, match="take 3 samples"):
            hfx.run_steps(e, faces, 6, fused=fused)
    assert ctx.get_clock()[:2] == (TIME0, 0) and e.probe_count()[0] == 0
    assert np.array_equal(e.download(hfx.DISU_UPTS0), u0)
    hfx.run_steps(e, faces, 5, fused=3)  # two samples: the history is full
    assert e.probe_count() == (2, len(ele))
    with pytest.raises(hfx.HfxError, match="history is full"):
        e.sample_probes(1.0, 6)
    with pytest.raises(hfx.HfxError, match="take 1 samples"):
        hfx.run_steps(e, faces, 1, fused=3)  # step 6 would be the third
    assert ctx.get_clock()[1] == 5
    t, s, v = e.read_probes()
    assert list(s) == [2, 4] and e.probe_count()[0] == 0
    e.sample_probes(1.0, 6)  # after the read the same call succeeds
    hfx.run_steps(e, faces, 1, fused=3)
    assert list(e.read_probes()[1]) == [6, 6]
    close(e, faces, ctx)
    # w on a two-dimensional block
    ctx = hfx.Context(0)
    q, qfaces = block(ctx, "quad_p2_plot")
    ctx.set_probes(["u", "w"], probe_freq=1, capacity=1)
    with pytest.raises(hfx.HfxError, match="two-dimensional"):
        q.set_probes([0], np.ones((q.n_upts, 1)))
    close(q, qfaces, ctx)


def test_registering_again_and_destroying_give_the_memory_back():
    before = live_bytes()
    ctx = hfx.Context(0)
    e, faces = block(ctx, "hex_p2_n3_deformed")
    held = live_bytes()
    ele, opp = loop_probes(e)
    ctx.set_probes(U.field_names(3), probe_freq=1, capacity=16)
    e.set_probes(ele, opp)
    once = live_bytes()
    assert once > held
    e.sample_probes(0.0, 0)
    e.set_probes(ele[::-1].copy(), opp[:, ::-1])  # registering again replaces the probes and empties the history
    assert live_bytes() == once and e.probe_count() == (0, len(ele))
    ctx.set_probes(["rho"], probe_freq=1, capacity=16)  # other fields: the history is made anew when it is next needed
    e.sample_probes(0.0, 0)
    assert live_bytes() < once
    e.set_probes([], np.zeros((e.n_upts, 0)))
    assert live_bytes() == held
    e.set_probes(ele, opp)
    close(e, faces, ctx)
    assert live_bytes() == before


# ---- 7. through the mirror -----------------------------------------------------------------------------------------------------
def test_interior_plot_points_through_the_mirror():
    """hfxh_case_set_probes with the physical positions of the interior plot points of hex_p3_plot (eight per element), zero
    steps and one sample: the reference's disu_ppts at those points through the formulas, at the bar of the first test; with
    `dimensional` the values carry the reference factors"""
    d = U.load("hex_p3_plot")
    c, shape, _ = U.mirror("hex_p3_plot")
    n_ppts, n_eles, n_fields = d["disu_ppts"].shape
    interior = [j for j in range(n_ppts) if np.all(np.abs(d["loc_ppts"][:, j]) < 1 - 1e-12)]
    assert len(interior) == 8
    ele = np.repeat(np.arange(n_eles), len(interior))
    pts = np.tile(interior, n_eles)
    pos = c.calc_pos(ele, d["loc_ppts"][:, pts])
    names = U.field_names(3)
    c.set_probes(pos, [f.upper() for f in names], probe_freq=1, capacity=2)
    p = c.probes()
    assert np.array_equal(p["p2c"], ele) and np.array_equal(p["global_index"], np.arange(len(ele)))
    c.to_device(0)
    c.sync_host()
    assert np.abs(c.array("disu_upts0") - d["u_init"]).max() <= 1e-14 * np.abs(d["u_init"]).max()  # (the mirror's initial state is the fixture's)
    c.run(0)
    c.sample_probes()
    c.sample_probes()
    times, steps, values = c.read_probes()
    want = U.probe_fields(d["disu_ppts"][pts, ele, :], names, c.params().gamma)
    check_fields(values[:, :, 0], want, names, "mirror")
    c.sample_probes()
    t_dim, _, v_dim = c.read_probes(dimensional=True)
    r = c.ref_values()
    assert r["viscous"] == 1.0
    scale = {"rho": r["rho_ref"], "u": r["uvw_ref"], "v": r["uvw_ref"], "w": r["uvw_ref"],
             "specific_total_energy": r["uvw_ref"] * r["uvw_ref"], "pressure": r["p_ref"]}
    for i, f in enumerate(names):
        assert np.array_equal(v_dim[i, :, 0], values[i, :, 1] * scale[f]), f
    assert list(t_dim) == [times[0] * r["time_ref"]]
    c.close()
