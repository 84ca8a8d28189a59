"""Shock capturing on triangles: the fixtures under tests/golden/tris_shock (tools/capture_tris_shock.py), the oracle in lockstep
with them -- orc_CalcResidual_bdy, orc_AdvanceSolution, orc_shock_capture per stage, as the reference's main loop calls them
(src/HiFiLES.cpp:198-216) -- and the blocks the GPU tests cut out of them -- TEST INFRASTRUCTURE.

A fixture holds the arrays a block is built from (those of the fixture of tests/golden/tris it is based on; ts_p3_cylinder holds
only what is new and takes them from tests/golden/tris/tri_p3_cylinder.npz), the operators of eles_tris rebuilt in numpy
(hfx.tri_shock_operators), the keys, and what the genuine DRIVER wrote with shock_cap 1: u_restart[i], the state of its restart file
after step restart_steps[i], and sensor_rows[s], the sensor column of its Tecplot file after step s + 1 (per element).

The conditions every fixture, cut block and virtual partition meets (asserted here over every stage a lockstep returns):
  3. no sensor value of any stage lies within MARGIN = 5e-4 of s0, relative to s0 (rounding cannot flip an element);
  4. in some stage at least one element is filtered and at least one is not (a block of ONE element: it is filtered in some stage)."""
import ctypes as C
import functools
import os

import numpy as np

import tri_util as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tris_shock")
MARGIN = 5e-4
TOL_STATE, TOL_SENSOR = 1e-12, 1e-10  # the oracle against the driver's files (15 printed digits)
SHOCK_KEYS = ("shock_cap", "inv_vandermonde", "exp_filter", "norm_basis_persson", "persson_high_modes", "s0", "shock_det_field",
              "expf_fac", "expf_order", "expf_cutoff")
# results of the base fixture's run without a filter
STALE = ("s0_", "u_step", "dt_step", "dt_local_step", "meta_json")
CUT_FROM = "ts_p3_n4"
G_P3 = T.GROUP[3]
# the virtual parts of the GPU tests (test_tris_partition_oracle.grow_parts: weights, seed).  The cylinder's: 17 partition and 6
# interior groups, and the stages that filter at all filter elements of both kinds (tests/test_tris_shock_oracle.py)
PARTS = {"ts_p3_n4": ([3, 2, 1], 3), "ts_p3_cylinder": ([20, 1, 1], 1)}
BY_ORDER = {1: "ts_p1_n4", 2: "ts_p2_n3", 3: "ts_p3_n4", 4: "ts_p4_n2", 5: "ts_p5_n2"}


def names():
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz")) if os.path.isdir(GOLDEN) else []


@functools.lru_cache(maxsize=None)
def _load(name):
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    if "based_on" in d and "u_init" not in d:  # (what the fixture does not hold: the arrays of the fixture it is based on)
        for k, v in T.load(bytes(d["based_on"]).decode()).items():
            if not k.startswith(STALE):
                d.setdefault(k, v)
    return d


def load(name):
    return dict(_load(name))


def scalar(d, k):
    return float(np.ravel(d[k])[0])


def n_steps_of(d):
    return int(np.asarray(d["sensor_rows"]).shape[0])


def choose_s0(sensors, skip=0):
    """the middle of the widest relative gap (the (skip + 1)-th widest) between neighbours in the upper half of the sorted values,
    rounded to five digits; one value: half of it"""
    v = np.sort(np.asarray(sensors, dtype=np.float64))
    if v.size == 1:
        return float("%.4e" % (0.5 * v[0]))
    lo = min(v.size // 2, v.size - 2)
    ratio = v[lo + 1:] / v[lo:-1]
    i = lo + int(np.argsort(-ratio, kind="stable")[min(skip, ratio.size - 1)])
    return float("%.4e" % (0.5 * (v[i] + v[i + 1])))


def lockstep(d, n_steps, shock=True, s0=None, dt_map=None):
    """the oracle on block d, the filter behind every stage (shock False: the sensor is computed and nothing is filtered)
    -> dict of u (per step), sensor (per step: the last stage's), stage_sensors (n_steps * n_stages, n_eles), bad.
    dt_map (dt_type 2): what a deliberately WRONG run does to the local time steps before it uses them"""
    import oracle_py as O
    o = O.load()
    d = dict(d)
    if s0 is not None:
        d["s0"] = np.array([s0])
    if not shock:
        d["s0"] = np.array([np.inf])
    c = O.Case(d)
    e = c.c_eles()
    f, nfb = c.c_faces()
    bd, nbd = c.c_bdy()
    sh = c.c_shock()
    nstage = int(d["sizes"][7])
    dt_type = int(np.ravel(d["dt_type"])[0])
    out = dict(u=[], sensor=[], stage_sensors=[], bad=-1)
    for st in range(n_steps):
        if dt_type != 0:
            CFL, order, h = scalar(d, "CFL"), int(d["sizes"][5]), np.ravel(d["h_ref"])
            dtl = np.array([o.orc_calc_dt_local(C.byref(e), C.byref(c.params), i, h[i], CFL, order) for i in range(c.n_eles)])
            c.params.dt = dtl.min()
            if dt_type == 2:
                dtl = dtl if dt_map is None else np.ascontiguousarray(dt_map(dtl))
                c._dtl = dtl
                e.dt_local = dtl.ctypes.data_as(O.dp)
        for rk in range(nstage):
            out["bad"] = max(out["bad"], o.orc_CalcResidual_bdy(C.byref(e), f, nfb, bd, nbd, C.byref(c.params)))
            o.orc_AdvanceSolution(C.byref(e), C.byref(c.params), rk)
            o.orc_shock_capture(C.byref(e), C.byref(sh))
            out["stage_sensors"].append(c.arr["sensor"].copy())
        out["u"].append(c.arr["u0"].copy(order="F"))
        out["sensor"].append(c.arr["sensor"].copy())
    out["stage_sensors"] = np.array(out["stage_sensors"])
    return out


def filtered_counts(stage_sensors, s0):
    return [int((s >= s0).sum()) for s in stage_sensors]


def closest(stage_sensors, s0):
    """the smallest distance of a sensor value of any stage from s0, relative to s0"""
    return float(np.abs(np.asarray(stage_sensors) - s0).min() / s0)


def check_conditions(stage_sensors, s0, what):
    """conditions 3 and 4 over every stage"""
    stage_sensors = np.asarray(stage_sensors)
    assert np.isfinite(stage_sensors).all(), what
    gap = closest(stage_sensors, s0)
    assert gap > MARGIN, "%s: a sensor value lies within %.1e of s0 = %.4e" % (what, gap, s0)
    counts = filtered_counts(stage_sensors, s0)
    ne = stage_sensors.shape[1]
    assert any(0 < c < ne for c in counts) or (ne == 1 and any(counts)), "%s: filtered per stage %s of %d" % (what, counts, ne)
    return counts


_references = {}


def reference(name, shock=True):
    """lockstep of fixture `name` over its steps, computed once and shared (read-only); conditions 3 and 4 asserted"""
    key = (name, shock)
    if key not in _references:
        d = load(name)
        _references[key] = lockstep(d, n_steps_of(d), shock)
        if shock:
            check_conditions(_references[key]["stage_sensors"], scalar(d, "s0"), name)
    return _references[key]


# ---- the blocks the GPU tests cut: tri_util.block(n, base) of the fixture a ts_* file is based on, with that file's operators ---------
N_STEPS = 2


@functools.lru_cache(maxsize=None)
def block(n, name=CUT_FROM):
    """-> (block with the shock keys, its lockstep over N_STEPS steps); s0: the middle of the widest upper-half gap of the first stage's
    oracle sensors (the next-widest where a later stage comes within MARGIN)"""
    src = load(name)
    based_on = bytes(src["based_on"]).decode()
    base = T.load(based_on)
    for k in ("u_init", "opp_0", "opp_3", "detjac_upts", "int0_L", "sizes", "adv_type", "dt_type", "RK_a", "RK_b"):
        assert np.array_equal(src[k], base[k]), k  # (tri_util.block cuts the fixture `name` is based on: the same arrays)
    b = dict(T.block(n, based_on))
    for k in SHOCK_KEYS:
        b[k] = src[k]
    first = lockstep(b, 1, shock=False)["stage_sensors"][0]
    for skip in range(max(1, min(6, n // 2))):
        s0 = choose_s0(first, skip)
        ref = lockstep(b, N_STEPS, s0=s0)
        if closest(ref["stage_sensors"], s0) > MARGIN and (n == 1 or any(0 < c < n for c in filtered_counts(ref["stage_sensors"], s0))):
            break
    b["s0"] = np.array([s0])
    check_conditions(ref["stage_sensors"], s0, "block of %d of %s" % (n, name))
    assert ref["bad"] == -1
    return b, ref


def group_of_filtered(stage_sensors, s0, G):
    """per stage the set of groups (of G consecutive elements) with a filtered element"""
    return [sorted(set((np.nonzero(s >= s0)[0] // G).tolist())) for s in stage_sensors]
