"""The LES closure on triangles: the fixtures under tests/golden/tris_les (tools/capture_tris_les.py), the conditions each meets, and
the blocks the GPU tests cut out of them -- TEST INFRASTRUCTURE.

A fixture is a DELTA file on the fixture of tests/golden/tris it is based on: the closure's keys and arrays of the genuine reference
(LES, SGS_model, C_s, filter_ratio, Kappa, prandtl_t, Jacobian_fpts and, by model, wall_distance / filter_upts) and the states of its
run with LES 1; every other array is the base fixture's (the capture tool asserted that bit for bit).  tl_p3_smag_walls has no base
(its mesh is new) and is stored whole.

The conditions (asserted by the capture tool before a file is written and recomputed by tests/test_tris_les_oracle.py):
  1. the oracle in lockstep (general_util.oracle_steps: calc_sgs_terms at a step's first stage) meets every dumped state at tri_util's
     bars;
  2. the run WITHOUT the closure differs from the fixture's final state by more than MOVED = 1e-7 of max |u| -- 10^4 times the GPU bar,
     so that a stage that silently skips the closure cannot pass;
  3. sum_k Jacobian_fpts(i, k) JGinv_fpts(k, j) = detjac_fpts delta_ij at every flux point, to JACOBIAN_CAPTURE = 1e-12 of max
     |detjac_fpts| (the fused stage, which projects the SGS flux with the block's own metrics, asks for 1e-9: JACOBIAN_STAGE);
  4. tl_p3_smag_walls: the wall term y^2 Kappa^2 is the smaller squared length scale at some solution points and C_s^2 Delta^2 at others;
  5. the similarity closures (models 2, 4): the Leonard terms Lu, Le of the first step are non-zero.

tl_p3_cylinder_shock (SHOCK) is the closure beside shock capturing through the genuine DRIVER: it holds the closure's scalars and the
driver's restart state and Tecplot sensor, and takes every array from ts_p3_cylinder and tl_p3_cylinder (compose_shock); its
conditions are shock_conditions below."""
import ctypes as C
import functools
import json
import os

import numpy as np

import general_util as G
import tri_util as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tris_les")
MOVED = 1e-7
JACOBIAN_CAPTURE, JACOBIAN_STAGE = 1e-12, 1e-9
LES_SCALARS = ("LES", "SGS_model", "C_s", "filter_ratio", "Kappa", "prandtl_t")
LES_KEYS = LES_SCALARS + ("Jacobian_fpts", "wall_distance", "filter_upts")
RESULTS = ("s0_", "u_step", "dt_step", "dt_local_step")  # results of the run (the base fixture's are those of another run)
STALE = RESULTS + ("meta_json",)
N_STEPS = 2
BY_ORDER = {1: "tl_p1_wale", 2: "tl_p2_wale", 3: "tl_p3_wale", 4: "tl_p4_wale", 5: "tl_p5_wale"}
WALLS, CYLINDER, SVV = "tl_p3_smag_walls", "tl_p3_cylinder", "tl_p3_svv"
SIMILARITY = ("tl_p3_wsm", "tl_p3_sim")


SHOCK = "tl_p3_cylinder_shock"  # the closure beside shock capturing, through the genuine DRIVER (below: load_shock)


def names():
    """the fixtures of the harness (SHOCK, which holds the driver's files instead of u_step*, is loaded by load_shock)"""
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz") and f[:-4] != SHOCK) if os.path.isdir(GOLDEN) else []


def overlay(base, own):
    """the base fixture without its run's results, with the file's arrays on top"""
    d = {k: v for k, v in base.items() if not k.startswith(STALE)}
    d.update(own)
    return d


@functools.lru_cache(maxsize=None)
def _load(name):
    own = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    if "based_on" not in own:
        return own
    return overlay(T.load(bytes(own["based_on"]).decode()), own)


def load(name):
    return dict(_load(name))


def scalar(d, k):
    return float(np.ravel(d[k])[0])


def model(d):
    return int(scalar(d, "SGS_model")) if "LES" in d and int(scalar(d, "LES")) else -1


def without_les(d):
    return {k: v for k, v in d.items() if k not in LES_KEYS}


def final_key(d, step):
    return "u_step%d_stage%d" % (step, int(d["sizes"][7]) - 1)


def n_steps_of(d):
    return max(T.stored_steps(d)) + 1


def fixture_states(d):
    """the genuine reference's state after every step of the fixture (None: not stored -- the cylinder keeps the last alone)"""
    return [d.get(final_key(d, st)) for st in range(n_steps_of(d))]


def jacobian_residual(Jacobian_fpts, d):
    """max |sum_k Jacobian_fpts(i, k) JGinv_fpts(k, j) - detjac_fpts delta_ij| / max |detjac_fpts|"""
    J, JG, dj = np.asarray(Jacobian_fpts), np.asarray(d["JGinv_fpts"]), np.asarray(d["detjac_fpts"])
    P = np.einsum("ikfe,kjfe->ijfe", J, JG)
    P[0, 0] -= dj
    P[1, 1] -= dj
    return float(np.abs(P).max() / np.abs(dj).max())


def length_scales(d):
    """(y^2 Kappa^2, C_s^2 Delta^2) at every solution point of a Smagorinsky fixture (src/eles.cpp:2436-2520; triangles: vol = 2 detjac)"""
    w = np.asarray(d["wall_distance"])
    y2 = (w ** 2).sum(axis=2)
    delta = scalar(d, "filter_ratio") * np.sqrt(2.0 * np.asarray(d["detjac_upts"])) / (int(d["sizes"][5]) + 1.0)
    return y2 * scalar(d, "Kappa") ** 2, scalar(d, "C_s") ** 2 * delta ** 2


def leonard_terms(d):
    """(max |Lu|, max |Le|) of the first calc_sgs_terms on the fixture's initial state (the oracle's)"""
    import oracle_py as O
    o = O.load()
    c = O.Case(d)
    e = c.c_eles()
    assert o.orc_calc_sgs_terms(C.byref(e)) < 0
    return float(np.abs(c.arr["Lu"]).max()), float(np.abs(c.arr["Le"]).max())


def lockstep(d):
    """the oracle's steps (general_util.oracle_steps) against every stored state -> {key: (error, bar)}, the steps"""
    ref = G.oracle_steps(d, n_steps_of(d))
    bar = T.RTOL_BDY if any(k.startswith("bdy") for k in d) else T.RTOL
    errs = {}
    for st, r in enumerate(ref):
        errs["nan_step%d" % st] = (0.0 if r["bad"] == -1 else 1.0, 0.5)
        if final_key(d, st) in d:
            errs[final_key(d, st)] = (T.relerr(r["u"], d[final_key(d, st)]), bar)
    return errs, ref


def conditions(d, name=""):
    """-> dict of failures (empty: all met), moved, jacobian, worst (key, error) of the lockstep, and what the case's own condition found"""
    errs, _ = lockstep(d)
    failures = dict(T.failures(errs))
    worst = max(((k, v) for k, v in errs.items() if not k.startswith("nan_")), key=lambda kv: kv[1][0] / kv[1][1])
    steps = n_steps_of(d)
    plain = G.oracle_steps(without_les(d), steps)
    moved = T.relerr(plain[-1]["u"], d[final_key(d, steps - 1)])
    if not moved > MOVED:
        failures["moved"] = (moved, MOVED)
    jac = jacobian_residual(d["Jacobian_fpts"], d)
    if not jac < JACOBIAN_CAPTURE:
        failures["jacobian"] = (jac, JACOBIAN_CAPTURE)
    out = dict(failures=failures, moved=moved, jacobian=jac, worst=(worst[0], worst[1][0]))
    if model(d) == 0:
        wall, grid = length_scales(d)
        out["wall_points"], out["grid_points"] = int((wall < grid).sum()), int((grid < wall).sum())
        if name == WALLS and not (out["wall_points"] > 0 and out["grid_points"] > 0):
            failures["length_scales"] = (out["wall_points"], out["grid_points"])
    if model(d) in (2, 4):
        out["Lu"], out["Le"] = leonard_terms(d)
        if not (out["Lu"] > 0.0 and out["Le"] > 0.0):
            failures["leonard"] = (out["Lu"], out["Le"])
    return out


# ---- the closure beside shock capturing: the shipped viscous cylinder keys + LES 1 through the genuine driver ---------------------------
def compose_shock(own):
    """the block of a SHOCK file: the arrays and shock keys of the ts_* fixture it names (tests/tri_shock_util.py), the closure's arrays
    of the tl_* fixture it names (the same mesh), and on top what the file holds itself: the closure's scalars and the driver's files
    (u_restart, restart_steps, sensor_rows, as in a ts_* fixture)"""
    import tri_shock_util as TS
    d = {k: v for k, v in TS.load(bytes(own["shock_from"]).decode()).items()
         if k not in ("u_restart", "restart_steps", "sensor_rows", "meta_json", "based_on")}
    les = _load(bytes(own["les_from"]).decode())
    for k in ("sizes", "u_init", "detjac_fpts", "JGinv_fpts", "opp_0"):
        assert np.array_equal(d[k], les[k]), k  # (the same mesh, order and initial state)
    d.update({k: les[k] for k in LES_KEYS if k in les})
    d.update(own)
    return d


@functools.lru_cache(maxsize=None)
def _load_shock():
    return compose_shock(dict(np.load(os.path.join(GOLDEN, SHOCK + ".npz"))))


def load_shock():
    return dict(_load_shock())


def shock_conditions(d):
    """the conditions of a SHOCK block: the oracle in lockstep (tri_shock_util.lockstep: the closure in CalcResidual, the filter behind
    every stage) meets the driver's restart state at 1e-12 and its Tecplot sensor at 1e-10 of the largest (tri_shock_util's bars: 15
    printed digits); conditions 3 and 4 of tests/tri_shock_util.py (no sensor within 5e-4 of s0; some stage filters some elements and
    not all); the run without the closure differs from the driver's final state by more than MOVED; the Jacobian identity
    -> dict of failures (empty: all met), the figures, and the lockstep"""
    import tri_shock_util as TS
    steps = TS.n_steps_of(d)
    s0 = TS.scalar(d, "s0")
    ref = TS.lockstep(d, steps)
    failures = {}
    rs = [int(s) for s in np.ravel(d["restart_steps"])]
    state = max(T.relerr(ref["u"][s - 1], d["u_restart"][i]) for i, s in enumerate(rs))
    big = np.abs(d["sensor_rows"]).max()
    sensor = max(float(np.abs(ref["sensor"][s] - d["sensor_rows"][s]).max() / big) for s in range(steps))
    gap = TS.closest(ref["stage_sensors"], s0)
    counts = TS.filtered_counts(ref["stage_sensors"], s0)
    ne = int(d["sizes"][0])
    moved = T.relerr(TS.lockstep(without_les(d), steps)["u"][rs[-1] - 1], d["u_restart"][-1])
    jac = jacobian_residual(d["Jacobian_fpts"], d)
    for key, ok, fig in (("state", state <= TS.TOL_STATE, state), ("sensor", sensor <= TS.TOL_SENSOR, sensor), ("margin", gap > TS.MARGIN, gap),
                         ("filtered", any(0 < c < ne for c in counts), counts), ("moved", moved > MOVED, moved),
                         ("jacobian", jac < JACOBIAN_CAPTURE, jac), ("nan", ref["bad"] == -1, ref["bad"])):
        if not ok:
            failures[key] = fig
    return dict(failures=failures, state=state, sensor=sensor, closest_sensor_to_s0=gap, filtered_per_stage=counts, moved=moved,
                jacobian=jac), ref


def shock_reference():
    """tri_shock_util.lockstep of the SHOCK block over its steps, computed once and shared (read-only)"""
    if SHOCK not in _references:
        _references[SHOCK] = shock_conditions(load_shock())[1]
    return _references[SHOCK]


_references = {}


def reference(name):
    """the oracle's steps on fixture `name`, computed once and shared (read-only)"""
    if name not in _references:
        d = load(name)
        _references[name] = G.oracle_steps(d, n_steps_of(d))
    return _references[name]


# ---- the blocks the GPU tests cut: tri_util's seeded choice and boundary records on the fixture WITH its closure ----------------------
@functools.lru_cache(maxsize=None)
def block(n, name):
    """n elements of fixture `name` as tri_util.block cuts them (tiled first where it has fewer than 2 n; the cut faces carry the
    boundary records of tri_p3_bdy in a seeded order); wall_distance and Jacobian_fpts are sliced with the elements"""
    d = load(name)
    ne = int(d["sizes"][0])
    if ne < 2 * n:
        d = G.tile(d, (2 * n + ne - 1) // ne)
    rng = np.random.default_rng(7000 + n)
    keep = rng.permutation(int(d["sizes"][0]))[:n]
    bc = T.load(T.BC_FROM)
    fl = np.asarray(bc["bc_flags"]).reshape(3, -1, order="F")
    ids = rng.permutation([i for i in range(fl.shape[1]) if fl[1, i] == 0])
    return G.cut(d, keep, bc, list(ids))


def edge_counts(name):
    g = T.GROUP[int(_load(name)["sizes"][5])]
    return [g - 1, g, g + 1, 2 * g + 1]


def order_blocks():
    """(fixture, n): blocks of G - 1, G, G + 1 and 2 G + 1 elements at every instantiated order"""
    return [(BY_ORDER[p], n) for p in sorted(BY_ORDER) if BY_ORDER[p] in names() for n in edge_counts(BY_ORDER[p])]


def similarity_block():
    """2 G + 1 elements of tl_p3_wsm: Lu / Le are indexed with e0 > 0"""
    return block(2 * T.GROUP[3] + 1, "tl_p3_wsm")


TILES = 3


@functools.lru_cache(maxsize=None)
def _tiled(name):
    return G.tile(load(name), TILES)


def tiled(name):
    """TILES disjoint copies of a fixture of ONE group (general_util.tile): virtual parts that cut the first copy leave the groups of
    the others interior"""
    return dict(_tiled(name))


def block_reference(key, d):
    if key not in _references:
        _references[key] = G.oracle_steps(d, N_STEPS)
    return _references[key]


def meta(name):
    return json.loads(bytes(np.load(os.path.join(GOLDEN, name + ".npz"))["meta_json"]).decode())
