"""Over-integration on triangles: the fixtures under tests/golden/tris_overint (tools/capture_tris_overint.py), the conditions each
meets, and the blocks the GPU tests cut out of them -- TEST INFRASTRUCTURE.

A fixture is a DELTA file on the fixture of tests/golden/tris it is based on: the three over-integration arrays of the genuine
reference (opp_over_int_cubpts, over_int_filter, JGinv_over_int_cubpts), over_int, the states of its run with over_int 1 and, where
the case changes keys of its base (to_p1_*: the inviscid vortex on tri_p1_n4_deformed's mesh), the arrays those keys change; every
other array is the base fixture's (the capture tool asserted that bit for bit).

The conditions (asserted by the capture tool before a file is written and recomputed by tests/test_tris_overint_oracle.py):
  1. the oracle in lockstep meets every dumped state at tri_util's bars;
  2. the run WITHOUT the over-integration arrays differs from the fixture's final state by more than MOVED = 1e-7 of max |u| -- 10^4
     times the GPU bar, so that a stage that silently skips de-aliasing cannot pass;
  3. the curved case: JGinv_over_int_cubpts varies over the cubature points of an element."""
import functools
import os

import numpy as np

import general_util as G
import tri_util as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tris_overint")
MOVED = 1e-7
OI_KEYS = ("over_int", "opp_over_int_cubpts", "over_int_filter", "JGinv_over_int_cubpts")
OWN = OI_KEYS + ("over_int_order",)                      # what every file holds of its own
RESULTS = ("s0_", "u_step", "dt_step", "dt_local_step")  # results of the run (the base fixture's are those of another run)
STALE = RESULTS + ("meta_json",)
N_STEPS = 2
CURVED = "to_p3_cylinder"
BY_ORDER = {1: "to_p1_o3", 2: "to_p2", 3: "to_p3", 4: "to_p4", 5: "to_p5"}
CUT_FROM = "to_p3"
NU = {1: 3, 2: 6, 3: 10, 4: 15, 5: 21}


def n_cubpts(over_int_order):
    return (over_int_order + 1) * (over_int_order + 2) // 2


def chunks_of(d):
    """(n_cubpts, chunk, chunks) the element kernel walks on block d: chunks of the order's solution points"""
    nc, nu = int(np.asarray(d["opp_over_int_cubpts"]).shape[0]), int(d["sizes"][1])
    return nc, nu, -(-nc // nu)


def names():
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz")) if os.path.isdir(GOLDEN) else []


def overlay(base, own):
    """the base fixture without its run's results, with the file's arrays on top"""
    own = dict(own)
    d = {k: v for k, v in base.items() if not k.startswith(STALE)}
    d.update(own)
    if "dropped" in own:  # (arrays of the base that a run with the case's keys does not have: the viscous operators of an inviscid run)
        import json
        for k in json.loads(bytes(own["dropped"]).decode()):
            d.pop(k)
    d.pop("dropped", None)
    return d


@functools.lru_cache(maxsize=None)
def _load(name):
    own = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    return overlay(T.load(bytes(own["based_on"]).decode()), own)


def load(name):
    return dict(_load(name))


def without_over_int(d):
    return {k: v for k, v in d.items() if k not in OI_KEYS}


def final_key(d, step):
    return "u_step%d_stage%d" % (step, int(d["sizes"][7]) - 1)


def metric_variation(d):
    """largest spread of JGinv_over_int_cubpts over the cubature points of an element, relative to its largest entry"""
    J = np.asarray(d["JGinv_over_int_cubpts"])
    return float((J.max(axis=2) - J.min(axis=2)).max() / np.abs(J).max())


def conditions(d, curved=False):
    """-> dict of failures (empty: all met), moved, metric_variation, worst (key, error) of the lockstep"""
    errs = T.lockstep(d)
    failures = dict(T.failures(errs))
    worst = max(((k, v) for k, v in errs.items() if not k.startswith("nan_")), key=lambda kv: kv[1][0] / kv[1][1])
    steps = max(T.stored_steps(d)) + 1
    plain = G.oracle_steps(without_over_int(d), steps)
    moved = T.relerr(plain[-1]["u"], d[final_key(d, steps - 1)])
    if not moved > MOVED:
        failures["moved"] = (moved, MOVED)
    var = metric_variation(d)
    if curved and not var > 1e-4:
        failures["metric_variation"] = (var, 1e-4)
    return dict(failures=failures, moved=moved, metric_variation=var, worst=(worst[0], worst[1][0]))


_references = {}


def reference(name):
    """the oracle's steps on fixture `name` (general_util.oracle_steps), computed once and shared (read-only)"""
    if name not in _references:
        d = load(name)
        _references[name] = G.oracle_steps(d, max(T.stored_steps(d)) + 1)
    return _references[name]


# ---- the blocks the GPU tests cut: tri_util's seeded choice and boundary records on the fixture WITH its over-integration arrays -----
@functools.lru_cache(maxsize=None)
def block(n, name=CUT_FROM, viscous=None):
    """n elements of fixture `name` as tri_util.block cuts them (tiled first where it has fewer than 2 n; the cut faces carry the
    boundary records of tri_p3_bdy in a seeded order, isothermal walls alone on an inviscid state); viscous 0: the same block
    run inviscid"""
    d = load(name)
    ne = int(d["sizes"][0])
    inviscid = (int(np.ravel(d["viscous"])[0]) if viscous is None else viscous) == 0  # (the library refuses adiabatic walls without viscous terms)
    if ne < 2 * n:
        d = G.tile(d, (2 * n + ne - 1) // ne)
    rng = np.random.default_rng(7000 + n)
    keep = rng.permutation(int(d["sizes"][0]))[:n]
    bc = T.load(T.BC_FROM)
    fl = np.asarray(bc["bc_flags"]).reshape(3, -1, order="F")
    kinds = (8,) if inviscid else None  # (tri_util.KINDS: what the vortex state takes)
    ids = rng.permutation([i for i in range(fl.shape[1]) if fl[1, i] == 0])
    b = G.cut(d, keep, bc, [i for i in ids if kinds is None or fl[0, i] in kinds])
    if viscous is not None:
        b["viscous"] = np.array([viscous], dtype=np.asarray(d["viscous"]).dtype)
    return b


def edge_counts(name):
    g = T.GROUP[int(_load(name)["sizes"][5])]
    return [g - 1, g, g + 1, 2 * g + 1]


def order_blocks():
    """(fixture, n): blocks of G - 1, G, G + 1 and 2 G + 1 elements at every instantiated order"""
    return [(BY_ORDER[p], n) for p in sorted(BY_ORDER) for n in edge_counts(BY_ORDER[p])]


@functools.lru_cache(maxsize=None)
def perturbed_block():
    """a P3 block of G + 1 elements whose JGinv_over_int_cubpts is multiplied by a seeded 1 + 0.1 xi, xi uniform in [-1, 1), per
    (l, n, m, ele): on the straight-sided boxes the metric is constant within an element, so that only this block (and the cylinder)
    pins the per-point index"""
    b = dict(block(T.GROUP[3] + 1))
    J = np.asarray(b["JGinv_over_int_cubpts"])
    xi = np.random.default_rng(4242).uniform(-1.0, 1.0, size=J.shape)
    b["JGinv_over_int_cubpts"] = np.asfortranarray(J * (1.0 + 0.1 * xi))
    return b


def block_reference(key, d):
    if key not in _references:
        _references[key] = G.oracle_steps(d, N_STEPS)
    return _references[key]


# ---- with shock capturing: a ts_* fixture's registration (same mesh) on the over-integrated block ------------------------------------
SHOCK_ON = {"to_p3": "ts_p3_n4", "to_p3_cylinder": "ts_p3_cylinder"}


@functools.lru_cache(maxsize=None)
def _with_shock(name):
    import tri_shock_util as TS
    d, s = load(name), TS.load(SHOCK_ON[name])
    for k in ("u_init", "opp_0", "detjac_upts", "sizes", "adv_type", "dt_type"):
        assert np.array_equal(d[k], s[k]), k  # (the same mesh, keys and initial state)
    for k in TS.SHOCK_KEYS:
        d[k] = s[k]
    ref = TS.lockstep(d, N_STEPS)
    TS.check_conditions(ref["stage_sensors"], TS.scalar(d, "s0"), name + " with " + SHOCK_ON[name])
    assert ref["bad"] == -1
    return d, ref


def with_shock(name):
    """-> (fixture `name` with the shock keys of SHOCK_ON[name], tri_shock_util.lockstep over N_STEPS steps: the oracle with both
    ingredients; conditions 3 and 4 of tests/tri_shock_util.py asserted on it)"""
    d, ref = _with_shock(name)
    return dict(d), ref
