"""Element blocks of ANY element count for the general fused stage (csrc/general.hip): TEST INFRASTRUCTURE.

The general stage works on batches of 16 elements; the simplex fixtures hold 48 tetrahedra or 16 prisms -- whole batches.  tile()
makes a block larger, cut() keeps any list of its elements in any order: every per-element array is sliced, the face tables are
renumbered, and a face pair that loses one side becomes a BOUNDARY face of the side that stays, with the boundary records of
hex_p2_bdy_walls (six kinds: sub_in_char, isotherm_wall, slip_wall, adiabat_wall, char, sub_out_char) dealt round-robin.  The
genuine reference never ran such a block: its reference is the oracle on the same block (oracle_steps), which the oracle tests pin
on every uncut fixture; a cut that keeps ALL elements in another order has the genuine reference's states, permuted.

A table entry is fpt + n_fpts * ele (hf_array order of the (n_fpts, n_eles) plane)."""
import ctypes as C
import functools
import os

import numpy as np

import mixed_util as MU

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BC_FROM = "hex_p2_bdy_walls"
# where the element axis sits
LAST_AXIS = ("shape", "JGinv_upts", "JGinv_fpts", "Jacobian_fpts", "JGinv_over_int_cubpts")
AXIS_1 = ("detjac_upts", "detjac_fpts", "tdA_fpts", "norm_fpts", "pos_upts", "pos_fpts", "u_init", "wall_distance")
AXIS_0 = ("h_ref",)
# results of the uncut run that no longer describe the block
STALE = ("s0_", "dt_step", "dt_local_step")


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def _axis(key):
    """the element axis of a per-element array of a single-class fixture (None: not per element)"""
    if key in LAST_AXIS:
        return -1
    if key in AXIS_1 or key.startswith("u_step"):
        return 1
    if key in AXIS_0:
        return 0
    return None


def _take(a, keep, axis):
    return np.asfortranarray(np.take(a, keep, axis=axis))


def _renumber(col, new, nfp):
    return (new[col // nfp] * nfp + col % nfp).astype(np.int32)


def _merge_bcs(d, out, bc_from):
    """the boundary records of bc_from behind the fixture's own -> the id of bc_from's first record"""
    if bc_from is None:
        return 0
    fl, par = np.asarray(bc_from["bc_flags"]).reshape(3, -1, order="F"), np.asarray(bc_from["bc_params"]).reshape(15, -1, order="F")
    first = 0
    if "bc_flags" in d:
        own_fl, own_par = np.asarray(d["bc_flags"]).reshape(3, -1, order="F"), np.asarray(d["bc_params"]).reshape(15, -1, order="F")
        assert float(np.ravel(d["bc_R_ref"])[0]) == float(np.ravel(bc_from["bc_R_ref"])[0])
        first = own_fl.shape[1]
        fl, par = np.concatenate([own_fl, fl], axis=1), np.concatenate([own_par, par], axis=1)
    out["bc_flags"], out["bc_params"] = np.asfortranarray(fl.astype(np.int32)), np.asfortranarray(par)
    out["bc_R_ref"] = np.array(bc_from["bc_R_ref"])
    out["ramp_counter"] = np.array(d["ramp_counter"] if "ramp_counter" in d else bc_from["ramp_counter"])
    return first


def _cut_faces(d, out, new, nfp, classes, ids, first_id):
    """face tables of the kept elements.  new[c]: old element -> new element or -1; nfp[c]: flux points per element of class c;
    a mixed fixture carries the class of every face side (int<t>_cl / _cr, bdy<t>_cl), a single-class one does not"""
    mixed = len(classes) > 1 or "classes" in d
    dealt = 0
    for t in range(3):
        kL, kR, kB, kI = "int%d_L" % t, "int%d_R" % t, "bdy%d_L" % t, "bdy%d_id" % t
        bL, bid, bcl = [], [], []
        if kB in d:  # the fixture's own boundary faces
            L, idv = np.asarray(d[kB]), np.ravel(d[kI])
            cl = np.ravel(d["bdy%d_cl" % t]) if mixed else np.full(L.shape[1], classes[0])
            for c in range(L.shape[1]):
                k = int(cl[c])
                if new[k][L[0, c] // nfp[k]] >= 0:
                    bL.append(_renumber(L[:, c], new[k], nfp[k])); bid.append(int(idv[c])); bcl.append(k)
        iL, iR, icl, icr = [], [], [], []
        if kL in d:
            L, R = np.asarray(d[kL]), np.asarray(d[kR])
            cl = np.ravel(d["int%d_cl" % t]) if mixed else np.full(L.shape[1], classes[0])
            cr = np.ravel(d["int%d_cr" % t]) if mixed else np.full(L.shape[1], classes[0])
            for c in range(L.shape[1]):
                a, b = int(cl[c]), int(cr[c])
                ea, eb = L[0, c] // nfp[a], R[0, c] // nfp[b]
                assert (L[:, c] // nfp[a] == ea).all() and (R[:, c] // nfp[b] == eb).all()  # a face belongs to one element per side
                ka, kb = new[a][ea] >= 0, new[b][eb] >= 0
                if ka and kb:
                    iL.append(_renumber(L[:, c], new[a], nfp[a])); iR.append(_renumber(R[:, c], new[b], nfp[b]))
                    icl.append(a); icr.append(b)
                elif ka or kb:  # the side that stays faces the boundary now
                    assert ids is not None and len(ids) > 0, "a cut face needs boundary ids"
                    col, k = (L[:, c], a) if ka else (R[:, c], b)
                    bL.append(_renumber(col, new[k], nfp[k])); bid.append(first_id + int(ids[dealt % len(ids)])); bcl.append(k)
                    dealt += 1
        for k in (kL, kR, kB, kI, "int%d_cl" % t, "int%d_cr" % t, "bdy%d_cl" % t):
            out.pop(k, None)
        if iL:  # (empty face blocks are dropped)
            out[kL], out[kR] = np.asfortranarray(np.stack(iL, axis=1)), np.asfortranarray(np.stack(iR, axis=1))
            if mixed:
                out["int%d_cl" % t], out["int%d_cr" % t] = np.array(icl, dtype=np.int32), np.array(icr, dtype=np.int32)
        if bL:
            out[kB], out[kI] = np.asfortranarray(np.stack(bL, axis=1)), np.array(bid, dtype=np.int32)
            if mixed:
                out["bdy%d_cl" % t] = np.array(bcl, dtype=np.int32)
    return dealt


def cut(d, keep, bc_from=None, ids=None):
    """the elements `keep` (any list without repeats, in that order) of a single-class fixture as a fixture of its own"""
    sz = [int(v) for v in d["sizes"]]
    ne, nfp, cls = sz[0], sz[2], sz[6]
    keep = np.asarray(keep, dtype=np.int64)
    assert len(set(keep.tolist())) == len(keep) and keep.min() >= 0 and keep.max() < ne
    whole = len(keep) == ne
    out = {}
    for k, v in d.items():
        if k.startswith(STALE) or (k.startswith("u_step") and not whole):
            continue
        ax = _axis(k)
        out[k] = v if ax is None else _take(v, keep, ax)
    out["sizes"] = np.array([len(keep)] + sz[1:], dtype=np.int32)
    new = np.full(ne, -1, dtype=np.int64)
    new[keep] = np.arange(len(keep))
    first = _merge_bcs(d, out, bc_from)
    _cut_faces(d, out, {cls: new}, {cls: nfp}, [cls], ids, first)
    return out


def cut_mixed(d, keep, bc_from=None, ids=None):
    """the same per class of a mixed fixture; keep: {class: element list}"""
    classes = [int(c) for c in d["classes"]]
    out, new, nfp = {}, {}, {}
    for c in classes:
        sz = [int(v) for v in d["c%d_sizes" % c]]
        kc = np.asarray(keep[c], dtype=np.int64)
        assert len(set(kc.tolist())) == len(kc) and kc.min() >= 0 and kc.max() < sz[0]
        new[c] = np.full(sz[0], -1, dtype=np.int64)
        new[c][kc] = np.arange(len(kc))
        nfp[c] = sz[2]
    for k, v in d.items():
        c = int(k[1]) if k[0] == "c" and k[1:2].isdigit() and k[2:3] == "_" else None
        if c is None:
            if not k.startswith(STALE):
                out[k] = v
            continue
        name = k[3:]
        whole = len(keep[c]) == len(new[c])
        if name.startswith(STALE) or (name.startswith("u_step") and not whole):
            continue
        ax = _axis(name)
        out[k] = v if ax is None else _take(v, np.asarray(keep[c], dtype=np.int64), ax)
    for c in classes:
        out["c%d_sizes" % c] = np.array([len(keep[c])] + [int(v) for v in d["c%d_sizes" % c]][1:], dtype=np.int32)
    first = _merge_bcs(d, out, bc_from)
    _cut_faces(d, out, new, nfp, classes, ids, first)
    return out


def tile(d, k):
    """k disjoint copies of a single-class fixture; copy i carries the state scaled by 1 + 0.02 (i % 7) (the conserved variables
    scaled together: the velocity field stays, density and pressure scale -- as the bench-size tests do)"""
    sz = [int(v) for v in d["sizes"]]
    ne, nfp = sz[0], sz[2]
    out = {}
    for key, v in d.items():
        if key.startswith(STALE) or key.startswith("u_step"):
            continue
        ax = _axis(key)
        out[key] = v if ax is None else np.asfortranarray(np.concatenate([v] * k, axis=ax))
    u = out["u_init"].copy(order="F")
    u *= np.repeat(1.0 + 0.02 * (np.arange(k) % 7), ne)[None, :, None]
    out["u_init"] = u
    out["sizes"] = np.array([ne * k] + sz[1:], dtype=np.int32)
    for t in range(3):
        for key in ("int%d_L" % t, "int%d_R" % t, "bdy%d_L" % t):
            if key in d:
                out[key] = np.asfortranarray(np.concatenate([np.asarray(d[key]) + i * ne * nfp for i in range(k)], axis=1).astype(np.int32))
        if "bdy%d_id" % t in d:
            out["bdy%d_id" % t] = np.tile(np.ravel(d["bdy%d_id" % t]), k).astype(np.int32)
    return out


def face_census(d):
    """how many registered faces own every flux point of a single-class block: (n_fpts * n_eles,) counts"""
    sz = [int(v) for v in d["sizes"]]
    count = np.zeros(sz[0] * sz[2], dtype=np.int64)
    for t in range(3):
        for key in ("int%d_L" % t, "int%d_R" % t, "bdy%d_L" % t):
            if key in d:
                np.add.at(count, np.ravel(d[key]), 1)
    return count


# ---- the blocks the GPU tests run (tests/test_gpu_general_batches.py), and their references ---------------------------------------
CLASSES = {"tet_p1": ("tet_p1_n2_deformed", 1), "tet_p2": ("tet_p2_n2_deformed", 1), "tet_p3": ("tet_p3_n2_deformed", 1),
           "tet_p4": ("tet_p4_n2_deformed", 1), "pri_p1": ("pri_p1_n2_deformed", 3), "pri_p2": ("pri_p2_n2_deformed", 3),
           "pri_p3": ("pri_p3_n2_deformed", 3)}  # class -> (fixture, tiles)
COUNTS = (1, 15, 17, 33)
FEATURES = ["tet_p2_les_wale", "pri_p2_les_wale", "tet_p3_les_wsm", "tet_p3_les_sim", "tet_p3_les_svv", "tet_p2_overint",
            "pri_p2_overint", "tet_p3_shock", "pri_p2_shock", "tet_p2_cfl_local", "tet_p2_roem_sutherland", "tet_p2_rusanov_ldg",
            "tet_p2_inviscid"]
N_STEPS = 2
# the boundary records are scaled for the Taylor-Green state of their fixture (p = 71.4); the isentropic vortex of the inviscid
# fixture has p = 1, where the in- and outflow and far-field kinds drive the pressure below zero within a step or return NaN:
# and the viscous walls belong to viscous runs alone (the library refuses them as the reference does): its cut faces are slip walls
KINDS = {"tet_p2_inviscid": (2,)}
MIXED_KEEP = {2: 23, 3: 15}


def _seed(name, n):
    return sum(ord(ch) for ch in name) * 64 + n


@functools.lru_cache(maxsize=None)
def block(name, n, tiles=1):
    """n elements of fixture `name` (tiled first where tiles > 1), picked and ordered by a seeded permutation; the cut faces carry
    the six boundary kinds of hex_p2_bdy_walls in a seeded order (KINDS: the kinds a fixture's state can take)"""
    d = load(name)
    if tiles > 1:
        d = tile(d, tiles)
    rng = np.random.default_rng(_seed(name, n))
    keep = rng.permutation(int(d["sizes"][0]))[:n]
    ids = rng.permutation(6)
    return cut(d, keep, load(BC_FROM), [i for i in ids if i in KINDS.get(name, ids)])


def class_block(cls, n):
    name, tiles = CLASSES[cls]
    return block(name, n, tiles)


def feature_block(name, n=17):
    return block(name, n, 2 if int(load(name)["sizes"][0]) < 2 * n else 1)


@functools.lru_cache(maxsize=None)
def mixed_block():
    d = load("mixed_p3_channel")
    rng = np.random.default_rng(2323)
    keep = {c: rng.permutation(int(d["c%d_sizes" % c][0]))[:MIXED_KEEP[c]] for c in (2, 3)}
    return cut_mixed(d, keep, load(BC_FROM), rng.permutation(6))


def permuted(name, seed=5):
    """the whole fixture in a seeded random element order -> (block, keep); mixed fixtures: every class permuted, keep per class"""
    d = load(name)
    rng = np.random.default_rng(seed)
    if "classes" in d:
        keep = {int(c): rng.permutation(int(d["c%d_sizes" % c][0])) for c in d["classes"]}
        return cut_mixed(d, keep), keep
    keep = rng.permutation(int(d["sizes"][0]))
    return cut(d, keep), keep


def primitive_minima(u, gamma):
    """(min rho, min p) of a state (n_upts, n_eles, 5)"""
    rho = u[:, :, 0]
    p = (gamma - 1.0) * (u[:, :, 4] - 0.5 * (u[:, :, 1] ** 2 + u[:, :, 2] ** 2 + u[:, :, 3] ** 2) / rho)
    return float(rho.min()), float(p.min())


def oracle_steps(d, n_steps=N_STEPS, dt_map=None):
    """n_steps time steps of the oracle on a single-class block, in the reference's call order (tests/test_oracle_vs_golden.py:
    CFL time step, calc_sgs_terms at the first stage, CalcResidual with boundary faces, AdvanceSolution, shock capturing)
    -> per step a dict of copies: u, div (of the last stage), sensor (shock capturing) and bad (the worst NaN report, -1: none).
    dt_map (dt_type 2): what a deliberately WRONG run does to the local time steps before it uses them"""
    import oracle_py as O
    o = O.load()
    c = O.Case(d)
    e = c.c_eles()
    f, nfb = c.c_faces()
    bd, nbd = c.c_bdy()
    sh = c.c_shock() if c.shock_cap else None
    nstage = int(d["sizes"][7])
    dt_type = int(np.ravel(d["dt_type"])[0])
    out = []
    for st in range(n_steps):
        bad = -1
        if dt_type != 0:
            CFL, order, h = float(np.ravel(d["CFL"])[0]), int(d["sizes"][5]), np.ravel(d["h_ref"])
            dtl = np.array([o.orc_calc_dt_local(C.byref(e), C.byref(c.params), i, h[i], CFL, order) for i in range(c.n_eles)])
            c.params.dt = dtl.min()
            if dt_type == 2:
                dtl = dtl if dt_map is None else np.ascontiguousarray(dt_map(dtl))
                c._dtl = dtl
                e.dt_local = dtl.ctypes.data_as(O.dp)
        for rk in range(nstage):
            if rk == 0 and c.les and c.les["sgs_model"] >= 2:
                bad = max(bad, o.orc_calc_sgs_terms(C.byref(e)))
            bad = max(bad, o.orc_CalcResidual_bdy(C.byref(e), f, nfb, bd, nbd, C.byref(c.params)))
            o.orc_AdvanceSolution(C.byref(e), C.byref(c.params), rk)
            if sh is not None:
                o.orc_shock_capture(C.byref(e), C.byref(sh))
        out.append(dict(u=c.arr["u0"].copy(order="F"), div=c.arr["div_tconf_upts"].copy(order="F"), bad=bad,
                        sensor=c.arr["sensor"].copy() if sh is not None else None))
    return out


def mixed_oracle_steps(d, n_steps=N_STEPS):
    """the same on a mixed block -> per step {class: dict(u, div)} and "bad\""""
    m = MU.MixedOracle(d)
    nstage = int(d["c%d_sizes" % m.classes[0]][7])
    out = []
    for st in range(n_steps):
        bad = -1
        for rk in range(nstage):
            bad = max(bad, m.CalcResidual())
            m.AdvanceSolution(rk)
        step = {c: dict(u=m.arr(c, "u0").copy(order="F"), div=m.arr(c, "div_tconf_upts").copy(order="F")) for c in m.classes}
        step["bad"] = bad
        out.append(step)
    return out


_references = {}


def reference(key, d):
    """oracle_steps / mixed_oracle_steps of block d, computed once per key and shared (read-only) among the tests"""
    if key not in _references:
        _references[key] = mixed_oracle_steps(d) if "classes" in d else oracle_steps(d)
    return _references[key]


def element_moves(before, after):
    """per element: max |after - before| relative to max |before| of the block"""
    return np.abs(after - before).max(axis=(0, 2)) / np.abs(before).max()
