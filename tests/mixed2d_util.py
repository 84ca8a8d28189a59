"""Mixed quadrilateral / triangle meshes in two dimensions: the mesh writer of the fixtures under tests/golden/mixed2d, the oracle in
lockstep with a fixture, tiling, and the blocks the GPU tests cut out of them -- TEST INFRASTRUCTURE.

The mesh is a periodic box of nx x ny squares.  Square (i, j) stays a quadrilateral (Gambit type 2, nodes v00 v10 v11 v01, counter-
clockwise) where the layout says so; every other square is cut along tri_util's diagonal into the triangles A = (v00, v10, v11) and
B = (v00, v11, v01) (Gambit type 3).  Elements are numbered square by square, i fastest.  Local face f of an element joins its nodes
f and f + 1; Gambit's face number is f + 1, and a boundary record carries the element's own type and face number.

A fixture has the layout of tests/mixed_util.py: `classes` (0 triangles, 1 quadrilaterals), every class's arrays under "c<class>_",
and per face block the class of either side of every face.  A table entry is fpt + n_fpts * ele within the side's class."""
import functools
import os

import numpy as np

import general_util as G
import mixed_util as MU
import tri_util as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixed2d")
TRI, QUAD = 0, 1
# elements per group of the fused stage by order: SIMPLEX2D_SIZES and QUAD2D_SIZES of csrc/simplex2d.hpp
GROUP = {TRI: {1: 64, 2: 64, 3: 32, 4: 32}, QUAD: {1: 64, 2: 32, 3: 16, 4: 8}}
# {solution points, flux points} and the fused stage's size class
POINTS = {TRI: {1: (3, 6), 2: (6, 9), 3: (10, 12), 4: (15, 15)}, QUAD: {1: (4, 8), 2: (9, 12), 3: (16, 16), 4: (25, 20)}}
SIZE_CLASS = {TRI: lambda p: p - 1, QUAD: lambda p: 5 + p - 1}
LDS_BUDGET = 80 * 1024
BY_ORDER = {1: "mx_p1_n4", 2: "mx_p2_n4", 3: "mx_p3_n4", 4: "mx_p4_n4"}
PHYSICS_BASE = "mx_p2_n4"
PHYSICS_ROWS = ("mx_p2_inviscid", "mx_p2_roem_sutherland", "mx_p2_rusanov_ldg")
N_STEPS = 2


# ---- layouts: which squares stay quadrilaterals ----------------------------------------------------------------------------------
def layout_checker(i, j, nx, ny):
    """the left half, and a checkerboard in the right half: all four class pairs among the interior faces"""
    return i < nx // 2 or (i + j) % 2 == 0


def layout_half(i, j, nx, ny):
    return i < nx // 2


def layout_walls(i, j, nx, ny):
    """quadrilateral rows on both walls in y, triangles between"""
    return j == 0 or j == ny - 1


LAYOUTS = {"checker": layout_checker, "half": layout_half, "walls": layout_walls}


def write_neu_mixed2d(path, n, xv, layout, bcname="Cyclic", bcs=None):
    """xv: the (nx + 1)(ny + 1) vertices of the box, x fastest (gen_neu_mesh.box_vertices); layout: a name of LAYOUTS; bcs: {side:
    group} for the sides that are not periodic (or a list of groups, dealt to the side's cells in turn), as tri_util.write_neu_tris
    -> [(class, element within the class)] per mesh element"""
    nx, ny = (n, n) if isinstance(n, int) else (n[0], n[1])
    is_quad = LAYOUTS[layout]

    def vid(i, j):
        return 1 + i + (nx + 1) * j

    def group(side, idx):
        g = (bcs or {}).get(side, bcname)
        return g if isinstance(g, str) else g[idx % len(g)]

    groups = []
    for side in T.SIDES:
        for idx in range(max(nx, ny)):
            if group(side, idx) not in groups:
                groups.append(group(side, idx))
    cells, bfaces, where, count = [], [], [], {TRI: 0, QUAD: 0}
    for j in range(ny):
        for i in range(nx):
            v00, v10, v01, v11 = vid(i, j), vid(i + 1, j), vid(i, j + 1), vid(i + 1, j + 1)
            lo, hi, le, ri = ("y-" if j == 0 else None), ("y+" if j == ny - 1 else None), ("x-" if i == 0 else None), ("x+" if i == nx - 1 else None)
            if is_quad(i, j, nx, ny):
                parts = [(2, [v00, v10, v11, v01], {0: lo, 1: ri, 2: hi, 3: le})]
            else:
                parts = [(3, [v00, v10, v11], {0: lo, 1: ri}), (3, [v00, v11, v01], {1: hi, 2: le})]
            for ty, nodes, sides in parts:
                cells.append((ty, nodes))
                cls = QUAD if ty == 2 else TRI
                where.append((cls, count[cls]))
                count[cls] += 1
                for f, side in sides.items():
                    if side is not None:
                        bfaces.append((len(cells), ty, f + 1, group(side, j if side[0] == "x" else i)))
    ne = len(cells)
    with open(path, "w") as f:
        f.write("        CONTROL INFO 2.3.16\n** GAMBIT NEUTRAL FILE\nperiodic_box\n")
        f.write("PROGRAM:                Gambit     VERSION:  2.3.16\n\n")
        f.write("     NUMNP     NELEM     NGRPS    NBSETS     NDFCD     NDFVL\n")
        f.write("%10d%10d%10d%10d%10d%10d\n" % (xv.shape[0], ne, 1, len(groups), 2, 2))
        f.write("ENDOFSECTION\n   NODAL COORDINATES 2.3.16\n")
        for i in range(xv.shape[0]):
            f.write("%10d" % (i + 1) + "".join(" %.17e" % c for c in xv[i]) + "\n")
        f.write("ENDOFSECTION\n      ELEMENTS/CELLS 2.3.16\n")
        for e, (ty, nodes) in enumerate(cells):
            f.write("%8d %2d %2d " % (e + 1, ty, len(nodes)) + "".join("%8d" % v for v in nodes) + "\n")
        f.write("ENDOFSECTION\n       ELEMENT GROUP 2.3.16\n")
        f.write("GROUP: %10d ELEMENTS: %10d MATERIAL: %10d NFLAGS: %10d\n" % (1, ne, 2, 1))
        f.write("                           fluid\n       0\n")
        ids = list(range(1, ne + 1))
        for s in range(0, ne, 10):
            f.write("".join("%8d" % v for v in ids[s:s + 10]) + "\n")
        f.write("ENDOFSECTION\n")
        for g in groups:
            mine = [b for b in bfaces if b[3] == g]
            f.write(" BOUNDARY CONDITIONS 2.3.16\n")
            f.write("%32s%8d%8d%8d%8d\n" % (g, 1, len(mine), 0, 6))
            for (el, ty, fc, _) in mine:
                f.write("%10d%5d%5d\n" % (el, ty, fc))
            f.write("ENDOFSECTION\n")
    return where


# ---- fixtures --------------------------------------------------------------------------------------------------------------------
def names():
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz")) if os.path.isdir(GOLDEN) else []


@functools.lru_cache(maxsize=None)
def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def load(name):
    return dict(_load(name))


relerr = T.relerr


def classes_of(d):
    return [int(c) for c in d["classes"]]


def sizes(d, c):
    return [int(v) for v in d["c%d_sizes" % c]]


def pair_census(d):
    """{(left class, right class): interior faces}"""
    out = {}
    for t in range(3):
        if "int%d_cl" % t in d:
            for a, b in zip(np.ravel(d["int%d_cl" % t]), np.ravel(d["int%d_cr" % t])):
                out[(int(a), int(b))] = out.get((int(a), int(b)), 0) + 1
    return out


def stored_steps(d):
    c = classes_of(d)[0]
    return sorted({int(k.split("_")[2][4:]) for k in d if k.startswith("c%d_u_step" % c)})


# hook of MixedOracle.CalcResidual -> (fixture key, oracle array)
INTERMEDIATES = {
    "disu_fpts": ("s0_disu_fpts", "disu_fpts"), "grad_disu_upts_ref": ("s0_grad_disu_upts_ref", "grad_disu_upts"),
    "tdisf_upts_inv": ("s0_tdisf_upts_inv", "tdisf_upts"), "norm_tconf_fpts_inv": ("s0_norm_tconf_fpts_inv", "norm_tconf_fpts"),
    "grad_disu_fpts": ("s0_grad_disu_fpts", "grad_disu_fpts"), "tdisf_upts": ("s0_tdisf_upts", "tdisf_upts"),
    "norm_tdisf_fpts": ("s0_norm_tdisf_fpts", "norm_tdisf_fpts"), "div_tconf_upts_disc": ("s0_div_tconf_upts_disc", "div_tconf_upts"),
    "norm_tconf_fpts": ("s0_norm_tconf_fpts", "norm_tconf_fpts"), "div_tconf_upts": ("s0_div_tconf_upts", "div_tconf_upts"),
}


def lockstep(d, copy_elements=None):
    """the oracle in lockstep with the dumped states of fixture d (every stage state of every class; a level-2 fixture: every
    intermediate of the first residual too) -> {what: (error, bar)}, the bars tri_util's; nothing asserted.  copy_elements: {class:
    n}: the oracle runs a LARGER block (tile_mixed) and its first n elements of the class are compared"""
    m = MU.MixedOracle(d)
    has_bdy = len(m.bdy) > 0
    bar = T.RTOL_BDY if has_bdy else T.RTOL
    out = {}
    first = [True]

    def part(c, a, axis):
        return a if copy_elements is None else np.take(a, np.arange(copy_elements[c]), axis=axis)

    def hook(what):
        key, arr = INTERMEDIATES[what]
        for c in m.classes:
            k = "c%d_%s" % (c, key)
            if first[0] and k in d:
                a = m.arr(c, arr)
                out[k] = (T.relerr(part(c, a, 1), part(c, d[k], 1)), bar)

    nstage = sizes(d, m.classes[0])[7]
    for st in range(max(stored_steps(d)) + 1):
        for rk in range(nstage):
            bad = m.CalcResidual(hook)
            first[0] = False
            out["nan_step%d_stage%d" % (st, rk)] = (0.0 if bad == -1 else 1.0, 0.5)
            m.AdvanceSolution(rk)
            for c in m.classes:
                k = "c%d_u_step%d_stage%d" % (c, st, rk)
                if k in d:
                    out[k] = (T.relerr(part(c, m.arr(c, "u0"), 1), part(c, d[k], 1)), bar)
    return out


def tile_mixed(d, k):
    """k disjoint copies of a mixed fixture: every class's per-element arrays repeated, the face tables shifted per class, copy i's
    state scaled by 1 + 0.02 (i % 7) as general_util.tile scales it (copy 0 carries the fixture's)"""
    cls = classes_of(d)
    ne = {c: sizes(d, c)[0] for c in cls}
    nfp = {c: sizes(d, c)[2] for c in cls}
    out = {}
    for key, v in d.items():
        c = int(key[1]) if key[0] == "c" and key[1:2].isdigit() and key[2:3] == "_" else None
        if c is None:
            if not key.startswith(G.STALE):
                out[key] = v
            continue
        name = key[3:]
        if name.startswith(G.STALE) or name.startswith("u_step"):
            continue
        ax = G._axis(name)
        out[key] = v if ax is None else np.asfortranarray(np.concatenate([v] * k, axis=ax))
    for c in cls:
        u = out["c%d_u_init" % c].copy(order="F")
        u *= np.repeat(1.0 + 0.02 * (np.arange(k) % 7), ne[c])[None, :, None]
        out["c%d_u_init" % c] = u
        out["c%d_sizes" % c] = np.array([ne[c] * k] + sizes(d, c)[1:], dtype=np.int32)
    for t in range(3):
        for key, side in (("int%d_L" % t, "int%d_cl" % t), ("int%d_R" % t, "int%d_cr" % t), ("bdy%d_L" % t, "bdy%d_cl" % t)):
            if key in d:
                tab, cl = np.asarray(d[key]), np.ravel(d[side])
                shift = np.array([ne[int(c)] * nfp[int(c)] for c in cl], dtype=np.int64)[None, :]
                out[key] = np.asfortranarray(np.concatenate([tab + i * shift for i in range(k)], axis=1).astype(np.int32))
                out[side] = np.tile(cl, k).astype(np.int32)
        if "bdy%d_id" % t in d:
            out["bdy%d_id" % t] = np.tile(np.ravel(d["bdy%d_id" % t]), k).astype(np.int32)
    return out


# ---- the blocks the GPU tests run ------------------------------------------------------------------------------------------------
def edge_counts(order):
    """[{class: n}]: per class G - 1, G + 1 and 2 G + 1 elements of that class's own G, both classes at once"""
    g = {c: GROUP[c][order] for c in (TRI, QUAD)}
    return [{c: g[c] - 1 for c in g}, {c: g[c] + 1 for c in g}, {c: 2 * g[c] + 1 for c in g}]


def _bc_ids(rng):
    bc = T.load(T.BC_FROM)
    fl = np.asarray(bc["bc_flags"]).reshape(3, -1, order="F")
    # (not the ramping inlet: the step loops advance its counter after every step, the oracle's loop here does not)
    return bc, [int(i) for i in rng.permutation([i for i in range(fl.shape[1]) if fl[1, i] == 0])]


@functools.lru_cache(maxsize=None)
def block(order, n_tri, n_quad):
    """n_tri triangles and n_quad quadrilaterals of the order's fixture, tiled until every class has twice as many, picked and
    ordered by a seeded permutation; the cut faces carry tri_p3_bdy's records (without the pressure ramp) in a seeded order"""
    d = load(BY_ORDER[order])
    want = {TRI: n_tri, QUAD: n_quad}
    k = max((2 * want[c] + sizes(d, c)[0] - 1) // sizes(d, c)[0] for c in want)
    d = tile_mixed(d, max(k, 1))
    rng = np.random.default_rng(9100 + 1000 * order + n_tri + 7 * n_quad)
    keep = {c: rng.permutation(sizes(d, c)[0])[:want[c]] for c in (TRI, QUAD)}
    bc, ids = _bc_ids(rng)
    return G.cut_mixed(d, keep, bc, ids)


@functools.lru_cache(maxsize=None)
def quad_block(order, n):
    """n quadrilaterals alone: the quadrilateral class cut out of the tiled fixture, as a single-class fixture (the faces to the
    triangles become boundary faces; cut_mixed keeps one triangle, which single_class drops)"""
    d = load(BY_ORDER[order])
    k = max(1, (2 * n + sizes(d, QUAD)[0] - 1) // sizes(d, QUAD)[0])
    d = tile_mixed(d, k)
    rng = np.random.default_rng(9500 + 1000 * order + n)
    keep = {QUAD: rng.permutation(sizes(d, QUAD)[0])[:n], TRI: np.arange(1)}
    bc, ids = _bc_ids(rng)
    m = G.cut_mixed(d, keep, bc, ids)
    return single_class(m, QUAD, ids)


def single_class(m, c, ids):
    """class c of a mixed block as a single-class fixture: the faces inside the class stay, a face to another class becomes a
    boundary face of the side in c with the next of the record ids `ids`, faces of the other classes are dropped"""
    classes, per, faces, bdy = MU.split(m)
    out = dict(per[c])
    for t in range(3):
        for key in ("int%d_L" % t, "int%d_R" % t, "bdy%d_L" % t, "bdy%d_id" % t):
            out.pop(key, None)
    iL, iR, bL, bid = [], [], [], []
    for a, b, L, R in faces:
        if a == c and b == c:
            iL.append(L); iR.append(R)
        elif a == c or b == c:
            side = L if a == c else R
            bL.append(side)
            bid.append(np.array([ids[(len(bid) + q) % len(ids)] for q in range(side.shape[1])], dtype=np.int32))
    for a, L, idv in bdy:
        if a == c:
            bL.append(L); bid.append(np.asarray(idv, dtype=np.int32))
    if iL:
        out["int0_L"], out["int0_R"] = np.asfortranarray(np.concatenate(iL, axis=1)), np.asfortranarray(np.concatenate(iR, axis=1))
    if bL:
        out["bdy0_L"], out["bdy0_id"] = np.asfortranarray(np.concatenate(bL, axis=1)), np.concatenate(bid)
    for k in ("bc_flags", "bc_params", "bc_R_ref", "ramp_counter"):
        out[k] = m[k]
    return out


def split_triangles(d, first):
    """a single-class triangle fixture as a MIXED-layout fixture of two triangle blocks: the elements `first` (a boolean mask) form
    block "0", the others block "2" -- a label, both are triangles --; faces between them become cross faces -> (mixed dict, labels)"""
    sz = [int(v) for v in d["sizes"]]
    ne, nfp = sz[0], sz[2]
    first = np.asarray(first, dtype=bool)
    lab = np.where(first, 0, 2)
    new = np.zeros(ne, dtype=np.int64)
    new[first] = np.arange(first.sum())
    new[~first] = np.arange((~first).sum())
    out = {"classes": np.array([0, 2], dtype=np.int32)}
    for k, v in d.items():
        if k.startswith(("int", "bdy")) and k[3:4].isdigit():
            continue
        ax = G._axis(k)
        if ax is None:
            if k != "sizes":
                out[k] = v
            continue
        for c, m in ((0, first), (2, ~first)):
            out["c%d_%s" % (c, k)] = np.asfortranarray(np.compress(m, v, axis=ax))
    for c, m in ((0, first), (2, ~first)):
        out["c%d_sizes" % c] = np.array([int(m.sum())] + sz[1:], dtype=np.int32)  # (operators stay common to both blocks)
    for t in range(3):
        for key, side in (("int%d_L" % t, "int%d_cl" % t), ("int%d_R" % t, "int%d_cr" % t), ("bdy%d_L" % t, "bdy%d_cl" % t)):
            if key in d:
                tab = np.asarray(d[key])
                el = tab // nfp
                out[key] = np.asfortranarray((new[el] * nfp + tab % nfp).astype(np.int32))
                out[side] = lab[el[0]].astype(np.int32)
        if "bdy%d_id" % t in d:
            out["bdy%d_id" % t] = np.ravel(d["bdy%d_id" % t]).astype(np.int32)
    return out


_references = {}


def reference(key, d, n_steps=N_STEPS):
    """mixed_oracle_steps / oracle_steps of block d, computed once per key and shared (read-only)"""
    if key not in _references:
        _references[key] = G.mixed_oracle_steps(d, n_steps) if "classes" in d else G.oracle_steps(d, n_steps)
    return _references[key]
