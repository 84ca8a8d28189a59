"""Triangles: the mesh writer of the fixtures under tests/golden/tris, the oracle in lockstep with a fixture, and the blocks the
GPU tests cut out of them -- TEST INFRASTRUCTURE.

The mesh is a periodic box of nx x ny squares, each cut along the same diagonal (lower left to upper right) into the triangles
A = (v00, v10, v11) and B = (v00, v11, v01), both counter-clockwise; element 2 (i + nx j) is A of square (i, j), the next one B.
Local face f of a triangle joins its nodes f and f + 1 (mod 3); Gambit's face number is f + 1.  With orient_seed every element's
node list is written rotated by a seeded 0, 1 or 2 places, so that faces meet in every combination of local faces.

A table entry of a fixture is fpt + n_fpts * ele; the flux points of local face f are f (order + 1) ... (f + 1)(order + 1) - 1."""
import ctypes as C
import functools
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tris")
SIDES = ("y-", "x+", "y+", "x-")
# the bars of tests/test_oracle_vs_golden.py
RTOL, RTOL_BDY, RTOL_RES = 1e-13, 1e-12, 1e-12


def names():
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz")) if os.path.isdir(GOLDEN) else []


@functools.lru_cache(maxsize=None)
def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def load(name):
    return dict(_load(name))


def relerr(a, b):
    s = np.abs(b).max()
    return float(np.abs(a - b).max() / (s if s > 0 else 1.0))


def rotations(ne, seed):
    """places every element's node list is rotated by: the first three elements carry 0, 1, 2 in a seeded order"""
    if seed is None:
        return np.zeros(ne, dtype=int)
    rng = np.random.RandomState(seed)
    rot = rng.randint(3, size=ne)
    first = rng.permutation(3)[:ne]
    rot[:first.size] = first
    return rot


def write_neu_tris(path, n, xv, length=2.0 * math.pi, bcname="Cyclic", bcs=None, orient_seed=None):
    """xv: the (nx + 1)(ny + 1) vertices of the box, x fastest (gen_neu_mesh.box_vertices); bcs: {side: group} for the sides that
    are not periodic, as gen_neu_mesh.write_neu takes it (or a list of groups, dealt to the side's cells in turn)"""
    nx, ny = (n, n) if isinstance(n, int) else (n[0], n[1])
    ne = 2 * nx * ny
    rot = rotations(ne, orient_seed)

    def vid(i, j):
        return 1 + i + (nx + 1) * j

    def group(side, idx):
        g = (bcs or {}).get(side, bcname)
        return g if isinstance(g, str) else g[idx % len(g)]  # (a list: the side's cells take its groups in turn)

    groups = []
    for side in SIDES:
        for idx in range(max(nx, ny)):
            if group(side, idx) not in groups:
                groups.append(group(side, idx))
    cells, bfaces = [], []
    for j in range(ny):
        for i in range(nx):
            v00, v10, v01, v11 = vid(i, j), vid(i + 1, j), vid(i, j + 1), vid(i + 1, j + 1)
            for half, nodes, sides in ((0, [v00, v10, v11], {0: "y-" if j == 0 else None, 1: "x+" if i == nx - 1 else None}),
                                       (1, [v00, v11, v01], {1: "y+" if j == ny - 1 else None, 2: "x-" if i == 0 else None})):
                e = 2 * (i + nx * j) + half
                r = int(rot[e])
                cells.append(nodes[r:] + nodes[:r])
                for f, side in sides.items():
                    if side is not None:
                        bfaces.append((e + 1, (f - r) % 3 + 1, group(side, j if side[0] == "x" else i)))
    with open(path, "w") as f:
        f.write("        CONTROL INFO 2.3.16\n** GAMBIT NEUTRAL FILE\nperiodic_box\n")
        f.write("PROGRAM:                Gambit     VERSION:  2.3.16\n\n")
        f.write("     NUMNP     NELEM     NGRPS    NBSETS     NDFCD     NDFVL\n")
        f.write("%10d%10d%10d%10d%10d%10d\n" % (xv.shape[0], ne, 1, len(groups), 2, 2))
        f.write("ENDOFSECTION\n   NODAL COORDINATES 2.3.16\n")
        for i in range(xv.shape[0]):
            f.write("%10d" % (i + 1) + "".join(" %.17e" % c for c in xv[i]) + "\n")
        f.write("ENDOFSECTION\n      ELEMENTS/CELLS 2.3.16\n")
        for e, nodes in enumerate(cells):
            f.write("%8d %2d %2d " % (e + 1, 3, 3) + "".join("%8d" % v for v in nodes) + "\n")
        f.write("ENDOFSECTION\n       ELEMENT GROUP 2.3.16\n")
        f.write("GROUP: %10d ELEMENTS: %10d MATERIAL: %10d NFLAGS: %10d\n" % (1, ne, 2, 1))
        f.write("                           fluid\n       0\n")
        ids = list(range(1, ne + 1))
        for s in range(0, ne, 10):
            f.write("".join("%8d" % v for v in ids[s:s + 10]) + "\n")
        f.write("ENDOFSECTION\n")
        for g in groups:
            mine = [b for b in bfaces if b[2] == g]
            f.write(" BOUNDARY CONDITIONS 2.3.16\n")
            f.write("%32s%8d%8d%8d%8d\n" % (g, 1, len(mine), 0, 6))
            for (el, fc, _) in mine:
                f.write("%10d%5d%5d\n" % (el, 3, fc))
            f.write("ENDOFSECTION\n")


def face_pair_census(d):
    """(3, 3) counts: interior faces whose left side is local face i and whose right side is local face j"""
    nfp, order = int(d["sizes"][2]), int(d["sizes"][5])
    out = np.zeros((3, 3), dtype=int)
    for t in range(3):
        if "int%d_L" % t in d:
            L, R = np.asarray(d["int%d_L" % t]), np.asarray(d["int%d_R" % t])
            for c in range(L.shape[1]):
                out[(L[0, c] % nfp) // (order + 1), (R[0, c] % nfp) // (order + 1)] += 1
    return out


def stored_steps(d):
    return sorted({int(k.split("_")[1][4:]) for k in d if k.startswith("u_step")})


def lockstep(d):
    """the oracle in lockstep with the dumped inputs of fixture d, as tests/test_oracle_vs_golden.py::test_stage_states (and, where
    the fixture holds them, ::test_every_intermediate / ::test_boundary_intermediates) -> {what: (error, bar)}; nothing asserted"""
    import oracle_py as O
    o = O.load()
    out = {}

    def note(key, err, bar):
        out[key] = (float(err), bar)

    c = O.Case(d)
    e = c.c_eles()
    f, nfb = c.c_faces()
    bd, nbd = c.c_bdy()
    nstage = int(d["sizes"][7])
    dt_type = int(np.ravel(d["dt_type"])[0])
    for st in range(max(stored_steps(d)) + 1):
        if dt_type != 0:
            CFL, order, h = float(np.ravel(d["CFL"])[0]), int(d["sizes"][5]), np.ravel(d["h_ref"])
            dtl = np.array([o.orc_calc_dt_local(C.byref(e), C.byref(c.params), i, h[i], CFL, order) for i in range(c.n_eles)])
            if "dt_step%d" % st in d:
                note("dt_step%d" % st, abs(dtl.min() - float(np.ravel(d["dt_step%d" % st])[0])) / dtl.min(), RTOL)
            c.params.dt = dtl.min()
            if dt_type == 2:
                note("dt_local_step%d" % st, relerr(dtl, np.ravel(d["dt_local_step%d" % st])), RTOL)
                c._dtl = dtl
                e.dt_local = dtl.ctypes.data_as(O.dp)
        for rk in range(nstage):
            bad = o.orc_CalcResidual_bdy(C.byref(e), f, nfb, bd, nbd, C.byref(c.params))
            note("nan_step%d_stage%d" % (st, rk), 0.0 if bad == -1 else 1.0, 0.5)
            if st == 0 and rk == 0:
                note("s0_div_tconf_upts", relerr(c.arr["div_tconf_upts"], d["s0_div_tconf_upts"]), RTOL_BDY if nbd else RTOL)
                if "s0_res_sums" in d:
                    for fld in range(c.n_fields):
                        for nt in (1, 2):
                            want = d["s0_res_sums"][fld, nt - 1]
                            note("s0_res_sums_%d_%d" % (fld, nt), abs(o.orc_compute_res_upts(C.byref(e), nt, fld) - want) / abs(want), RTOL_RES)
            o.orc_AdvanceSolution(C.byref(e), C.byref(c.params), rk)
            key = "u_step%d_stage%d" % (st, rk)
            if key in d:
                note(key, relerr(c.arr["u0"], d[key]), RTOL_BDY if nbd else RTOL)
    if "s0_grad_disu_upts" in d and "s0_tdisf_upts" in d:
        intermediates(d, note)
    return out


def intermediates(d, note):
    """every intermediate of the first residual (a level-2 fixture with all of them)"""
    import oracle_py as O
    o = O.load()
    c = O.Case(d)
    e = c.c_eles()
    f, nfb = c.c_faces()
    bd, nbd = c.c_bdy()
    P, E, a = C.byref(c.params), C.byref(e), c.arr
    bar = RTOL_BDY if nbd else RTOL

    def both_inv():
        for b in range(nfb):
            o.orc_int_calculate_common_invFlux(C.byref(f[b]), E, P)
        for b in range(nbd):
            o.orc_bdy_evaluate_boundaryConditions_invFlux(C.byref(bd[b]), E, P)

    o.orc_extrapolate_solution(E)
    note("s0_disu_fpts", relerr(a["disu_fpts"], d["s0_disu_fpts"]), bar)
    o.orc_calculate_gradient(E)
    note("s0_grad_disu_upts_ref", relerr(a["grad_disu_upts"], d["s0_grad_disu_upts_ref"]), bar)
    o.orc_evaluate_invFlux(E, P)
    note("s0_tdisf_upts_inv", relerr(a["tdisf_upts"], d["s0_tdisf_upts_inv"]), bar)
    both_inv()
    note("s0_norm_tconf_fpts_inv", relerr(a["norm_tconf_fpts"], d["s0_norm_tconf_fpts_inv"]), bar)
    note("s0_delta_disu_fpts", relerr(a["delta_disu_fpts"], d["s0_delta_disu_fpts"]), bar)
    o.orc_correct_gradient(E)
    note("s0_grad_disu_upts", relerr(a["grad_disu_upts"], d["s0_grad_disu_upts"]), bar)
    note("s0_grad_disu_fpts", relerr(a["grad_disu_fpts"], d["s0_grad_disu_fpts"]), bar)
    o.orc_evaluate_viscFlux(E, P)
    note("s0_tdisf_upts", relerr(a["tdisf_upts"], d["s0_tdisf_upts"]), bar)
    o.orc_extrapolate_totalFlux(E)
    note("s0_norm_tdisf_fpts", relerr(a["norm_tdisf_fpts"], d["s0_norm_tdisf_fpts"]), bar)
    o.orc_calculate_divergence(E)
    note("s0_div_tconf_upts_disc", relerr(a["div_tconf_upts"], d["s0_div_tconf_upts_disc"]), bar)
    for b in range(nfb):
        o.orc_int_calculate_common_viscFlux(C.byref(f[b]), E, P)
    for b in range(nbd):
        o.orc_bdy_evaluate_boundaryConditions_viscFlux(C.byref(bd[b]), E, P)
    note("s0_norm_tconf_fpts", relerr(a["norm_tconf_fpts"], d["s0_norm_tconf_fpts"]), bar)
    o.orc_calculate_corrected_divergence(E)
    note("s0_div_tconf_upts(2)", relerr(a["div_tconf_upts"], d["s0_div_tconf_upts"]), bar)


def failures(errs):
    return {k: v for k, v in errs.items() if not v[0] < v[1]}


# ---- the blocks the GPU tests run: any element count, cut faces become boundary faces ------------------------------------------
CUT_FROM, BC_FROM = "tri_p3_n4_deformed", "tri_p3_bdy"
N_STEPS = 2
GROUP = {1: 64, 2: 64, 3: 32, 4: 32, 5: 16}  # elements per group by order: SIMPLEX2D_SIZES of csrc/simplex2d.hpp
BY_ORDER = {1: "tri_p1_n4_deformed", 2: "tri_p2_n3_deformed", 3: "tri_p3_n4_deformed", 4: "tri_p4_n2_deformed", 5: "tri_p5_n2_deformed"}
# the boundary records are scaled for the Taylor-Green state of their fixture; on the isentropic vortex of the inviscid fixture the
# oracle itself returns NaN with the characteristic outflow (type 3) and the far field (type 10) among the cut faces, and the
# library refuses the adiabatic wall (type 9) without viscous terms, as the reference does (src/input.cpp:427): its cut faces
# are isothermal walls (type 8) alone, whose inviscid state is all an inviscid run uses (tests/test_tris_oracle.py runs the
# oracle on every block)
KINDS = {"tri_p2_inviscid": (8,)}


def group_of(name):
    """elements per group of the fused stage at the fixture's order"""
    return GROUP[int(_load(name)["sizes"][5])]


def edge_counts(name):
    """G - 1, G, G + 1, 2 G + 1"""
    g = group_of(name)
    return [g - 1, g, g + 1, 2 * g + 1]


@functools.lru_cache(maxsize=None)
def block(n, name=CUT_FROM, kinds=None):
    """n elements of the fixture (tiled first where it has fewer than 2 n), picked and ordered by a seeded permutation; the cut
    faces carry the boundary records of tri_p3_bdy without a pressure ramp (isothermal and adiabatic wall, far field, characteristic
    outflow) in a seeded order; kinds: only the records of these types (bc_flags row 0; None: KINDS of the fixture, or all)"""
    import general_util as G
    d = load(name)
    ne = int(d["sizes"][0])
    if ne < 2 * n:
        d = G.tile(d, (2 * n + ne - 1) // ne)
    rng = np.random.default_rng(7000 + n)
    keep = rng.permutation(int(d["sizes"][0]))[:n]
    bc = load(BC_FROM)
    fl = np.asarray(bc["bc_flags"]).reshape(3, -1, order="F")
    kinds = KINDS.get(name) if kinds is None else kinds
    # (not the ramping inlet: the step loops advance its counter after every step, general_util.oracle_steps does not)
    ids = rng.permutation([i for i in range(fl.shape[1]) if fl[1, i] == 0])
    return G.cut(d, keep, bc, [i for i in ids if kinds is None or fl[0, i] in kinds])


def order_blocks():
    """(fixture, n): blocks of G - 1, G, G + 1 and 2 G + 1 elements at every instantiated order"""
    return [(BY_ORDER[p], n) for p in sorted(BY_ORDER) for n in edge_counts(BY_ORDER[p])]


# the run-wide switches past group 0 (P2: G = 64); dt_type 2 also with a second group of ONE element
SWITCH_BLOCKS = [("tri_p2_roem_sutherland", 129), ("tri_p2_rusanov_ldg", 129), ("tri_p2_inviscid", 129), ("tri_p2_cfl_local", 129),
                 ("tri_p2_cfl_local", 65)]

_references = {}


def block_reference(n, name=CUT_FROM):
    """the oracle's N_STEPS steps on block(n, name), computed once and shared (read-only)"""
    return reference(("block", n) if name == CUT_FROM else ("block", n, name), block(n, name))


def offset_differences(u, g):
    """per element a < n - g: max |u[a] - u[a + g]| relative to max |u| (a state that takes element a + g for element a shows)"""
    return np.abs(u[:, :-g] - u[:, g:]).max(axis=(0, 2)) / np.abs(u).max()


def reference(key, d, n_steps=N_STEPS):
    import general_util as G
    if key not in _references:
        _references[key] = G.oracle_steps(d, n_steps)
    return _references[key]
