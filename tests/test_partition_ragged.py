"""The partition-face path on RAGGED, graph-like partitions (ragged_partition.py): parts of unequal size with up to five
neighbours of unequal share, elements with several faces on one neighbour, parts without an element free of partition-face
points, partition faces whose left normal points in -x / -y / -z on the lower rank.  The undivided mesh's registration is cut
along seeded per-element part vectors in test code; the raw C ABI (hfx.Eles, hfx.IntInters, hfx.BdyInters, hfx.MpiInters,
hfx.stage_partitioned, hfx.run_steps_partitioned*) runs the parts.  The invariant is the project's own: the N-part result
equals the 1-rank oracle of the same mesh, which is pinned bit-exactly against the genuine reference."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import mixed_util as MU
import ragged_partition as RP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LENGTH = 6.2831853071795862
CFG = dict(order=2, amp=0.05, length=LENGTH, T_c_ic=300.0, dt=1e-4)
BOX = [4, 4, 4]
# (weights, seed) of ragged_partition.grow_parts on the 64 hexahedra; test_census_of_the_cuts states what they have to offer
CUTS = {"ragged4": ([10, 3, 2, 1], 13), "ragged6": ([8, 4, 3, 2, 2, 1], 2)}
VIRTUAL3 = ([3, 2, 1], 5)  # the three virtual parts of the cut_self rows
FREE_STREAM = dict(riemann_solve_type=0, viscous=0, ic_form=1, u_c_ic=30.0, v_c_ic=10.0, w_c_ic=5.0, p_c_ic=101325.0, rho_c_ic=1.2)


def rel(a, b):
    s = np.abs(b).max()
    return np.abs(a - b).max() / (s if s > 0 else 1.0)


def part_vector(name):
    w, seed = CUTS[name] if isinstance(name, str) else name
    return RP.grow_parts(BOX, w, seed)


# ---- cases and references: computed once, never written to -------------------------------------------------------------------

_cache = {}


def key_of(kw):
    return json.dumps(kw, sort_keys=True, default=str)


def walls_kw():
    """a box built like the fixture hex_p2_bdy_walls (all six sides boundary groups: characteristic inflow / outflow, an
    isothermal and an adiabatic wall, far field, slip wall), 4 x 4 x 4"""
    import bdy_util
    d = np.load(os.path.join(GOLDEN, "hex_p2_bdy_walls.npz"))
    meta = json.loads(bytes(d["meta_json"]).decode())
    kk = meta["keys"]
    bcs, sides = bdy_util.groups_of(meta)
    return dict(bcs=bcs, sides=sides, order=kk["order"], amp=meta["amp"], riemann_solve_type=kk["riemann_solve_type"], dt=kk["dt"],
                T_c_ic=kk["T_c_ic"], rho_c_ic=kk["rho_c_ic"], fix_vis=kk["fix_vis"])


def registration(kw):
    """(registration dict, pos_fpts) of the undivided box under the host mirror's keywords kw"""
    k = ("reg", key_of(kw))
    if k not in _cache:
        import hfx_host as H
        c = H.Case(BOX, **kw)
        _cache[k] = (c.registration(), c.array("pos_fpts"))
        c.close()
    return _cache[k]


def undivided(kw, n_steps):
    k = ("one", key_of(kw), n_steps)
    if k not in _cache:
        u, div = RP.undivided_oracle(registration(kw)[0], n_steps)
        u.setflags(write=False)
        div.setflags(write=False)
        _cache[k] = (u, div)
    return _cache[k]


def cut_of(kw, name):
    k = ("cut", key_of(kw), key_of(name))
    if k not in _cache:
        _cache[k] = RP.cut(registration(kw)[0], part_vector(name))
    return _cache[k]


def oracle_parts(kw, name, n_steps=1, spoil=None):
    parts = cut_of(kw, name)
    tables = RP.part_tables(parts)
    if spoil:
        tables = spoil(tables)
    cases = RP.oracle_lockstep(tables, n_steps)
    shape = undivided(kw, n_steps)[0].shape
    return RP.assemble(parts, [c.arr["u0"] for c in cases], shape), RP.assemble(parts, [c.arr["div_tconf_upts"] for c in cases], shape)


def check_invariance(u, div, kw, n_steps, tol_u, tol_div):
    u1, div1 = undivided(kw, n_steps)
    print("rel(u) %.3g  rel(div) %.3g  |div - div1| / max|u| %.3g" % (rel(u, u1), rel(div, div1), np.abs(div - div1).max() / np.abs(u1).max()))
    if kw.get("viscous", 1):
        assert rel(div, div1) < tol_div
    else:  # uniform free stream: the residual is rounding noise, compare it on the scale of the state
        assert np.abs(div - div1).max() < tol_u * np.abs(u1).max()
    assert rel(u, u1) < tol_u


# ---- what the cuts offer (no device, no oracle: conditions on the tables) ------------------------------------------------------

def element_lists(P, nfp):
    """(elements with a partition-face point, the others): fused_build(..., allow_unpaired = true)'s n_list_b / n_list_i"""
    b = np.unique(P.L // nfp)
    return b, np.setdiff1d(np.arange(P.elems.size), b)


def test_census_of_the_cuts():
    reg, _ = registration(dict(CFG, riemann_solve_type=3))
    nfp = int(reg["sizes"][2])
    sizes, n_nbr, n_i = [], [], []
    ratio2 = shifted = twice = two_peers = False
    neg = [0, 0, 0]
    for name in CUTS:
        parts = RP.cut(reg, part_vector(name))
        assert len(parts) == len(CUTS[name][0])
        for r, P in enumerate(parts):
            assert P.elems.size > 0
            sizes.append(P.elems.size)
            n_nbr.append(len(P.segments))
            n_i.append(element_lists(P, nfp)[1].size)
            counts = [s[3] for s in P.segments]
            total = sum(counts)
            assert total == P.L.shape[1] and [s[1] for s in P.segments] == list(np.cumsum([0] + counts[:-1]))
            assert [s[0] for s in P.segments] == sorted(s[0] for s in P.segments) and r not in [s[0] for s in P.segments]
            ratio2 = ratio2 or max(counts) >= 2 * min(counts)
            shifted = shifted or P.segments[-1][1] * len(counts) != total * (len(counts) - 1)
            ele = P.L[0] // nfp
            peer = np.repeat([s[0] for s in P.segments], counts)
            for el in np.unique(ele):
                peers = peer[ele == el]
                twice = twice or np.bincount(peers).max() >= 2
                two_peers = two_peers or np.unique(peers).size >= 2
            # left normals of the lower rank's sides: the dominant component of the face's mean normal
            norm = P.reg["norm_fpts"].reshape(-1, 3, order="F")
            for q, first, _, count in P.segments:
                if q > r:
                    for i in range(first, first + count):
                        m = norm[P.L[:, i]].mean(axis=0)
                        d = int(np.argmax(np.abs(m)))
                        neg[d] += int(m[d] < 0)
    print("sizes %s neighbours %s n_list_i %s negative normals %s" % (sizes, n_nbr, n_i, neg))
    assert max(sizes[:4]) >= 2 * min(sizes[:4]) and max(sizes[4:]) >= 2 * min(sizes[4:])
    assert max(n_nbr) >= 4
    assert ratio2 and shifted and twice and two_peers
    assert 0 in n_i and 1 in n_i and any(n >= 3 and n % 2 for n in n_i)
    assert min(neg) >= 8, neg


def test_cut_tables_are_mutually_consistent():
    """Both sides of a rank pair list their shared faces in the same order: flux-point positions of face i of a's segment for b
    coincide (through Rlut, modulo the period) with those of face i of b's segment for a.  And every flux point of every part
    belongs to exactly one face of one of its three tables."""
    reg, pos = registration(dict(CFG, riemann_solve_type=3))
    nfp = int(reg["sizes"][2])
    for name in CUTS:
        parts = RP.cut(reg, part_vector(name))
        for a, A in enumerate(parts):
            seen = np.concatenate([np.ravel(A.reg["int2_L"]), np.ravel(A.reg["int2_R"]), np.ravel(A.L)])
            assert np.array_equal(np.sort(seen), np.arange(nfp * A.elems.size))
            for b, fa, _, count in A.segments:
                B = parts[b]
                fb = [s for s in B.segments if s[0] == a][0][1]
                assert [s for s in B.segments if s[0] == a][0][3] == count
                La, Ra, Lb = A.L[:, fa:fa + count], A.Rlut[:, fa:fa + count], B.L[:, fb:fb + count]
                ob = np.take_along_axis(Lb, Ra, axis=0)  # the record slot Rlut(j) of b's face i is b's j'-th flux point
                pa = pos[La % nfp, A.elems[La // nfp], :]
                pb = pos[ob % nfp, B.elems[ob // nfp], :]
                d = pa - pb
                d -= LENGTH * np.round(d / LENGTH)
                assert np.abs(d).max() < 1e-9


def test_census_of_the_walls_cut():
    """the box with boundary groups on all six sides under ragged4: the boundary table is sliced with the elements, and some
    element carries boundary points, partition-face points and interior partners at once"""
    kw = walls_kw()
    reg, _ = registration(kw)
    nfp = int(reg["sizes"][2])
    parts = cut_of(kw, "ragged4")
    assert sum(P.reg["bdy2_L"].shape[1] for P in parts if "bdy2_L" in P.reg) == reg["bdy2_L"].shape[1] == 6 * 16
    all_three = 0
    for P in parts:
        seen = np.concatenate([np.ravel(P.reg["int2_L"]), np.ravel(P.reg["int2_R"]), np.ravel(P.L), np.ravel(P.reg["bdy2_L"])])
        assert np.array_equal(np.sort(seen), np.arange(nfp * P.elems.size))
        ids = {int(i) for i in np.ravel(P.reg["bdy2_id"])}
        assert ids <= set(range(reg["bc_flags"].shape[1]))
        e_bdy = set(np.unique(P.reg["bdy2_L"] // nfp))
        e_mpi = set(np.unique(P.L // nfp))
        e_int = set(np.unique(np.concatenate([np.ravel(P.reg["int2_L"]), np.ravel(P.reg["int2_R"])]) // nfp))
        all_three += len(e_bdy & e_mpi & e_int)
    assert all_three >= 4, all_three


# ---- the oracle in lockstep against the 1-rank oracle --------------------------------------------------------------------------

ORACLE_ROWS = [dict(riemann_solve_type=3), dict(riemann_solve_type=0), dict(riemann_solve_type=2)]


@pytest.mark.parametrize("kw", ORACLE_ROWS + [FREE_STREAM, dict(riemann_solve_type=3, Mach_c_ic=1.2)],
                         ids=["hllc", "rusanov", "roem", "free_stream", "hllc_mach1.2"])
@pytest.mark.parametrize("name", ["ragged4", "ragged6"])
def test_ragged_invariance_oracle(name, kw):
    """one RK step; not bit-exact: a partition face is evaluated from both sides (left = self on each rank), the interior face
    once from its left cell"""
    kw = dict(CFG, **kw)
    u, div = oracle_parts(kw, name)
    check_invariance(u, div, kw, 1, 1e-12, 1e-11)


def test_walls_invariance_oracle():
    kw = walls_kw()
    u, div = oracle_parts(kw, "ragged4")
    check_invariance(u, div, kw, 1, 1e-12, 1e-11)


def self_tables(kw, virtual=VIRTUAL3):
    reg = registration(kw)[0]
    d, L, Rlut, seg = RP.cut_self(reg, part_vector(virtual))
    return [(d, L, Rlut, seg)]


def test_cut_self_three_virtual_parts_oracle():
    """one rank, three virtual parts: six directed segments of unequal size to the rank itself, send_first != recv_first"""
    kw = dict(CFG, riemann_solve_type=3)
    tables = self_tables(kw)
    seg = tables[0][3]
    counts = [s[3] for s in seg]
    assert len(seg) == 6 and all(s[0] == 0 for s in seg) and len(set(counts)) >= 2
    assert all(s[1] != s[2] for s in seg) and sorted(s[1] for s in seg) == sorted(s[2] for s in seg)
    case = RP.oracle_lockstep(tables, 1)[0]
    check_invariance(case.arr["u0"], case.arr["div_tconf_upts"], kw, 1, 1e-12, 1e-11)


# ---- the mixed channel: virtual parts inside each class ------------------------------------------------------------------------

def mixed_virtual_parts(per, classes):
    """Three virtual parts per class of mixed_p3_channel, by the elements' centroid in x (the periodic streamwise direction).
    The prisms' quadrilateral faces with a normal in x would be cut by it, and the reference's LDG switch
    (src/inters.cpp:568-581) reads a normal component that is rounding noise at points of such faces -- decided by the LEFT
    normal on an interior face and by each side's own on a partition face (test_simplex_les_on_partitioned_blocks) -- so the
    prisms are cut by their centroid in z instead, whose faces are the triangles."""
    part = {}
    for c in classes:
        x = per[c]["shape"].mean(axis=1)  # (3, n_eles) centroids
        s = x[2] if c == 3 else x[0]
        order = np.argsort(s, kind="stable")
        v = np.zeros(s.size, dtype=np.int64)
        n = s.size
        v[order[n // 2:]] = 1          # unequal shares: 1/2, 1/3, 1/6
        v[order[n // 2 + n // 3:]] = 2
        part[c] = v
    return part


class PartitionedMixedOracle(MU.MixedOracle):
    """MixedOracle with partition-face blocks the rank exchanges with itself, in the reference's order (src/solver.cpp:59-221)"""

    def __init__(self, d, rest, mpi):
        import oracle_py as O
        super().__init__(d)
        self.faces = []
        for a, b, L, R in rest:
            L, R = RP.F32(L), RP.F32(R)
            f = O.IntInters()
            f.n_fpts_per_inter, f.n_inters = L.shape
            f.L, f.R = O.iptr(L), O.iptr(R)
            self.faces.append((a, b, f, (L, R)))
        self.mpi = []
        for a, L, Rlut, seg in mpi:
            nf, nd = self.case[a].n_fields, self.case[a].n_dims
            m = O.MpiInters()
            m.n_fpts_per_inter, m.n_inters = L.shape
            m.L, m.Rlut = O.iptr(L), O.iptr(Rlut)
            buf = {k: np.zeros(L.size * nf * (1 if "disu" in k else nd)) for k in ("out_disu", "in_disu", "out_grad", "in_grad")}
            for k, v in buf.items():
                setattr(m, k, v.ctypes.data_as(O.dp))
            self.mpi.append((a, m, buf, seg, (L, Rlut)))

    def exchange(self, kind):
        o, i = RP.KIND_BUF[kind]
        for a, m, buf, seg, _ in self.mpi:
            RP.move_records([seg], [buf[o]], [buf[i]], buf[o].size // m.n_inters)

    def CalcResidual(self, hook=None):
        o, P = self.o, C.byref(self.params)
        E = {c: C.byref(self.e[c]) for c in self.classes}
        for c in self.classes: o.orc_extrapolate_solution(E[c])
        for a, m, _, _, _ in self.mpi: o.orc_mpi_pack_solution(C.byref(m), E[a])
        for c in self.classes: o.orc_calculate_gradient(E[c])
        for c in self.classes: o.orc_evaluate_invFlux(E[c], P)
        for a, b, f, _ in self.faces: o.orc_int_calculate_common_invFlux_lr(C.byref(f), E[a], E[b], P)
        for a, f, _ in self.bdy: o.orc_bdy_evaluate_boundaryConditions_invFlux(C.byref(f), E[a], P)
        self.exchange(0)
        for a, m, _, _, _ in self.mpi: o.orc_mpi_calculate_common_invFlux(C.byref(m), E[a], P)
        for c in self.classes: o.orc_correct_gradient(E[c])
        for a, m, _, _, _ in self.mpi: o.orc_mpi_pack_corrected_gradient(C.byref(m), E[a])
        for c in self.classes: o.orc_evaluate_viscFlux(E[c], P)
        for c in self.classes: o.orc_extrapolate_totalFlux(E[c])
        for c in self.classes: o.orc_calculate_divergence(E[c])
        for a, b, f, _ in self.faces: o.orc_int_calculate_common_viscFlux_lr(C.byref(f), E[a], E[b], P)
        for a, f, _ in self.bdy: o.orc_bdy_evaluate_boundaryConditions_viscFlux(C.byref(f), E[a], P)
        self.exchange(1)
        for a, m, _, _, _ in self.mpi: o.orc_mpi_calculate_common_viscFlux(C.byref(m), E[a], P)
        bad = -1
        for c in self.classes:
            bad = max(bad, o.orc_calculate_corrected_divergence(E[c]))
        return bad


def mixed_cut():
    d = dict(np.load(os.path.join(GOLDEN, "mixed_p3_channel.npz")))
    blocks = MU.split(d)
    classes, per, faces, bdy = blocks
    rest, mpi = RP.cut_self(blocks, mixed_virtual_parts(per, classes))
    return d, blocks, rest, mpi


def test_cut_self_mixed_channel_oracle():
    """the mixed channel with three virtual parts per class (class-to-itself faces only), against MixedOracle on the undivided
    mesh after every stage of a time step"""
    d, (classes, per, faces, bdy), rest, mpi = mixed_cut()
    assert {a for a, _, _, _ in mpi} == {2, 3}
    for a, L, Rlut, seg in mpi:
        assert all(s[0] == 0 for s in seg) and len(seg) % 2 == 0 and sum(s[3] for s in seg) == L.shape[1]
    assert max(len(seg) for _, _, _, seg in mpi) >= 4 and any(len({s[3] for s in seg}) >= 2 for _, _, _, seg in mpi)
    one, cut = MU.MixedOracle(d), PartitionedMixedOracle(d, rest, mpi)
    assert int(cut.params.viscous) == 1
    nstage = int(d["c2_sizes"][7])
    for rk in range(nstage):
        assert one.CalcResidual() == -1 and cut.CalcResidual() == -1
        for c in classes:
            print("stage %d class %d: rel(div) %.3g" % (rk, c, rel(cut.arr(c, "div_tconf_upts"), one.arr(c, "div_tconf_upts"))))
            assert rel(cut.arr(c, "div_tconf_upts"), one.arr(c, "div_tconf_upts")) < 1e-11
        one.AdvanceSolution(rk)
        cut.AdvanceSolution(rk)
        for c in classes:
            assert rel(cut.arr(c, "u0"), one.arr(c, "u0")) < 1e-12


# ---- the comparison sees a mis-routed record (CPU only: a wrong table never runs on the device) ---------------------------------

def swap_recv_first(tables):
    """the first two segments of the rank with the most faces receive in each other's place: the second one first, the first
    one behind it (their lengths differ, so exchanging the two numbers alone would write past the buffer's end)"""
    r = int(np.argmax([t[1].shape[1] for t in tables]))
    reg, L, Rlut, seg = tables[r]
    seg = list(seg)
    assert seg[0][3] != seg[1][3] and seg[0][2] == 0 and seg[1][2] == seg[0][3]
    seg[0], seg[1] = seg[0][:2] + (seg[1][3], seg[0][3]), seg[1][:2] + (0, seg[1][3])
    tables = list(tables)
    tables[r] = (reg, L, Rlut, seg)
    return tables


def reverse_one_rlut_column(tables):
    reg, L, Rlut, seg = tables[0]
    Rlut = Rlut.copy(order="F")
    Rlut[:, 3] = Rlut[::-1, 3]
    tables = list(tables)
    tables[0] = (reg, L, Rlut, seg)
    return tables


@pytest.mark.parametrize("spoil", [swap_recv_first, reverse_one_rlut_column])
def test_misrouted_records_miss_the_tolerance_by_three_orders(spoil):
    kw = dict(CFG, riemann_solve_type=3)
    u, div = oracle_parts(kw, "ragged4", spoil=spoil)
    u1, div1 = undivided(kw, 1)
    print("%s: rel(u) %.3g rel(div) %.3g" % (spoil.__name__, rel(u, u1), rel(div, div1)))
    assert rel(u, u1) > 1e3 * 1e-12
    assert rel(div, div1) > 1e3 * 1e-11


# ---- the device ---------------------------------------------------------------------------------------------------------------

GPU_ROWS = [dict(riemann_solve_type=3, Mach_c_ic=1.2), dict(riemann_solve_type=2, Mach_c_ic=1.2), dict(riemann_solve_type=3)]
TOL_U, TOL_DIV = 1e-11, 5e-10


def gpu_parts(kw, name, mode, n_steps=2, options=()):
    parts = cut_of(kw, name)
    assert len(parts) <= 6
    out, grids = RP.gpu_lockstep(RP.part_tables(parts), n_steps, mode, options)
    shape = undivided(kw, n_steps)[0].shape
    return RP.assemble(parts, [o[0] for o in out], shape), RP.assemble(parts, [o[1] for o in out], shape), grids


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["methods", "fused", "fused2"])
@pytest.mark.parametrize("kw", GPU_ROWS, ids=["hllc_mach1.2", "roem_mach1.2", "hllc"])
@pytest.mark.parametrize("name", ["ragged4", "ragged6"])
def test_gpu_ragged_invariance(name, kw, mode):
    """two RK steps of every part on the device, the records moved between the parts' contexts by device-to-device copies"""
    kw = dict(CFG, **kw)
    u, div, _ = gpu_parts(kw, name, mode)
    check_invariance(u, div, kw, 2, TOL_U, TOL_DIV)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["methods", "fused"])
def test_gpu_ragged_walls(mode):
    kw = walls_kw()
    u, div, _ = gpu_parts(kw, "ragged4", mode)
    check_invariance(u, div, kw, 2, TOL_U, TOL_DIV)


@pytest.mark.gpu
def test_gpu_ragged_order_3():
    """a second tensor size for the element lists and the packed operator rows"""
    kw = dict(CFG, riemann_solve_type=0, order=3)
    u, div, _ = gpu_parts(kw, "ragged4", "fused")
    check_invariance(u, div, kw, 2, TOL_U, TOL_DIV)


@pytest.mark.gpu
def test_gpu_ragged_lists_loop():
    """persistent_grid_cap 2: the flux and update kernels of every part walk its 40, 12, 8 or 4 elements with two workgroups
    (hfx_stage_partitioned launches them on all elements of the rank; the lists: test_gpu_rccl_cut_self_three_virtual_parts)"""
    kw = dict(CFG, riemann_solve_type=3)
    u, div, grids = gpu_parts(kw, "ragged4", "fused", options=(("persistent_grid_cap", 2),))
    print("grids %s" % (grids,))
    for g in grids:
        assert g and {s for s, _, _ in g} == {1, 3}, g  # flux / gradient kernel, update / residual kernel
        for slot, grid, work in g:
            assert grid == min(work, 2) and work > grid, (slot, grid, work)
    assert max(-(-work // grid) for g in grids for _, grid, work in g) >= 3
    check_invariance(u, div, kw, 2, TOL_U, TOL_DIV)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n_list_i,fused_mode,cap", [(5, 3, 3, 0), (5, 3, 2, 0), (1, 1, 3, 0), (8, 0, 3, 0), (2, 5, 3, 2)])
def test_gpu_rccl_cut_self_three_virtual_parts(seed, n_list_i, fused_mode, cap):
    """hfx_run_steps_partitioned over the library's RCCL transport: one rank, three virtual parts of the 64-hex box -- six
    segments of unequal size to the rank itself, send_first != recv_first.  This loop (not hfx_stage_partitioned's phases) runs
    its flux and update kernels on the element lists of fused_build(..., allow_unpaired = true): the seeds leave 3 (1 + 2), 1
    (0 + 1), 0 and 5 (2 + 3, walked by two workgroups each) elements free of partition-face points."""
    import hfx
    kw = dict(CFG, riemann_solve_type=3)
    (reg, L, Rlut, seg), = self_tables(kw, (VIRTUAL3[0], seed))
    assert len(seg) == 6 and all(s[1] != s[2] for s in seg) and len({s[3] for s in seg}) >= 2
    assert BOX[0] * BOX[1] * BOX[2] - np.unique(L // int(reg["sizes"][2])).size == n_list_i
    r = RP.GpuPart(reg, L, Rlut, seg, fused_mode=fused_mode, options=(("persistent_grid_cap", cap),) if cap else ())
    comm = hfx.Comm(r.ctx.h, hfx.comm_unique_id(), 1, 0)
    try:
        fi = (C.c_void_p * len(r.ints))(*[f.h for f in r.ints])
        fm = (C.c_void_p * 1)(r.m.h)
        hfx.check(hfx.lib().hfx_run_steps_partitioned(r.e.h, fi, C.c_int(len(r.ints)), fm, C.c_int(1), comm.h, C.c_int(2)))
        r.ctx.synchronize()
        u, div = r.e.download(hfx.DISU_UPTS0), r.e.download(hfx.DIV_TCONF_UPTS)
        grids = hfx.fused_launch_grids(r.e.h)
    finally:
        comm.close()
        r.close()
    print("n_list_i %d, fused mode %d: grids %s" % (n_list_i, fused_mode, grids))
    if fused_mode == 3:  # the update on the two lists; the flux kernel on the lists that are not empty
        assert [w for s, _, w in grids if s == 3] == [64 - n_list_i] + ([n_list_i] if n_list_i else [])
        assert [w for s, _, w in grids if s == 1] == [w for w in (n_list_i // 2, 64 - n_list_i, n_list_i - n_list_i // 2) if w]
    if cap:
        assert all(g == min(w, cap) for _, g, w in grids)
    check_invariance(u, div, kw, 2, TOL_U, TOL_DIV)


@pytest.mark.gpu
def test_gpu_mixed_channel_on_three_virtual_parts():
    """hfx_run_steps_partitioned_blocks on the mixed channel with three virtual parts per class, against the genuine reference's
    undivided run after every step (the tolerance of test_mixed_channel_on_partitioned_blocks)"""
    import hfx
    d, (classes, per, faces, bdy), rest, mpi = mixed_cut()
    ctx = hfx.Context(0)
    ctx.set_params(hfx.params_from(per[classes[0]]))
    E = {}
    for c in classes:
        sz = [int(v) for v in per[c]["sizes"]]
        E[c] = hfx.Eles(ctx, sz[:5], per[c], ele_type=sz[6], order=sz[5])
        E[c].upload(hfx.DISU_UPTS0, per[c]["u_init"])
    M = []
    for a, L, Rlut, seg in mpi:
        M.append(hfx.MpiInters(ctx, E[a], L, Rlut))
        M[-1].set_neighbours(seg)
    F = [hfx.IntInters(ctx, E[a], E[b], L, R) for a, b, L, R in rest]
    for a, L, ids in bdy:
        F.append(hfx.BdyInters(ctx, E[a], L, ids, hfx.bc_records(d["bc_flags"], d["bc_params"]), float(np.ravel(d["bc_R_ref"])[0]),
                               int(np.ravel(d["ramp_counter"])[0])))
    comm = hfx.Comm(ctx.h, hfx.comm_unique_id(), 1, 0)
    nstage = int(d["c2_sizes"][7])
    steps = sorted({int(k.split("_")[2][4:]) for k in d if k.startswith("c2_u_step")})
    try:
        for st in steps:
            hfx.run_steps_partitioned_blocks([E[c] for c in classes], F, M, comm, 1)
            for c in classes:
                k = "c%d_u_step%d_stage%d" % (c, st, nstage - 1)
                print("%s: %.3g" % (k, rel(E[c].download(hfx.DISU_UPTS0), d[k])))
                assert rel(E[c].download(hfx.DISU_UPTS0), d[k]) < 1e-11, k
        for c in classes:
            assert E[c].check_nan() == -1
    finally:
        comm.close()
        for f in F + M:
            f.close()
        for c in classes:
            E[c].close()
        ctx.close()
