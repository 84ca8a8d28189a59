"""Partitioned triangle blocks without a GPU: the cuts tests/test_gpu_tris_partition.py runs are sound inputs.

ragged_partition.cut / cut_self of the triangle fixtures under tests/golden/tris along seeded random-walk part vectors over the
face adjacency; ragged_partition.oracle_lockstep on the parts meets the GENUINE reference's final state of the undivided mesh at
the bar of tests/test_gpu_tris.py (1e-11 of the state's largest magnitude).  The oracle alone is far inside it (1e-16 to 1e-19 were
measured), so the bar is the device tests', not the oracle's.  A census states what the cuts offer to the fused stage's group
lists (csrc/simplex2d.hip: groups of G consecutive elements, a partition group has an element that owns a partition flux point),
and one spoiled table shows that the comparison sees a wrong partner.

The helpers here (part vectors, virtual tables, the census) are imported by the GPU tests."""
import numpy as np
import pytest

import ragged_partition as RP
import tri_util as T

TOL_U = 1e-11
GROUP = T.GROUP                              # elements per group by order: SIMPLEX2D_SIZES of csrc/simplex2d.hpp
CUT4 = ([10, 3, 2, 1], 13)                   # (weights, seed): four ragged parts
VIRTUAL3 = ([3, 2, 1], 3)                    # three virtual parts of one rank (a seed whose six segments differ in size on every fixture)
G_P3 = GROUP[3]


def adjacency(reg):
    """per element the elements across its interior faces"""
    ne, nfp = int(reg["sizes"][0]), int(reg["sizes"][2])
    adj = [[] for _ in range(ne)]
    for t in RP.face_types(reg):
        L, R = np.asarray(reg["int%d_L" % t]), np.asarray(reg["int%d_R" % t])
        for a, b in zip(L[0] // nfp, R[0] // nfp):
            adj[int(a)].append(int(b))
            adj[int(b)].append(int(a))
    return adj


def grow_parts(reg, weights, seed):
    """ragged_partition.grow_parts over the face adjacency of a registration dict: every part grows from a seeded element by a random
    walk over face neighbours until it holds its share; what no walk reached goes to a neighbouring part (or to part 0)"""
    rng = np.random.RandomState(seed)
    adj = adjacency(reg)
    ne = len(adj)
    w = np.array(weights, dtype=np.float64)
    target = np.maximum(1, np.floor(w / w.sum() * ne).astype(int))
    part = -np.ones(ne, dtype=np.int64)
    seeds = rng.choice(ne, size=len(w), replace=False)
    at = [int(s) for s in seeds]
    for p, s in enumerate(seeds):
        part[s] = p
    size = np.ones(len(w), dtype=int)
    for _ in range(200 * ne):
        open_parts = [p for p in range(len(w)) if size[p] < target[p]]
        if not open_parts or (part >= 0).all():
            break
        p = open_parts[rng.randint(len(open_parts))]
        free = [q for q in adj[at[p]] if part[q] < 0]
        if free:
            at[p] = free[rng.randint(len(free))]
            part[at[p]] = p
            size[p] += 1
        else:  # walk on inside the part
            own = [q for q in adj[at[p]] if part[q] == p]
            at[p] = own[rng.randint(len(own))] if own else int(rng.choice(np.flatnonzero(part == p)))
    for _ in range(ne):
        if (part >= 0).all():
            break
        for el in np.flatnonzero(part < 0):
            near = [part[q] for q in adj[el] if part[q] >= 0]
            if near:
                part[el] = near[0]
    part[part < 0] = 0
    return part


def virtual_tables(reg, part):
    """ragged_partition.cut_self for one block of triangles, also where nothing is cut (a block without interior faces, or one whose
    faces all stay inside a virtual part): -> (registration dict with the remaining interior faces, L, Rlut, segments)"""
    nfpi = int(reg["sizes"][5]) + 1
    empty = np.zeros((nfpi, 0), dtype=np.int32, order="F")
    tt = RP.face_types(reg)
    part = np.asarray(part)
    if not tt:
        return dict(reg), empty, empty.copy(order="F"), []
    nfp = int(reg["sizes"][2])
    L, R = np.asarray(reg["int%d_L" % tt[0]]), np.asarray(reg["int%d_R" % tt[0]])
    if (part[L[0] // nfp] == part[R[0] // nfp]).all():
        return dict(reg), empty, empty.copy(order="F"), []
    return RP.cut_self(reg, part)


def block_parts(n, name=T.CUT_FROM):
    """the virtual parts of tri_util.block(n, name), n = 1, G - 1, G + 1, 2 G + 1 at the fixture's G.  1: nothing to cut.  G - 1: one
    partial group, every third element a part.  G + 1: the cut lies inside the whole group and away from element G and its
    neighbours, so that the last partial group is an interior group.  2 G + 1: three runs of about 2 G / 3 consecutive elements."""
    g = T.group_of(name)
    d = T.block(n, name)
    v = np.zeros(n, dtype=np.int64)
    if n == g - 1:
        v = np.arange(n) % 3
    elif n == g + 1:
        adj = adjacency(d)
        near_last = {g} | set(adj[g])
        near_last |= {q for el in list(near_last) for q in adj[el]}
        others = [el for el in range(g) if el not in near_last]
        v[others[0::3]] = 1
        v[others[1::3]] = 2
    elif n == 2 * g + 1:
        v = np.arange(n) // ((n + 2) // 3)  # (runs of 22 at G = 32)
    return v


def group_census(reg, L):
    """(partition groups, interior groups, the last group is partial, it is a partition group) of a block with the partition-face
    table L, as simplex2d_build classifies them"""
    ne, nfp, G = int(reg["sizes"][0]), int(reg["sizes"][2]), GROUP[int(reg["sizes"][5])]
    n_groups = (ne + G - 1) // G
    marked = np.zeros(n_groups, dtype=bool)
    marked[np.unique((np.ravel(L) // nfp) // G)] = True
    return int(marked.sum()), int(n_groups - marked.sum()), ne % G != 0, bool(marked[-1])


def steps_of(d):
    return max(T.stored_steps(d)) + 1


def final_state(d):
    return d["u_step%d_stage%d" % (max(T.stored_steps(d)), int(d["sizes"][7]) - 1)]


# ---- the oracle in lockstep on the parts against the genuine reference -----------------------------------------------------------
@pytest.mark.parametrize("name", ["tri_p3_n4_deformed", "tri_p1_n4_deformed", "tri_p3_bdy", "tri_p2_inviscid"])
def test_four_ragged_parts_meet_the_reference(name):
    d = T.load(name)
    part = grow_parts(d, *CUT4)
    parts = RP.cut(d, part)
    sizes = [P.elems.size for P in parts]
    assert len(parts) == 4 and max(sizes) >= 2 * min(sizes), sizes
    cases = RP.oracle_lockstep(RP.part_tables(parts), steps_of(d))
    u = RP.assemble(parts, [c.arr["u0"] for c in cases], d["u_init"].shape)
    err = T.relerr(u, final_state(d))
    print("%s: four parts of %s elements, state %.2e" % (name, sizes, err))
    assert err < TOL_U


@pytest.mark.parametrize("name", ["tri_p3_n4_deformed", "tri_p3_bdy", "tri_p5_n2_deformed"])
def test_three_virtual_parts_meet_the_reference(name):
    """one rank, three virtual parts: six directed segments of unequal size to the rank itself, send_first != recv_first"""
    d = T.load(name)
    tables = virtual_tables(d, grow_parts(d, *VIRTUAL3))
    seg = tables[3]
    counts = [s[3] for s in seg]
    assert len(seg) == 6 and all(s[0] == 0 for s in seg) and len(set(counts)) >= 2, seg
    assert all(s[1] != s[2] for s in seg) and sorted(s[1] for s in seg) == sorted(s[2] for s in seg)
    case = RP.oracle_lockstep([tables], steps_of(d))[0]
    err = T.relerr(case.arr["u0"], final_state(d))
    print("%s: three virtual parts, segments %s, state %.2e" % (name, counts, err))
    assert err < TOL_U


def test_a_reversed_rlut_column_misses_the_bar():
    d = T.load("tri_p3_n4_deformed")
    reg, L, Rlut, seg = virtual_tables(d, grow_parts(d, *VIRTUAL3))
    bad = np.array(Rlut, order="F")
    bad[:, 0] = bad[::-1, 0]
    assert not np.array_equal(bad, Rlut)
    case = RP.oracle_lockstep([(reg, L, bad, seg)], steps_of(d))[0]
    err = T.relerr(case.arr["u0"], final_state(d))
    print("reversed Rlut column: state %.2e" % err)
    assert err > 1e4 * TOL_U


# ---- what the cuts of the GPU tests offer to the group lists ---------------------------------------------------------------------
GPU_FIXTURES = ["tri_p1_n4_deformed", "tri_p3_n4_deformed", "tri_p5_n2_deformed", "tri_p3_bdy", "tri_p2_inviscid", "tri_p2_rusanov_ldg",
                "tri_p2_roem_sutherland", "tri_p3_cylinder"]
BLOCKS = [1, G_P3 - 1, G_P3 + 1, 2 * G_P3 + 1]


def gpu_cuts():
    for name in GPU_FIXTURES:
        d = T.load(name)
        yield name, d, grow_parts(d, *VIRTUAL3)
    for n in BLOCKS:
        yield "block %d" % n, T.block(n), block_parts(n)


def test_census_of_the_cuts():
    interior_present = zero_interior = partial_on_partition = partial_on_interior = part_without_free_element = False
    for what, d, part in gpu_cuts():
        reg, L, Rlut, seg = virtual_tables(d, part)
        ne, nfp = int(d["sizes"][0]), int(d["sizes"][2])
        # every flux point belongs to exactly one face of one table
        seen = [np.ravel(L)] + [np.ravel(reg[k]) for k in reg if k.startswith(("int", "bdy")) and k.endswith(("_L", "_R"))]
        assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(nfp * ne)), what
        n_part, n_int, partial, last_marked = group_census(reg, L)
        print("%-24s %4d elements: %2d partition groups, %2d interior groups, last partial %s on the %s list" %
              (what, ne, n_part, n_int, partial, "partition" if last_marked else "interior"))
        interior_present = interior_present or (n_int > 0 and n_part > 0)
        zero_interior = zero_interior or n_int == 0
        partial_on_partition = partial_on_partition or (partial and last_marked)
        partial_on_interior = partial_on_interior or (partial and not last_marked and n_part > 0)
        owners = set(np.unique(np.ravel(L) // nfp))
        for p in np.unique(part):
            part_without_free_element = part_without_free_element or set(np.flatnonzero(part == p)) <= owners
    assert interior_present and zero_interior and partial_on_partition and partial_on_interior and part_without_free_element


# (partition groups, interior groups) of block_parts at n = G - 1, G + 1, 2 G + 1, per fixture: what tests/test_gpu_tris_orders.py asserts
# of hfx_simplex2d_partition_plan.  At P1 the one element of group 2 owns no partition face
ORDER_CUTS = {"tri_p1_n4_deformed": [(1, 0), (1, 1), (2, 1)], "tri_p2_n3_deformed": [(1, 0), (1, 1), (3, 0)],
              "tri_p3_n4_deformed": [(1, 0), (1, 1), (3, 0)], "tri_p4_n2_deformed": [(1, 0), (1, 1), (3, 0)],
              "tri_p5_n2_deformed": [(1, 0), (1, 1), (3, 0)]}


def order_cuts():
    """(fixture, n, (partition groups, interior groups))"""
    for name, want in ORDER_CUTS.items():
        g = T.group_of(name)
        for n, w in zip((g - 1, g + 1, 2 * g + 1), want):
            yield name, n, w


def test_block_cuts_are_what_the_gpu_tests_assert():
    """the group counts tests/test_gpu_tris_partition.py and tests/test_gpu_tris_orders.py expect of hfx_simplex2d_partition_plan"""
    got = {n: group_census(*virtual_tables(T.block(n), block_parts(n))[:2])[:2] for n in BLOCKS}
    assert got[1] == (0, 1) and got[G_P3 - 1] == (1, 0) and got[G_P3 + 1] == (1, 1) and got[2 * G_P3 + 1][0] >= 2, got
    assert sorted(ORDER_CUTS) == sorted(T.BY_ORDER.values())
    for name, n, want in order_cuts():
        reg, L, Rlut, seg = virtual_tables(T.block(n, name), block_parts(n, name))
        nfp = int(reg["sizes"][2])
        seen = [np.ravel(L)] + [np.ravel(reg[k]) for k in reg if k.startswith(("int", "bdy")) and k.endswith(("_L", "_R"))]
        assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(nfp * n)), (name, n)
        assert len(seg) == 6 and group_census(reg, L)[:2] == want, (name, n, group_census(reg, L))
