"""Mixed quadrilateral / triangle meshes without a GPU: the fixtures under tests/golden/mixed2d (tools/capture_mixed2d.py, the
genuine reference's harness) against the oracle, and the soundness of every input tests/test_gpu_mixed2d.py builds from them
(tests/mixed2d_util.py): tiled fixtures, blocks cut at the edges of the fused stage's groups, the quadrilateral class alone, a
triangle fixture split into two element blocks.

Bars: tests/tri_util.py's (1e-13 of the array's largest magnitude, 1e-12 with boundary faces)."""
import json

import numpy as np
import pytest

import general_util as G
import mixed2d_util as X
import mixed_util as MU
import tri_util as T

FIXTURES = ["mx_p1_n4", "mx_p2_n4", "mx_p3_n4", "mx_p4_n4", "mx_p3_walls", "mx_p2_inviscid", "mx_p2_roem_sutherland", "mx_p2_rusanov_ldg"]
ALL_PAIRS = {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_all_fixtures_are_there():
    assert X.names() == sorted(FIXTURES)


@pytest.mark.parametrize("name", FIXTURES)
def test_lockstep_with_the_reference(name):
    """every dumped stage state of both classes (mx_p2_n4: every intermediate of the first residual too)"""
    d = X.load(name)
    errs = X.lockstep(d)
    assert not T.failures(errs), T.failures(errs)
    states = [k for k in errs if "u_step" in k]
    nstage = X.sizes(d, 0)[7]
    assert len(states) == 2 * nstage * len(X.stored_steps(d))
    if name == "mx_p2_n4":
        assert sum(k.startswith(("c0_s0_", "c1_s0_")) for k in errs) >= 18


@pytest.mark.parametrize("name", FIXTURES)
def test_pair_census(name):
    d = X.load(name)
    assert X.classes_of(d) == [0, 1]
    census = X.pair_census(d)
    order = X.sizes(d, 0)[5]
    for c in (0, 1):
        sz = X.sizes(d, c)
        assert (sz[1], sz[2]) == X.POINTS[c][order] and sz[3:7] == [4, 2, order, c]
    if name in ("mx_p1_n4", "mx_p3_n4"):  # 8 triangles, 12 quadrilaterals, 36 interior faces of all four class pairs
        assert census == {(0, 0): 4, (0, 1): 6, (1, 0): 10, (1, 1): 16}
        assert (X.sizes(d, 0)[0], X.sizes(d, 1)[0]) == (8, 12)
    elif name == "mx_p3_walls":
        assert set(census) == ALL_PAIRS
        classes, per, faces, bdy = MU.split(d)
        assert {a for a, _, _ in bdy} == {0, 1}  # walls on the quadrilaterals, in- and outflow on both classes
        fl = np.asarray(d["bc_flags"]).reshape(3, -1, order="F")
        assert len(set(fl[0].tolist())) >= 4
    else:
        assert census == {(0, 0): 20, (1, 0): 8, (1, 1): 12}
    # every flux point of either class belongs to exactly one face
    count = {c: np.zeros(X.sizes(d, c)[0] * X.sizes(d, c)[2], dtype=int) for c in (0, 1)}
    classes, per, faces, bdy = MU.split(d)
    for a, b, L, R in faces:
        np.add.at(count[a], np.ravel(L), 1)
        np.add.at(count[b], np.ravel(R), 1)
    for a, L, ids in bdy:
        np.add.at(count[a], np.ravel(L), 1)
    assert all((count[c] == 1).all() for c in (0, 1))


@pytest.mark.parametrize("name", ["mx_p1_n4", "mx_p3_n4", "mx_p3_walls"])
def test_tiled_copy_0_is_the_fixture(name):
    """tile_mixed: k disjoint copies; copy 0 reproduces the fixture's stage states in the oracle, another copy does not"""
    d = X.load(name)
    k = 3
    t = X.tile_mixed(d, k)
    ne = {c: X.sizes(d, c)[0] for c in (0, 1)}
    for c in (0, 1):
        assert X.sizes(t, c)[0] == k * ne[c]
        assert np.array_equal(t["c%d_u_init" % c][:, :ne[c]], d["c%d_u_init" % c])
        assert T.relerr(t["c%d_u_init" % c][:, ne[c]:2 * ne[c]], 1.02 * d["c%d_u_init" % c]) < 1e-15
    assert X.pair_census(t) == {p: k * n for p, n in X.pair_census(d).items()}
    with_states = dict(t)
    with_states.update({key: v for key, v in d.items() if "u_step" in key})
    errs = X.lockstep(with_states, copy_elements=ne)
    assert not T.failures(errs), T.failures(errs)
    # (copy 1 carries another state: its elements must not meet the fixture's)
    m = G.mixed_oracle_steps(t, 1)
    nstage = X.sizes(d, 0)[7]
    for c in (0, 1):
        want = d["c%d_u_step0_stage%d" % (c, nstage - 1)]
        assert T.relerr(m[0][c]["u"][:, :ne[c]], want) < T.RTOL_BDY
        assert T.relerr(m[0][c]["u"][:, ne[c]:2 * ne[c]], want) > 1e-3


def finite(ref):
    return all(step["bad"] == -1 and all(np.isfinite(step[c]["u"]).all() for c in step if c != "bad") for step in ref)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_cut_blocks_are_sound(order):
    """the blocks at the group edges: the oracle runs them, finite, no NaN report; every flux point has one face; both classes
    have the counts asked for and cross faces remain"""
    for want in X.edge_counts(order):
        d = X.block(order, want[X.TRI], want[X.QUAD])
        assert (X.sizes(d, 0)[0], X.sizes(d, 1)[0]) == (want[X.TRI], want[X.QUAD])
        assert any(a != b for a, b in X.pair_census(d)), X.pair_census(d)
        assert finite(X.reference(("block", order, want[X.TRI], want[X.QUAD]), d)), (order, want)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_quadrilateral_class_alone_is_sound(order):
    g = X.GROUP[X.QUAD][order]
    d = X.quad_block(order, 2 * g + 1)
    assert [int(v) for v in d["sizes"]][:3] == [2 * g + 1, *X.POINTS[X.QUAD][order]] and int(d["sizes"][6]) == 1
    assert (G.face_census(d) == 1).all()
    ref = X.reference(("quad", order), d)
    assert all(s["bad"] == -1 and np.isfinite(s["u"]).all() for s in ref)


def test_split_triangles_is_the_fixture():
    """a triangle fixture as two element blocks with cross faces between them: the mixed oracle meets the fixture's states"""
    d = T.load("tri_p3_n4_deformed")
    ne = int(d["sizes"][0])
    first = np.arange(ne) % 3 != 0
    m = X.split_triangles(d, first)
    census = X.pair_census(m)
    assert set(census) == {(0, 0), (0, 2), (2, 0)} or set(census) == {(0, 0), (0, 2), (2, 0), (2, 2)}
    ref = G.mixed_oracle_steps(m, 2)
    nstage = int(d["sizes"][7])
    for st in range(2):
        want = d["u_step%d_stage%d" % (st, nstage - 1)]
        assert ref[st]["bad"] == -1
        assert T.relerr(ref[st][0]["u"], want[:, first]) < T.RTOL and T.relerr(ref[st][2]["u"], want[:, ~first]) < T.RTOL


@pytest.mark.parametrize("name", X.PHYSICS_ROWS)
def test_physics_rows_move_the_state(name):
    """each physics row moves the final state by more than 1e-6 against mx_p2_n4 (same mesh, same order)"""
    d, base = X.load(name), X.load(X.PHYSICS_BASE)
    nstage = X.sizes(d, 0)[7]
    keys = json.loads(bytes(d["meta_json"]).decode())["keys"]
    assert json.loads(bytes(base["meta_json"]).decode())["keys"] != keys
    for c in (0, 1):
        k = "c%d_u_step0_stage%d" % (c, nstage - 1)
        if name == "mx_p2_inviscid":  # (another initial state: compared as the change of a step relative to the state)
            move = T.relerr(d[k], d["c%d_u_init" % c])
            assert move > 1e-6 and int(np.ravel(d["viscous"])[0]) == 0
        else:
            assert T.relerr(d[k], base[k]) > 1e-6, (name, c)
