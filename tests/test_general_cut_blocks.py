"""tests/general_util.py -- blocks of any element count cut from the simplex fixtures -- checked without a GPU: the cut keeps the
tables and arrays consistent (the oracle on a permuted block reproduces the genuine reference's states, permuted), and every
block the GPU tests of the general fused stage run (tests/test_gpu_general_batches.py) is a sound input: the oracle reports no
NaN, density and pressure stay positive, and EVERY element moves measurably in a step -- so an element a kernel skipped, or wrote
twice, cannot hide below the tolerance."""
import numpy as np
import pytest

import general_util as G

BLOCKS = [("class", c, n) for c in G.CLASSES for n in G.COUNTS] + [("feature", f, 17) for f in G.FEATURES] + [("mixed", "mixed_p3_channel", 38)]
PERMUTED = ["tet_p2_n2_deformed", "pri_p3_n2_deformed", "tet_p1_n2_deformed", "pri_p1_n2_deformed", "tet_p4_n2_deformed",
            "tet_p2_les_wale", "tet_p3_les_wsm", "tet_p2_overint", "tet_p3_shock", "tet_p2_cfl_local", "mixed_p3_channel"]


def relerr(a, b):
    s = np.abs(b).max()
    return np.abs(a - b).max() / (s if s > 0 else 1.0)


def get(kind, name, n):
    if kind == "class":
        return G.class_block(name, n)
    if kind == "feature":
        return G.feature_block(name, n)
    return G.mixed_block()


@pytest.mark.parametrize("name", ["tet_p2_n2_deformed", "pri_p3_n2_deformed", "tet_p2_les_wale", "tet_p2_cfl_local"])
def test_keeping_all_elements_reproduces_the_fixture(name):
    d = G.load(name)
    c = G.cut(d, np.arange(int(d["sizes"][0])), G.load(G.BC_FROM), np.arange(6))
    assert not any(k.startswith("bdy") for k in c)
    for k, v in d.items():
        if k.startswith(G.STALE):
            assert k not in c
        else:
            assert np.array_equal(c[k], v), k


def test_keeping_all_elements_of_the_mixed_channel_reproduces_the_fixture():
    d = G.load("mixed_p3_channel")
    c = G.cut_mixed(d, {2: np.arange(24), 3: np.arange(16)})
    stale = [k for k in d if k.startswith(G.STALE) or k[3:].startswith(G.STALE)]
    assert sorted(c) == sorted(set(d) - set(stale))
    for k in c:
        assert np.array_equal(c[k], d[k]), k


@pytest.mark.parametrize("name", PERMUTED)
def test_oracle_on_a_permuted_block_equals_the_reference_permuted(name):
    """every element in another place, every array sliced, every table renumbered: the states are the genuine reference's, in the
    new order (an array sliced on the wrong axis, or a table entry renumbered wrongly, changes them)"""
    d = G.load(name)
    p, keep = G.permuted(name)
    if "classes" in d:
        nstage = int(d["c2_sizes"][7])
        ref = G.mixed_oracle_steps(p, 1)
        assert ref[0]["bad"] == -1
        for c in keep:
            assert relerr(ref[0][c]["u"], d["c%d_u_step0_stage%d" % (c, nstage - 1)][:, keep[c], :]) < 1e-13, c
        return
    assert not any(k.startswith("bdy") for k in p)
    nstage = int(d["sizes"][7])
    steps = sorted({int(k.split("_")[1][4:]) for k in d if k.startswith("u_step")})
    ref = G.oracle_steps(p, len(steps))
    for st in steps:
        assert ref[st]["bad"] == -1
        assert relerr(ref[st]["u"], d["u_step%d_stage%d" % (st, nstage - 1)][:, keep, :]) < 1e-13, st
        assert np.array_equal(p["u_step%d_stage%d" % (st, nstage - 1)], d["u_step%d_stage%d" % (st, nstage - 1)][:, keep, :])


def test_tiles_are_disjoint_copies_with_their_own_state():
    d = G.load("pri_p2_n2_deformed")
    t = G.tile(d, 3)
    ne, nstage = int(d["sizes"][0]), int(d["sizes"][7])
    assert int(t["sizes"][0]) == 3 * ne and (G.face_census(t) == 1).all()
    ref = G.oracle_steps(t, 1)[0]
    assert relerr(ref["u"][:, :ne, :], d["u_step0_stage%d" % (nstage - 1)]) < 1e-13  # copy 0 carries the fixture's state
    assert relerr(ref["u"][:, ne:2 * ne, :], ref["u"][:, :ne, :]) > 1e-3            # copy 1 its own
    assert np.array_equal(t["u_init"][:, 2 * ne:, :], 1.04 * d["u_init"])


@pytest.mark.parametrize("kind,name,n", BLOCKS)
def test_every_flux_point_of_a_cut_block_belongs_to_exactly_one_face(kind, name, n):
    d = get(kind, name, n)
    if kind == "mixed":
        classes, per, faces, bdy = G.MU.split(d)
        count = {c: np.zeros(int(per[c]["sizes"][0]) * int(per[c]["sizes"][2]), dtype=np.int64) for c in classes}
        for a, b, L, R in faces:
            np.add.at(count[a], np.ravel(L), 1)
            np.add.at(count[b], np.ravel(R), 1)
        for a, L, ids in bdy:
            np.add.at(count[a], np.ravel(L), 1)
        assert [int(per[c]["sizes"][0]) for c in classes] == [G.MIXED_KEEP[c] for c in classes]
        assert all((count[c] == 1).all() for c in classes)
        # partner words cross the blocks, the fixture's walls are present as well as the cut faces
        assert {(a, b) for a, b, _, _ in faces} >= {(2, 3), (3, 2)}
        ids = np.concatenate([i for _, _, i in bdy])
        assert set(ids[ids < 3]) == {1, 2} and (ids >= 3).any()
        return
    assert int(d["sizes"][0]) == n
    assert (G.face_census(d) == 1).all()
    if n > 1:
        assert any(k.startswith("int") for k in d)
    assert any(k.startswith("bdy") for k in d)


@pytest.mark.parametrize("kind,name,n", BLOCKS)
def test_blocks_of_the_gpu_tests_are_sound_inputs(kind, name, n):
    """the oracle returns -1 and keeps rho and p positive after every step, and every element -- the last n mod 16 included --
    moves by more than 1e-6 of max |u| in every step"""
    d = get(kind, name, n)
    ref = G.reference((kind, name, n), d)
    gamma = float(np.ravel(d["gamma"])[0])
    assert len(ref) == G.N_STEPS
    for c in ([int(x) for x in d["classes"]] if kind == "mixed" else [None]):
        before = d["u_init"] if c is None else d["c%d_u_init" % c]
        for st, r in enumerate(ref):
            assert r["bad"] == -1, (st, r["bad"])
            u = r["u"] if c is None else r[c]["u"]
            assert np.isfinite(u).all()
            rho, p = G.primitive_minima(u, gamma)
            assert rho > 0.0 and p > 0.0, (st, rho, p)
            moves = G.element_moves(before, u)
            assert moves.min() > 1e-6, (st, int(moves.argmin()), moves.min())
            before = u
