"""The fixtures of the LES closure on triangles (tests/golden/tris_les, tools/capture_tris_les.py) without a GPU: the conditions of
tests/tri_les_util.py recomputed on every file, and the oracle on every block tests/test_gpu_tris_les.py cuts out of them."""
import numpy as np
import pytest

import tri_util as T
import tri_les_util as TL

NAMES = TL.names()
EXPECTED = ["tl_p1_wale", "tl_p2_wale", "tl_p3_cylinder", "tl_p3_sim", "tl_p3_smag_walls", "tl_p3_svv", "tl_p3_wale", "tl_p3_wsm",
            "tl_p4_wale", "tl_p5_wale"]


def test_the_fixtures_are_there():
    assert NAMES == EXPECTED


@pytest.mark.parametrize("name", EXPECTED)
def test_conditions(name):
    """lockstep at tri_util's bars, moved by more than 1e-7 without the closure, the Jacobian identity below 1e-12, and the case's own"""
    d = TL.load(name)
    cond = TL.conditions(d, name)
    print(name, {k: v for k, v in cond.items() if k != "failures"})
    assert not cond["failures"], cond["failures"]
    assert cond["moved"] > TL.MOVED and cond["jacobian"] < TL.JACOBIAN_CAPTURE
    want = {"tl_p3_smag_walls": 0, "tl_p3_wsm": 2, "tl_p3_sim": 4, "tl_p3_svv": 3}.get(name, 1)
    assert TL.model(d) == want
    if name == TL.WALLS:
        assert cond["wall_points"] > 0 and cond["grid_points"] > 0
        assert sum(k.startswith("bdy") and k.endswith("_L") for k in d) > 0
    if name in TL.SIMILARITY:
        assert cond["Lu"] > 0.0 and cond["Le"] > 0.0
    if name == TL.CYLINDER:
        J = np.asarray(d["Jacobian_fpts"])
        assert int(d["sizes"][0]) == 714 and (np.ptp(J.reshape(4, int(d["sizes"][2]), -1), axis=1) > 0).any()  # (curved: it varies along an element's flux points)


def test_conditions_of_the_shock_fixture():
    """tl_p3_cylinder_shock (the genuine driver): restart state at 1e-12, Tecplot sensor at 1e-10, no sensor within 5e-4 of s0, some
    stage filters some elements and not all, moved by more than 1e-7 without the closure, the Jacobian identity"""
    import tri_shock_util as TS
    d = TL.load_shock()
    cond, ref = TL.shock_conditions(d)
    print({k: v for k, v in cond.items() if k != "failures"})
    assert not cond["failures"], cond["failures"]
    assert TL.model(d) == 1 and int(TS.scalar(d, "shock_cap")) == 1 and int(d["sizes"][0]) == 714
    plain = TS.reference("ts_p3_cylinder")  # (the same keys without the closure: the pair is not either ingredient alone)
    assert T.relerr(plain["u"][-1], ref["u"][-1]) > TL.MOVED
    assert T.relerr(TL.reference(TL.CYLINDER)[-1]["u"], ref["u"][-1]) > TL.MOVED


def test_the_all_ones_jacobian_fails_the_identity():
    """what tests/test_gpu_tris.py, test_gpu_tris_shock.py and test_gpu_tris_overint.py register: far from the stage's 1e-9 on every mesh"""
    for name in ("tri_p3_n4_deformed", "tri_p3_cylinder", "tri_p1_n4_deformed"):
        d = T.load(name)
        ones = np.ones((2, 2, int(d["sizes"][2]), int(d["sizes"][0])), order="F")
        assert TL.jacobian_residual(ones, d) > 1e-3


@pytest.mark.parametrize("name,n", TL.order_blocks() + [("tl_p3_wsm", 2 * T.GROUP[3] + 1)])
def test_cut_blocks_are_sound(name, n):
    """the oracle on every cut block: finite, no NaN report, the closure's arrays sliced with the elements, the identity kept"""
    d = TL.block(n, name)
    ne, nu, nfp = int(d["sizes"][0]), int(d["sizes"][1]), int(d["sizes"][2])
    assert ne == n and d["Jacobian_fpts"].shape == (2, 2, nfp, n)
    assert TL.jacobian_residual(d["Jacobian_fpts"], d) < TL.JACOBIAN_CAPTURE
    ref = TL.block_reference("%s %d" % (name, n), d)
    assert len(ref) == TL.N_STEPS and all(r["bad"] == -1 and np.isfinite(r["u"]).all() for r in ref)
    plain = TL.G.oracle_steps(TL.without_les(d), TL.N_STEPS)
    assert T.relerr(plain[-1]["u"], ref[-1]["u"]) > TL.MOVED  # (the closure moves the cut block too)
    assert nu == TL.load(name)["sizes"][1]


@pytest.mark.parametrize("name", ["tl_p3_wale", "tl_p3_wsm", "tl_p3_smag_walls"])
def test_tiled_blocks_are_sound(name):
    """three copies of a 32-element fixture (one group each: the partitioned tests cut the first and keep two interior groups)"""
    d = TL.tiled(name)
    ref = TL.block_reference(name + " tiled", d)
    assert all(r["bad"] == -1 and np.isfinite(r["u"]).all() for r in ref)
    assert int(d["sizes"][0]) == 3 * int(TL.load(name)["sizes"][0])
