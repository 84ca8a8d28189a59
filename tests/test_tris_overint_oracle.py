"""Over-integration on triangles without a GPU: every fixture of tests/golden/tris_overint (tools/capture_tris_overint.py) against the
oracle in lockstep, the conditions the capture tool enforced recomputed, and every block tests/test_gpu_tris_overint.py runs shown to
be a sound input (the oracle's two steps are finite and report no NaN)."""
import json

import numpy as np
import pytest

import tri_util as T
import tri_overint_util as TO
import tri_shock_util as TS

NAMES = TO.names()
WANT = {"to_p1_o3": (1, 10), "to_p1_o2": (1, 6), "to_p2": (2, 21), "to_p3": (3, 28), "to_p3_o2": (3, 6), "to_p3_bdy": (3, 6),
        "to_p4": (4, 28), "to_p5": (5, 36), "to_p3_cylinder": (3, 15)}  # fixture -> (order, n_cubpts)


def test_the_fixtures_are_there():
    assert sorted(NAMES) == sorted(WANT), NAMES
    for name, (order, nc) in WANT.items():
        d = TO.load(name)
        assert int(d["sizes"][5]) == order and TO.chunks_of(d)[0] == nc and int(np.ravel(d["over_int"])[0]) == 1
        assert np.asarray(d["over_int_filter"]).shape == (int(d["sizes"][1]), nc)
        assert np.asarray(d["JGinv_over_int_cubpts"]).shape == (2, 2, nc, int(d["sizes"][0]))
    # whole and partial chunks: NU divides n_cubpts (to_p1_o2), a last partial chunk, one partial chunk alone (n_cubpts < NU)
    assert TO.chunks_of(TO.load("to_p1_o2")) == (6, 3, 2) and TO.chunks_of(TO.load("to_p1_o3")) == (10, 3, 4)
    assert TO.chunks_of(TO.load("to_p3_o2")) == (6, 10, 1) and TO.chunks_of(TO.load("to_p5")) == (36, 21, 2)


@pytest.mark.parametrize("name", NAMES)
def test_conditions(name):
    """lockstep at tri_util's bars; moved by more than 1e-7 without the arrays; the cylinder's metric varies inside an element and
    the straight-sided boxes' does not (beyond rounding)"""
    d = TO.load(name)
    cond = TO.conditions(d, curved=name == TO.CURVED)
    print("%s: lockstep worst %s %.1e, moved %.2e, metric variation %.1e" % (name, cond["worst"][0], cond["worst"][1], cond["moved"],
                                                                            cond["metric_variation"]))
    assert not cond["failures"], cond["failures"]
    if name != TO.CURVED:
        assert cond["metric_variation"] < 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_delta_files(name):
    """a file holds its own arrays and results; only a case that changes keys of its base holds more"""
    own = dict(np.load(TO.GOLDEN + "/" + name + ".npz"))
    meta = json.loads(bytes(own["meta_json"]).decode())
    extra = [k for k in own if k not in TO.OWN and not k.startswith(TO.RESULTS) and k not in ("meta_json", "based_on", "dropped")]
    assert all(k in own for k in TO.OI_KEYS) and meta["level"] == 1 and meta["based_on"] == bytes(own["based_on"]).decode()
    assert not extra or name.startswith("to_p1"), extra


def blocks():
    for name, n in TO.order_blocks():
        yield "%s %d" % (name, n), lambda name=name, n=n: TO.block(n, name)
    for n in TO.edge_counts(TO.CUT_FROM):
        yield "to_p3 %d inviscid" % n, lambda n=n: TO.block(n, TO.CUT_FROM, 0)
    yield "perturbed", TO.perturbed_block


@pytest.mark.parametrize("what,make", list(blocks()), ids=[w for w, _ in blocks()])
def test_blocks_are_sound_inputs(what, make):
    d = make()
    ref = TO.block_reference(what, d)
    assert len(ref) == TO.N_STEPS and all(r["bad"] == -1 and np.isfinite(r["u"]).all() for r in ref), what
    assert TO.chunks_of(d)[0] == np.asarray(d["JGinv_over_int_cubpts"]).shape[2] and np.asarray(d["JGinv_over_int_cubpts"]).shape[3] == int(d["sizes"][0])


def test_the_perturbed_block_differs_from_its_twin():
    n = T.GROUP[3] + 1
    a = TO.block_reference("perturbed", TO.perturbed_block())
    b = TO.block_reference("to_p3 %d" % n, TO.block(n, TO.CUT_FROM))
    moved = T.relerr(a[-1]["u"], b[-1]["u"])
    print("perturbed metrics move the state by %.2e" % moved)
    assert moved > TO.MOVED
    assert TO.metric_variation(TO.perturbed_block()) > 0.05


@pytest.mark.parametrize("name", sorted(TO.SHOCK_ON))
def test_with_shock_capturing(name):
    """both ingredients in the oracle: finite, no sensor near s0, some element filtered and some not; each ingredient moves the state"""
    d, ref = TO.with_shock(name)
    both = ref["u"][-1]
    no_oi = TS.lockstep(TO.without_over_int(d), TO.N_STEPS)["u"][-1]
    no_shock = TO.reference(name)[-1]["u"]
    print("%s: without over-integration %.2e, without the filter %.2e" % (name, T.relerr(no_oi, both), T.relerr(no_shock, both)))
    assert np.isfinite(both).all() and T.relerr(no_oi, both) > TO.MOVED and T.relerr(no_shock, both) > TO.MOVED
