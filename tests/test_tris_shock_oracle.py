"""Shock capturing on triangles without a GPU: the fixtures of tests/golden/tris_shock (tools/capture_tris_shock.py; the genuine
driver with shock_cap 1) against the oracle in lockstep, the numpy operators of hfx.tri_shock_operators, and the inputs the GPU tests
of tests/test_gpu_tris_shock.py cut out of them (tests/tri_shock_util.py).

Bars: the oracle meets the driver's restart state within 1e-12 of its largest value and its Tecplot sensor within 1e-10 of the
largest sensor (the files carry 15 digits); the operators are reproduced at 1e-13; every input keeps every sensor value of every
stage 5e-4 of s0 away from s0 and has a stage that filters some elements and not others."""
import json

import numpy as np
import pytest

import hfx
import tri_util as T
import tri_shock_util as TS
from test_tris_partition_oracle import grow_parts, virtual_tables, group_census

NAMES = ["ts_p1_n4", "ts_p2_cfl_local", "ts_p2_n3", "ts_p3_bdy", "ts_p3_cylinder", "ts_p3_energy", "ts_p3_n4", "ts_p4_n2", "ts_p5_n2"]
BLOCKS = (1, TS.G_P3 - 1, TS.G_P3 + 1)


def test_every_fixture_is_there():
    assert TS.names() == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_lockstep_meets_the_driver(name):
    """conditions 1 and 2 of the capture tool again, 3 and 4 inside TS.reference; the counts in meta_json are the lockstep's"""
    d = TS.load(name)
    ref = TS.reference(name)
    assert ref["bad"] == -1
    steps = [int(s) for s in d["restart_steps"]]
    for i, s in enumerate(steps):
        err = T.relerr(ref["u"][s - 1], d["u_restart"][i])
        print("%s step %d: state %.2e" % (name, s, err))
        assert err < TS.TOL_STATE, (name, s, err)
    big = np.abs(d["sensor_rows"]).max()
    for s in range(TS.n_steps_of(d)):
        err = float(np.abs(ref["sensor"][s] - d["sensor_rows"][s]).max() / big)
        print("%s step %d: sensor %.2e" % (name, s + 1, err))
        assert err < TS.TOL_SENSOR, (name, s, err)
    meta = json.loads(bytes(d["meta_json"]).decode())
    assert meta["filtered_per_stage"] == TS.filtered_counts(ref["stage_sensors"], TS.scalar(d, "s0"))


@pytest.mark.parametrize("name", NAMES)
def test_operators_are_reproduced(name):
    d = TS.load(name)
    iv, ef, norm, high = hfx.tri_shock_operators(d["loc_upts"], int(d["sizes"][5]), TS.scalar(d, "expf_fac"), int(TS.scalar(d, "expf_order")),
                                                 int(TS.scalar(d, "expf_cutoff")))
    assert T.relerr(iv, d["inv_vandermonde"]) < 1e-13 and T.relerr(ef, d["exp_filter"]) < 1e-13
    assert np.array_equal(norm, np.ravel(d["norm_basis_persson"])) and (norm == 1.0).all()
    p = int(d["sizes"][5])
    assert np.array_equal(high, np.ravel(d["persson_high_modes"])) and np.array_equal(np.nonzero(high)[0], np.arange(p * (p + 1) // 2, len(high)))
    # the basis is orthonormal on the reference triangle, so V^-1 V = 1 and the filter keeps the constant mode
    assert np.abs(ef.sum(axis=1) - 1.0).max() < 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_the_filter_matters(name):
    """the lockstep without orc_shock_capture misses the driver's restart state by more than 1e-6"""
    d = TS.load(name)
    plain = TS.reference(name, shock=False)
    miss = T.relerr(plain["u"][int(d["restart_steps"][-1]) - 1], d["u_restart"][-1])
    print("%s without the filter: %.2e" % (name, miss))
    assert miss > 1e-6


def test_cut_blocks_are_sound_inputs():
    """conditions 3 and 4 (inside TS.block); the filtered element lies in the LAST PARTIAL group of at least one block"""
    in_last = []
    for n in BLOCKS:
        b, ref = TS.block(n)
        s0 = TS.scalar(b, "s0")
        groups = TS.group_of_filtered(ref["stage_sensors"], s0, TS.G_P3)
        last = (n - 1) // TS.G_P3
        print("block of %d: s0 %.4e, filtered per stage %s, their groups %s" % (n, s0, TS.filtered_counts(ref["stage_sensors"], s0), groups))
        in_last.append(n % TS.G_P3 != 0 and any(last in g for g in groups))
    assert any(in_last), in_last


def partition_census(name, part):
    """per stage: (filtered elements in partition groups, in interior groups) of fixture `name` cut into the virtual parts"""
    d = TS.load(name)
    reg, L, Rlut, seg = virtual_tables(d, part)
    ne, nfp, G = int(d["sizes"][0]), int(d["sizes"][2]), T.GROUP[int(d["sizes"][5])]
    marked = np.zeros((ne + G - 1) // G, dtype=bool)
    marked[np.unique((np.ravel(L) // nfp) // G)] = True
    ref = TS.reference(name)
    s0 = TS.scalar(d, "s0")
    out = []
    for s in ref["stage_sensors"]:
        el = np.nonzero(s >= s0)[0]
        out.append((int(marked[el // G].sum()), int((~marked[el // G]).sum())))
    return out, group_census(d, L)


@pytest.mark.parametrize("name", ["ts_p3_n4", "ts_p3_cylinder"])
def test_virtual_partitions_are_sound_inputs(name):
    """the three virtual parts the GPU tests cut: the undivided lockstep is their reference (conditions 3 and 4 hold for it); on the
    cylinder some stage filters an element of a partition group AND an element of an interior group"""
    d = TS.load(name)
    census, (n_part, n_int, _, _) = partition_census(name, grow_parts(d, *TS.PARTS[name]))
    print(name, "filtered per stage (partition groups, interior groups):", census, "groups", n_part, n_int)
    assert n_part > 0
    assert any(a > 0 for a, b in census)
    if name == "ts_p3_cylinder":
        assert n_int > 0 and any(a > 0 and b > 0 for a, b in census)


# ---- the blocks of tests/test_gpu_tris_orders.py: the filter in whole and later groups at every instantiated order ---------------
def group_of(name):
    return T.group_of(bytes(TS.load(name)["based_on"]).decode())


ORDER_BLOCKS = [(TS.BY_ORDER[p], n) for p in sorted(TS.BY_ORDER) for n in (group_of(TS.BY_ORDER[p]), 2 * group_of(TS.BY_ORDER[p]) + 1)]
ORDER_BLOCKS.append(("ts_p2_cfl_local", 129))
LANES = 256  # S2D_T of csrc/simplex2d.hip: a group of NU * G solution points takes ceil(NU G / 256) trips


def second_trip_and_later_groups(name, n):
    """per stage: (filtered elements with a point in the update kernel's second trip, filtered elements beyond group 0)"""
    b, ref = TS.block(n, name)
    nu, g, s0 = int(b["sizes"][1]), group_of(name), TS.scalar(b, "s0")
    out = []
    for s in ref["stage_sensors"]:
        el = np.nonzero(s >= s0)[0]
        out.append((int((((el % g) * nu + nu - 1) >= LANES).sum()), int((el >= g).sum())))
    return out


@pytest.mark.parametrize("name,n", ORDER_BLOCKS)
def test_order_blocks_are_sound_inputs(name, n):
    """conditions 3 and 4 and no NaN (inside TS.block).  Orders whose whole group takes two trips (P2 to P5): some stage filters an
    element of the SECOND trip; every 2 G + 1 block has a stage that filters an element beyond group 0"""
    b, ref = TS.block(n, name)
    nu, g = int(b["sizes"][1]), group_of(name)
    assert int(b["sizes"][0]) == n and ref["bad"] == -1 and all(np.isfinite(u).all() for u in ref["u"])
    census = second_trip_and_later_groups(name, n)
    print("%s, %d elements: s0 %.4e (nearest sensor %.1e away), filtered per stage %s, (second trip, beyond group 0) %s" %
          (name, n, TS.scalar(b, "s0"), TS.closest(ref["stage_sensors"], TS.scalar(b, "s0")), TS.filtered_counts(ref["stage_sensors"], TS.scalar(b, "s0")), census))
    trips = -(-nu * g // LANES)
    assert trips == (1 if nu == 3 else 2)
    if trips == 2:
        assert any(second > 0 for second, _ in census), census
    if n == 2 * g + 1:
        assert any(later > 0 for _, later in census), census


def test_local_time_steps_of_another_group_miss_under_the_filter():
    """ts_p2_cfl_local at 129 elements: filter, local time step and second group together; dt_local rolled by G misses by > 1e-6"""
    b, ref = TS.block(129, "ts_p2_cfl_local")
    assert int(np.ravel(b["dt_type"])[0]) == 2
    rolled = TS.lockstep(b, TS.N_STEPS, dt_map=lambda dtl: np.roll(dtl, 64))
    miss = T.relerr(rolled["u"][-1], ref["u"][-1])
    print("ts_p2_cfl_local, 129 elements: rolled dt_local %.1e" % miss)
    assert miss > 1e-6
