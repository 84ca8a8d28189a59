"""The integral monitor without a GPU: the numpy restatement of eles::CalcIntegralQuantities (tests/integral_history_util.py)
against the genuine reference, the pairing of state and gradient that the driver's history.plt rows pin
(tests/golden/integral_history/ih_*.npz, tools/capture_integral_history.py), the sampling rule, the capacity count and the host
mirror's keys and refusals.  CPU only: nothing here touches the GPU."""
import json
import os

import numpy as np
import pytest

import hfx
import hfx_host as H
import integral_history_util as IU


@pytest.mark.parametrize("name", IU.INTEGRALS)
def test_restatement_vs_reference(name):
    """the state u_init and the corrected gradient of its residual (the oracle's), against the harness's s0_integral_quantities at
    the project's bar for this monitor: 1e-11 of the largest"""
    d = IU.load(name)
    run = IU.OracleRun(d)
    got = IU.fixture_quantities(d, d["u_init"], run.own_gradient())
    want = np.ravel(d["s0_integral_quantities"])
    err = np.abs(got - want).max() / np.abs(want).max()
    print("%s: %.3e" % (name, err))
    assert err <= 1e-11


@pytest.mark.parametrize("name", IU.IH)
def test_rows_pair_the_new_state_with_the_last_stages_gradient(name):
    """the oracle runs the fixture's steps; at each sampling step the restatement on the new state and the gradient the last stage
    left equals the driver's row within 1e-11 of the row's largest value plus 1e-14 for the printed digits -- and with the
    sampled state's own gradient the enstrophy misses by more than 1e-6: a port that refreshes the gradient fails here"""
    d = IU.load(name)
    ids = np.ravel(d["integral_quantity_ids"])
    rows, diag = [int(v) for v in d["hist_iter"]], d["hist_diag"]
    freq = int(d["monitor_res_freq"][0])
    n_steps = json.loads(bytes(d["meta_json"]).decode())["steps"]
    assert rows == IU.sample_steps(0, n_steps, freq)
    ens = int(np.where(ids == 1)[0][0])
    run = IU.OracleRun(d)
    for s in range(1, max(rows) + 1):
        run.step()
        if s not in rows:
            continue
        row = diag[rows.index(s)]
        got = IU.fixture_quantities(d, run.u, run.grad)
        err = np.abs(got - row).max()
        own = IU.fixture_quantities(d, run.u, run.own_gradient(), ids=[1])[0]
        miss = abs(own - row[ens]) / abs(row[ens])
        print("%s step %d: paired %.3e of the largest, own gradient misses the enstrophy by %.3e" % (name, s, err / np.abs(row).max(), miss))
        assert err <= 1e-11 * np.abs(row).max() + 1e-14 * np.abs(row).max()
        assert miss > 1e-6
    # the euler case has one stage per step: the harness's first gradient and first state are row 1's inputs
    if name == "ih_hex_p2_euler":
        got = IU.fixture_quantities(d, d["u_step0_stage0"], d["s0_grad_disu_upts"])
        assert np.abs(got - diag[0]).max() <= (1e-11 + 1e-14) * np.abs(diag[0]).max()


def test_sampling_rule_and_capacity_count():
    """i_steps == 1 || i_steps % monitor_res_freq == 0 over a range of steps, and the library's count of the samples a call of n
    steps from any i_steps takes (what the loops check before their first launch)"""
    assert [s for s in range(0, 13) if IU.sample_step(s, 4)] == [0, 1, 4, 8, 12]
    assert IU.sample_steps(0, 5, 2) == [1, 2, 4] and IU.sample_steps(0, 4, 3) == [1, 3] and IU.sample_steps(1, 4, 3) == [3]
    for freq in (1, 2, 3, 7, 100, 1000):
        for i_steps in list(range(0, 12)) + [99, 100, 999, 1000]:
            for n in (0, 1, 2, 5, 13, 101, 2001):
                assert hfx.integral_monitor_samples(i_steps, n, freq) == len(IU.sample_steps(i_steps, n, freq)), (i_steps, n, freq)
    with pytest.raises(hfx.HfxError):
        hfx.integral_monitor_samples(0, 3, 0)


def test_monitor_res_freq_of_the_mirror():
    """default 100, 0 means 1000 (src/input.cpp:101,534-535); no monitor until a capacity is given"""
    c = H.Case([3, 3, 3], order=1, amp=0.05)
    assert c.monitor_res_freq() == (100, 0)
    c.set_monitor_res_freq(0, 4)
    assert c.monitor_res_freq() == (1000, 4)
    c.set_monitor_res_freq(7, 2)
    assert c.monitor_res_freq() == (7, 2)
    c.close()


def test_refusals_leave_the_case_as_it_was():
    c = H.Case([3, 3, 3], order=1, amp=0.05)
    c.set_integral_quantities(["kineticenergy", "enstropy"])
    c.set_monitor_res_freq(5, 3)
    with pytest.raises(hfx.HfxError, match="monitor_res_freq"):
        c.set_monitor_res_freq(-1, 3)
    with pytest.raises(hfx.HfxError, match="samples"):
        c.set_monitor_res_freq(5, -2)
    assert c.monitor_res_freq() == (5, 3)
    with pytest.raises(hfx.HfxError, match="integral diagnostic quantity not recognized"):
        c.set_integral_quantities(["kineticenergy", "vorticity"])
    assert c.array("opp_volume_cubpts").shape[0] == 8  # (the cubature of the quantities that stay)
    # not on the device: nothing to sample, count or read
    for call in (c.sample_integral_quantities, c.integral_count, c.read_integral_history):
        with pytest.raises(hfx.HfxError, match="not on the device"):
            call()
    c.close()


def test_new_declarations_are_exported():
    dev = ("hfx_ctx_set_integral_monitor", "hfx_eles_sample_integral_quantities", "hfx_eles_integral_count",
           "hfx_eles_read_integral_history", "hfx_eles_integral_launch", "hfx_integral_monitor_samples", "hfx_time_integral_quantities")
    host = ("hfxh_case_set_monitor_res_freq", "hfxh_case_get_monitor_res_freq", "hfxh_case_sample_integral_quantities",
            "hfxh_case_integral_count", "hfxh_case_read_integral_history")
    declared = hfx.declared_symbols()
    for n in dev:
        assert n in declared and hasattr(hfx.lib(), n), n
    txt = open(os.path.join(hfx.ROOT, "include", "hfx_host.h")).read()
    for n in host:
        assert n + "(" in txt and hasattr(H.lib(), n), n


def test_fixtures_are_small_and_hold_no_program_text():
    for name in IU.IH:
        path = os.path.join(IU.IH_DIR, name + ".npz")
        assert os.path.getsize(path) < (1 << 20), name
        d = IU.load(name)
        assert all(v.dtype.kind in "fiuU" for v in d.values()), name
