"""Every per-step duty of the main loop at once (src/HiFiLES.cpp:194-300) -- TEST INFRASTRUCTURE.

The fixtures tests/golden/full_loop/fl_*.npz (tools/capture_full_loop.py) hold what the genuine driver wrote in ONE run with the
body force, the time averages, history.plt (residual norms, wall forces, integral quantities) and the plot files all switched on,
history and plot at different frequencies.  This module steps the oracle (tests/oracle_py.py) in lockstep with that run and
restates every row through the existing restatements: history_rows_util (residual and force columns, the mass-flux controller),
integral_history_util (integral quantities), plot_rows_util (plot rows, the clock and the time averages), probe_util (probes).

`walk(d)` is the one pass all users share -- the capture tool (conditions before a file is written), tests/test_full_loop_host.py
(the same conditions from the committed files) and tests/test_gpu_full_loop.py (expected values, scales).  Bars are those of
history_rows_util and plot_rows_util; the probes take the bar of a plotted conserved or primitive column, 1e-11 of the field's
largest magnitude over the probes (the same operation: a row of an interpolation operator applied to the state, then the pointwise
field), a field that is zero at every probe exactly.

Triangles (fl_tri_p3_*): the host mirror builds none, so the wall faces and their surface cubature (force_setup) come from the arrays
the reference itself formed and the fixture holds, and the probes sit at plot points, where a probe operator is a row of opp_p; that
gives a check of the probes against the DRIVER's plot rows (probes_against_plot_rows).  The shock filter of fl_tri_p3_shock runs
behind every stage in plot_rows_util.Run; its counts come from tri_shock_util's lockstep (filtered_counts).

Sensitivity numbers (condition 3 of the capture; each must exceed 1e-6, the margin of tests/test_gpu_physics_matrix.py):
  own_gradient_force      per history row: the viscous force formed with the sampled state's OWN gradient, miss of the driver's
                          viscous part relative to that part's largest component
  own_gradient_vorticity  per plot file: the vorticity column so formed, miss relative to the column's largest value
  previous_state_row      per plot file: the row formed from the state one step earlier (same gradient, same averages): the largest
                          miss of any column relative to that column's largest value
  unforced_state          the final state of the run without the body force against the forced run's, of the largest value
  spinup_zero_average     per plot file: the average columns formed with spinup_time 0 instead of the time of step 1: the largest
                          miss of any average column relative to that column's largest value
"""
import functools
import json
import os

import numpy as np

import history_rows_util as HU
import integral_history_util as IU
import plot_rows_util as PU
import probe_util

FL_DIR = os.path.join(PU.GOLDEN, "full_loop")
FL = ["fl_hex_p2_channel", "fl_hex_p2_forced", "fl_quad_p3_walls", "fl_tet_p2_euler", "fl_tri_p3_walls", "fl_tri_p3_shock"]
SENSITIVITY = ["own_gradient_force", "own_gradient_vorticity", "previous_state_row", "unforced_state", "spinup_zero_average"]
MARGIN = 1e-6
PROBE_FREQ = {"fl_hex_p2_channel": 5, "fl_hex_p2_forced": 1, "fl_quad_p3_walls": 1, "fl_tet_p2_euler": 1, "fl_tri_p3_walls": 1,
              "fl_tri_p3_shock": 1}
N_PROBES = 8
TRIANGLES = 0  # (sizes[6] of a triangle block: the class the host mirror does not build)
# the virtual parts of fl_tri_p3_walls in the partitioned loop (test_tris_partition_oracle.grow_parts: weights, seed): parts of 31, 6
# and 3 elements whose 22 partition faces all lie in the first group of 32 -- one partition group, and the ragged group of 8 interior
TRI_PARTS = ([10, 2, 1], 11)


def load(name):
    return dict(np.load(os.path.join(FL_DIR, name + ".npz")))


def meta_of(d):
    return json.loads(bytes(d["meta_json"]).decode())


def forced(d):
    return bool("body_forcing" in d and int(d["body_forcing"][0]))


def _current(u, name, n_dims):
    plane = {"rho_average": 0, "u_average": 1, "v_average": 2, "w_average": 3, "e_average": n_dims + 1}[name]
    return u[:, :, 0] if plane == 0 else u[:, :, plane] / u[:, :, 0]


class _Stages:
    """what HU.ForcedRun steps between two evaluations of the controller: the stages, the clock and the averages of a Run"""

    def __init__(self, run):
        self._run = run

    @property
    def u(self):
        return self._run.u

    def step(self):
        PU.Run.step(self._run)


class Run(PU.Run):
    """plot_rows_util.Run (stages, clock, spinup latch, time averages) with the body force of history_rows_util.ForcedRun in front
    of every step where the driver ran with body_forcing 1; average0 is what the averages would be with spinup_time left at 0"""

    def __init__(self, d, with_force=None):
        import oracle_py as O
        super().__init__(d, PU.names_of(d, "average_fields"))
        self.src, self.ctl = None, None
        if forced(d) if with_force is None else with_force:
            self.ctl = HU.ForcedRun(d, HU.forcing_of(d))
            self.ctl.run = _Stages(self)
            self.src = self.ctl.src
            self.e.src_upts = O.fptr(self.src)
        self.average0 = np.zeros_like(self.average)

    def step(self):
        if self.ctl is not None:
            self.ctl.step()  # (the controller on the state as it stands, then the stages)
        else:
            super().step()
        dt = self.case.params.dt
        a, b = (self.time - dt) / self.time, dt / self.time
        for i, n in enumerate(self.average_names):
            self.average0[:, :, i] = a * self.average0[:, :, i] + b * _current(self.u, n, self.u.shape[2] - 2)

    @property
    def controller_rows(self):
        """(mass_flux, body_force(1)) as evaluated before every step taken so far"""
        return np.array(self.ctl.rows) if self.ctl is not None else np.zeros((0, 2))


def fixture_wall_faces(d):
    """(ele, local face, flag) of every face in a wall group, from the fixture's boundary tables alone: a table entry is
    fpt + n_fpts * ele, the flux points of local face l are l (order + 1) ... (l + 1)(order + 1) - 1 (tests/tri_util.py).  In the
    order of eles::compute_wall_forces (src/eles.cpp:5746-5769): ascending by element, then by local face"""
    import wall_force_util as W
    n_fpts, order = int(d["sizes"][2]), int(d["sizes"][5])
    flags = np.asarray(d["bc_flags"]).reshape(3, -1, order="F")[0]
    faces = []
    for t in range(3):
        if "bdy%d_L" % t in d:
            L, ids = np.asarray(d["bdy%d_L" % t]), np.ravel(d["bdy%d_id" % t])
            for i in range(L.shape[1]):
                ele, l = int(L[0, i]) // n_fpts, (int(L[0, i]) % n_fpts) // (order + 1)
                assert np.array_equal(L[:, i] // n_fpts, np.full(L.shape[0], ele)) and int(L[-1, i]) % n_fpts == (l + 1) * (order + 1) - 1
                if int(flags[ids[i]]) in W.WALL_FLAGS:
                    faces.append((ele, l, int(flags[ids[i]])))
    faces.sort()
    return tuple(np.array(c, dtype=np.int32) for c in zip(*faces))


def fixture_device_arrays(d):
    """test_wall_force_host.device_arrays from the arrays the reference itself formed (eles_tris::set_inters_cubpts,
    eles::set_opp_inters_cubpts, set_transforms_inters_cubpts) and the harness dumped into the fixture, in the mirror's shapes:
    per local face opp (n_cubpts, n_upts), weight (n_cubpts), detjac (n_cubpts, n_eles), norm (n_cubpts, n_eles, n_dims)"""
    ele, inter, flag = fixture_wall_faces(d)
    n_inters = len([k for k in d if k.startswith("opp_inters_cubpts_")])
    opp = [np.asarray(d["opp_inters_cubpts_%d" % l]) for l in range(n_inters)]
    weight = [np.ravel(d["weight_inters_cubpts_%d" % l]) for l in range(n_inters)]
    detjac = [np.asarray(d["inter_detjac_inters_cubpts_%d" % l])[:, e] for e, l in zip(ele, inter)]
    norm = [np.asarray(d["norm_inters_cubpts_%d" % l])[:, e, :] for e, l in zip(ele, inter)]
    return dict(face_ele=ele, face_inter=inter, face_flag=flag, opp=opp, weight=weight, detjac=detjac, norm=norm)


def force_setup(d):
    """the wall faces of the fixture (no device): dict(A, phys, ref), or None without calc_force.  From the host mirror, except on
    triangles, which the mirror does not build: there from the surface cubature the fixture holds"""
    if not int(d["calc_force"][0]):
        return None
    if int(d["sizes"][6]) == TRIANGLES:
        phys = {k: PU.scalar(d, k) for k in ("gamma", "rt_inf", "mu_inf", "c_sth", "fix_vis")}
        phys["viscous"] = int(PU.scalar(d, "viscous"))
        ref = {k: PU.scalar(d, k) for k in ("rho_c_ic", "u_c_ic", "v_c_ic", "w_c_ic", "p_c_ic", "area_ref")}
        return dict(A=fixture_device_arrays(d), phys=phys, ref=ref)
    from test_wall_force_host import device_arrays, mirror_case, phys_of, ref_of
    mc, _ = mirror_case(d)
    out = dict(A=device_arrays(mc), phys=phys_of(mc), ref=ref_of(mc))
    mc.close()
    return out


def rel_columns(got, want):
    """per column the largest difference over the column's largest magnitude in `want`"""
    return np.abs(got - want).max(axis=0) / np.maximum(np.abs(want).max(axis=0), 1e-300)


def walk(d):
    """the oracle in lockstep with the fixture's driver: per step the state, per history row and plot file the restated columns,
    their scales, their miss of the driver's in bars, and the sensitivity numbers of condition 3"""
    import wall_force_util as W
    meta = meta_of(d)
    steps = meta["steps"]
    n_fields, n_dims = int(d["sizes"][3]), int(d["sizes"][4])
    hist_iter, plot_iter = [int(v) for v in d["hist_iter"]], [int(v) for v in d["plot_iter"]]
    diag, avg = PU.names_of(d, "diagnostic_fields"), PU.names_of(d, "average_fields")
    F = force_setup(d)
    n_diag = d["hist_diag"].shape[1]
    run = Run(d)
    out = dict(states=[], hist=[], plot=[], sens={k: [] for k in SENSITIVITY}, detjac=run.case.arr["detjac_upts"].copy(order="F"))
    for s in range(1, steps + 1):
        prev = run.u.copy(order="F")
        run.step()
        out["states"].append(run.u.copy(order="F"))
        if s in hist_iter:
            k = hist_iter.index(s)
            row = dict(step=s, res=HU.residual_columns(d, run))
            row["res_bars"] = HU.log_miss(row["res"], d["hist_res"][k])
            if F is not None:
                grad = run.grad if F["phys"]["viscous"] else None
                row["force"], row["force_scale"] = HU.force_columns(W, F["A"], F["phys"], F["ref"], run.u, grad)
                row["force_bars"] = HU.value_miss(row["force"], d["hist_force"][k], row["force_scale"])
                # (for the record, not a bar: the same miss in units of 1e-11 of the row's own size; the channel's wall forces cancel
                # to 1e-3 of their un-cancelled scale and the restatement itself comes to 0.99 of that unit)
                row["force_row_size"] = HU.value_miss(row["force"], d["hist_force"][k], np.abs(d["hist_force"][k]).max())
                if F["phys"]["viscous"]:
                    inv = HU.force_columns(W, F["A"], dict(F["phys"], viscous=0), F["ref"], run.u, None)[0]
                    own = HU.force_columns(W, F["A"], F["phys"], F["ref"], run.u, run.own_gradient())[0]
                    row_vis = (d["hist_force"][k] - inv)[:n_dims]
                    out["sens"]["own_gradient_force"].append(float(np.abs((own - inv)[:n_dims] - row_vis).max() / np.abs(row_vis).max()))
            if n_diag:
                row["diag"] = IU.fixture_quantities(d, run.u, run.grad)
                row["diag_bars"] = HU.value_miss(row["diag"], d["hist_diag"][k], np.abs(d["hist_diag"][k]).max())
            out["hist"].append(row)
        if s in plot_iter:
            k = plot_iter.index(s)
            drv = d["plot_rows"][k][:, n_dims:]
            got, scales = PU.fixture_fields(d, run)
            snap = dict(step=s, rows=PU.rows_of(got), scales=scales)
            snap["bars"] = PU.miss(snap["rows"], drv, scales)
            out["plot"].append(snap)
            na = len(avg)
            if "vorticity" in diag:
                col = n_fields + na + diag.index("vorticity")
                own = PU.rows_of(PU.fixture_fields(d, run, grad=run.own_gradient())[0])
                out["sens"]["own_gradient_vorticity"].append(float(rel_columns(own, drv)[col]))
            grad = run.grad if PU.reads_gradient(diag) else None
            before = PU.fields(diag, d["opp_p"], prev, grad, PU.scalar(d, "gamma"), average=run.average if na else None,
                               sensor=run.sensor)[0]
            out["sens"]["previous_state_row"].append(float(rel_columns(PU.rows_of(before), drv).max()))
            if na:
                zero = np.einsum("jk,kif->jif", d["opp_p"], run.average0)
                out["sens"]["spinup_zero_average"].append(float(rel_columns(PU.rows_of(zero), drv[:, n_fields:n_fields + na]).max()))
    out["average"] = run.average.copy(order="F")
    out["controller"] = run.controller_rows
    out["time"], out["spinup_time"], out["dt"] = run.time, run.spinup_time, run.case.params.dt
    if run.ctl is not None:
        free = Run(d, with_force=False)
        for _ in range(steps):
            free.step()
        out["unforced"] = free.u.copy(order="F")
        out["sens"]["unforced_state"].append(float(np.abs(free.u - run.u).max() / np.abs(run.u).max()))
    if shock(d):
        # the harness does not dump a triangle run with shock_cap 1 (tools/capture_tris_shock.py): it ran without the filter, and
        # the run without the filter is what its last state is tied to
        free = Run(dict(d, shock_cap=np.array([0], dtype=np.int32)))
        for _ in range(steps):
            free.step()
        out["unfiltered"] = free.u.copy(order="F")
    return out


def shock(d):
    return bool("shock_cap" in d and int(np.ravel(d["shock_cap"])[0]))


def harness_state(d, w):
    """the lockstep state the harness's own last state is tied to: of the run without the body force or without the shock filter
    where the harness ran without it, else the run's"""
    return w["unforced"] if forced(d) else w["unfiltered"] if shock(d) else w["states"][-1]


def filtered_counts(d):
    """the shock filter of a fixture with shock_cap 1 through tri_shock_util's lockstep: (per stage (n_steps, n_stages) the number
    of filtered elements, per step the number of elements some stage of the step filtered, the smallest distance of a sensor value of
    any stage from s0 relative to s0)"""
    import tri_shock_util as TS
    steps, n_stages, s0 = meta_of(d)["steps"], int(d["sizes"][7]), TS.scalar(d, "s0")
    sens = TS.lockstep(d, steps)["stage_sensors"]
    per_stage = np.array(TS.filtered_counts(sens, s0)).reshape(steps, n_stages)
    per_step = np.array([int((sens[s * n_stages:(s + 1) * n_stages] >= s0).any(axis=0).sum()) for s in range(steps)])
    return per_stage, per_step, TS.closest(sens, s0)


def worst_bars(w):
    """the largest miss of any restated column of any row the driver wrote, in bars"""
    worst = 0.0
    for row in w["hist"]:
        worst = max([worst] + [row[k] for k in ("res_bars", "force_bars", "diag_bars") if k in row])
    for snap in w["plot"]:
        worst = max(worst, float(snap["bars"].max()))
    return worst


def controller_tie(d, w):
    """the lockstep controller against the lines the driver printed before every step (8 digits; src/eles.cpp:5430): the largest
    miss of the mass flux and the force relative to the column's largest value"""
    drv = d["driver_controller"]
    return float((np.abs(w["controller"] - drv[:, 3:]).max(axis=0) / np.abs(drv[:, 3:]).max(axis=0)).max())


@functools.lru_cache(maxsize=None)
def reference(name):
    """(fixture, walk(fixture)): computed once per session, left unchanged"""
    d = load(name)
    return d, walk(d)


# ---- the sampling schedule ---------------------------------------------------------------------------------------------------
def schedule(d):
    """per step 1..n: (history row?, plot file?, last stage call by call on a plan that keeps the gradient on chip?)"""
    freq, pf = int(d["monitor_res_freq"][0]), int(d["plot_freq"][0])
    reads = PU.reads_gradient(PU.names_of(d, "diagnostic_fields"))
    grad_hist = bool(int(d["calc_force"][0]) and IU.scalar(d, "viscous")) or any(int(i) for i in np.ravel(d["integral_quantity_ids"]))
    out = []
    for s in range(1, meta_of(d)["steps"] + 1):
        h, p = IU.sample_step(s, freq), s % pf == 0
        out.append((h, p, (h and grad_hist) or (p and reads)))
    return out


def cuts(n, parts):
    """every way to cut n steps into `parts` calls of at least one step"""
    if parts == 1:
        return [[n]]
    return [[k] + rest for k in range(1, n - parts + 2) for rest in cuts(n - k, parts - 1)]


# ---- probes ------------------------------------------------------------------------------------------------------------------
PROBE_PERM = [5, 2, 7, 0, 3, 6, 1, 4]


def probe_mirror(d):
    """the host mirror of the fixture's element class on the fixture's mesh (no device): an hfx_host.Case or an hfx_host.Simplex"""
    import bdy_util
    import hfx_host as H
    et = int(d["sizes"][6])
    if et in (1, 4):
        return bdy_util.case_from_fixture(d, loc_1d_upts=d["loc_upts"][0, :meta_of(d)["keys"]["order"] + 1])[0]
    return H.Simplex(et, meta_of(d)["keys"]["order"], d["shape"])


@functools.lru_cache(maxsize=None)
def probes(name):
    """8 fixed physical points -- the images of fixed reference locations in fixed elements -- located by the mirror:
    dict(pos (n_dims, 8), ele (8), opp (n_upts, 8), perm: the scrambled order of registration, names: the probe fields)"""
    d = load(name)
    n_dims, n_eles, et = int(d["sizes"][4]), int(d["sizes"][0]), int(d["sizes"][6])
    ele = np.array([0, 1, n_eles // 3, n_eles // 2, n_eles // 2, (2 * n_eles) // 3, n_eles - 2, n_eles - 1], dtype=np.int32)
    if et == TRIANGLES:
        # no mirror: the probes sit at plot points strictly inside their elements, dealt in turn over the elements, and a probe's
        # operator is the row of opp_p of its plot point (the nodal basis there).  pos: as the driver printed it in its plot file
        loc = np.asarray(d["loc_ppts"])
        inside = np.nonzero((loc[0] > -1 + 1e-6) & (loc[1] > -1 + 1e-6) & (loc[0] + loc[1] < -1e-6))[0]
        assert len(inside) >= 2, "p_res %d has no two plot points strictly inside a triangle" % int(d["p_res"][0])
        ppt = inside[np.arange(N_PROBES) % len(inside)]
        assert len(set(zip(ele.tolist(), ppt.tolist()))) == N_PROBES
        pos = d["plot_rows"][0][ele * loc.shape[1] + ppt, :n_dims].T.copy(order="F")
        return dict(pos=pos, ele=ele, opp=np.asarray(d["opp_p"])[ppt, :].T.copy(order="F"), perm=np.array(PROBE_PERM),
                    names=probe_util.field_names(n_dims), ppt=ppt)
    m = probe_mirror(d)
    loc = probe_util.random_interior_locs(et, N_PROBES, 20261020)
    pos = m.calc_pos(ele, loc)
    p2c, found = m.locate(pos)
    assert np.array_equal(p2c, ele), (p2c, ele)
    opp = m.opp_probe(found)
    m.close()
    return dict(pos=pos, ele=p2c, opp=opp, perm=np.array(PROBE_PERM), names=probe_util.field_names(n_dims))


def expected_probes(name):
    """(steps, values (n_fields, 8, n_samples)): opp_probe^T . the oracle's lockstep state of every step with step % probe_freq == 0"""
    d, w = reference(name)
    P = probes(name)
    steps = [s for s in range(1, meta_of(d)["steps"] + 1) if s % PROBE_FREQ[name] == 0]
    vals = [probe_util.probe_fields(probe_util.interpolate(P["opp"], P["ele"], w["states"][s - 1]), P["names"], PU.scalar(d, "gamma"))
            for s in steps]
    return steps, np.stack(vals, axis=2)


def probes_against_plot_rows(name, steps, values):
    """probes registered at plot points (triangles) against the DRIVER's plot files, independent of the lockstep: at every step that
    both sample, the conserved state of the probe samples `values` (n_fields, 8, n_samples; taken at `steps`) against the file's
    rows at those plot points, the largest miss in units of the plot bar (plot_rows_util.miss).  None where the probes sit elsewhere"""
    d, w = reference(name)
    P = probes(name)
    if "ppt" not in P:
        return None
    nd, nf, n_ppts = int(d["sizes"][4]), int(d["sizes"][3]), d["opp_p"].shape[0]
    assert nd == 2
    at = {n: i for i, n in enumerate(P["names"])}
    worst, steps = None, list(steps)
    for k, s in enumerate(int(v) for v in d["plot_iter"]):
        if s in steps:
            v = values[:, :, steps.index(s)]
            rho = v[at["rho"]]
            cons = np.stack([rho, rho * v[at["u"]], rho * v[at["v"]], rho * v[at["specific_total_energy"]]], axis=1)
            rows = d["plot_rows"][k][P["ele"] * n_ppts + P["ppt"], nd:nd + nf]
            worst = max(worst or 0.0, float(PU.miss(cons, rows, w["plot"][k]["scales"][:nf]).max()))
    return worst


def probe_miss(got, want):
    """per field the largest miss over all probes and samples, relative to the field's largest magnitude (exact where that is 0)"""
    return probe_util.field_rel(got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1))
