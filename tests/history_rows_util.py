"""The residual and force columns of history.plt restated in numpy -- TEST INFRASTRUCTURE.

eles::compute_res_upts (src/eles.cpp:5045-5074): per field the max |r|, the sum |r| or the sum r^2 over the solution points of
r = div_tconf_upts(0) / detjac_upts - src_upts.  output::CalcNormResidual (src/output.cpp:2166-2248): max or sum over the element
classes and ranks, then sum, sum / n_upts or sqrt(sum) / n_upts -- the reference DOES divide the L2 sum's root by n_upts.
HistoryOutput (src/output.cpp:2375-2402) writes log10 of each norm, with calc_force the total force per dimension, CL and CD, the
integral quantities, and the time (x time_ref on a viscous case), after step 1 and every monitor_res_freq-th step
(src/HiFiLES.cpp:247-266).

The bar of a residual column: 1e-11 relative on the norm, the project's bar for rows of history.plt -- log10(1 + 1e-11) on the
printed value -- plus 1e-14 x max(1, |value|) for the 15 digits the file prints.
"""
import json
import os

import numpy as np

import integral_history_util as IU

GOLDEN = IU.GOLDEN
HR_DIR = os.path.join(GOLDEN, "history_rows")
WF_DIR = os.path.join(GOLDEN, "wall_force")
HR = ["hr_hex_p2_rk45", "hr_hex_p2_euler", "hr_hex_p2_norm0", "hr_hex_p2_norm1", "hr_quad_p3_walls", "hr_hex_p2_walls", "hr_tet_p2_rk45",
      "hr_hex_p2_forced"]
WF = ["wf_hex_p2_a", "wf_hex_p2_b", "wf_quad_p3_a", "wf_quad_p3_b", "wf_quad_p3_inviscid"]
LOG_BAR = float(np.log10(1.0 + 1e-11))


def load(name):
    return dict(np.load(os.path.join(WF_DIR if name.startswith("wf_") else HR_DIR, name + ".npz")))


def meta_of(d):
    return json.loads(bytes(d["meta_json"]).decode())


def res_upts(norm_type, div_tconf_upts, detjac_upts, src_upts=None):
    """eles::compute_res_upts of every field: (n_fields)"""
    r = np.asarray(div_tconf_upts, dtype=np.float64) / np.asarray(detjac_upts, dtype=np.float64)[:, :, None]
    if src_upts is not None:
        r = r - src_upts
    if norm_type == 0:
        return np.abs(r).max(axis=(0, 1))
    if norm_type == 1:
        return np.abs(r).sum(axis=(0, 1))
    if norm_type == 2:
        return (r * r).sum(axis=(0, 1))
    raise ValueError("norm_type not recognized")


def norm_residual(norm_type, sums, n_upts, root_inside=False):
    """the finish of output::CalcNormResidual; root_inside: sqrt(sum / n_upts), what the reference does NOT compute"""
    sums = np.asarray(sums, dtype=np.float64)
    if norm_type == 0:
        return sums
    if norm_type == 1:
        return sums / n_upts
    return np.sqrt(sums / n_upts) if root_inside else np.sqrt(sums) / n_upts


def log_miss(got_log10, want):
    """|got - want| / bar of log10 columns: <= 1 passes"""
    got_log10, want = np.asarray(got_log10, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got_log10 - want) / (LOG_BAR + 1e-14 * np.maximum(1.0, np.abs(want)))).max())


def residual_columns(d, run, norm_type=None, root_inside=False):
    """log10 of the norms after the step `run` (an IU.OracleRun or a ForcedRun) has just taken"""
    nt = int(d["res_norm_type"][0]) if norm_type is None else norm_type
    a = run.case.arr
    sums = res_upts(nt, a["div_tconf_upts"], a["detjac_upts"], getattr(run, "src", None))
    return np.log10(norm_residual(nt, sums, a["detjac_upts"].size, root_inside))


# the reference hard-codes the inflow area and the target mass flux of its body force (src/eles.cpp:5393-5395)
FORCING_AREA = FORCING_MDOT0 = 9.162


def forcing_of(d):
    """the inflow faces the reference's rule selects on the fixture's mesh and their surface cubature, from the host mirror (no
    device): a test_gpu_body_force.Forcing with the reference's hard-coded area"""
    import bdy_util
    from test_gpu_body_force import Forcing
    kk = meta_of(d)["keys"]
    c, _ = bdy_util.case_from_fixture(d, body_forcing=1, loc_1d_upts=d["loc_upts"][0, :kk["order"] + 1])
    ele, inter = (a.tolist() for a in c.inflow_faces())
    opp = [c.array("opp_inters_cubpts_%d" % l) for l in range(6)]
    wgt = [c.array("weight_inters_cubpts_%d" % l) for l in range(6)]
    dj = [c.array("inter_detjac_inters_cubpts_%d" % l) for l in range(6)]
    detjac = [dj[l][:, e].copy() for e, l in zip(ele, inter)]
    c.close()
    return Forcing(ele, inter, opp, wgt, detjac, FORCING_AREA)


class ForcedRun:
    """the oracle in lockstep with the mass-flux controller (src/eles.cpp:5340-5428 restated in test_gpu_body_force.restatement):
    before every step the force of the state as it stands is added to src_upts, which the oracle's stages subtract"""

    def __init__(self, d, forcing):
        import oracle_py as O
        self.run, self.F = IU.OracleRun(d), forcing
        self.src = np.zeros(self.run.u.shape, order="F")
        self.run.e.src_upts = O.fptr(self.src)
        self.mdot_old, self.dt, self.rows = FORCING_MDOT0, IU.scalar(d, "dt"), []
        self.case = self.run.case

    def step(self):
        from test_gpu_body_force import restatement
        r = restatement(self.F, self.run.u, FORCING_MDOT0, self.mdot_old, self.dt)
        self.src[:, :, 1] += r["bf1"]
        self.src[:, :, 4] += r["bf4"]
        self.mdot_old = r["mass_flux"]
        self.rows.append((r["mass_flux"], r["bf1"]))
        self.run.step()

    @property
    def u(self):
        return self.run.u

    @property
    def grad(self):
        return self.run.grad


def oracle_run(d):
    """the run that reproduces the fixture's driver: forced where the driver ran with body_forcing 1"""
    return ForcedRun(d, forcing_of(d)) if "body_forcing" in d and int(d["body_forcing"][0]) else IU.OracleRun(d)


def value_miss(got, want, scale):
    """|got - want| / (1e-11 scale + 1e-14 max(1, |want|)): the bar of the force and diagnostic columns"""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    return float((np.abs(got - want) / (1e-11 * np.asarray(scale, dtype=np.float64) + 1e-14 * np.maximum(1.0, np.abs(want)))).max())


def force_columns(W, A, phys, ref, u, grad):
    """(values, scales) of the force columns F (n_dims), CL, CD: wall_force_util's restatement, inviscid + viscous"""
    args = (A["face_ele"], A["face_inter"], A["face_flag"], A["opp"], A["weight"], A["detjac"], A["norm"], u, grad, phys, ref)
    v, S = W.both(*args)
    cat = lambda r: np.concatenate([np.asarray(r["inv_force"] + r["vis_force"], dtype=np.float64), [float(r["cl"])], [float(r["cd"])]])
    return cat(v), cat(S)
