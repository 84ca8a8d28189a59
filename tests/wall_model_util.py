"""The wall model restated in Python from the arrays of a fixture: TEST INFRASTRUCTURE (no GPU, no library).

Three pieces, each in the reference's operation order:
  * input_points  -- eles::calc_wm_upts_dist: one input point per wall-model FACE, the first solution point of the face's own
                     element with the strictly largest minimum over the face's flux points of (pos_fpt - pos_upt) . n_fpt;
  * wall_state    -- bdy_inters::set_boundary_conditions with sol_spec 2: the no-slip wall state the model takes;
  * wall_stress   -- calc_wall_stress: model 1 Werner-Wengle (two branches at Rey = 11.81^2), model 2 the compressible wall
                     function with its Newton loop from utau = 1 until |dutau| <= 1e-6.
wall_flux puts them together: fn . tdA at every flux point of every wall-model face, what the viscous boundary sweep adds to
norm_tconf_fpts there.  tools/capture_wall_model.py checks its fixtures with it before it writes them; the tests check the
library and the host mirror against it.
"""
import json
import math

import numpy as np

ISOTHERM_WALL, ADIABAT_WALL = 8, 9
REY_C = 11.81 * 11.81
NEWTON_CAP = 64  # the library's cap (csrc/wall_model.hpp); the reference has none


def scalar(d, k):
    return float(np.ravel(d[k])[0])


def meta_of(d):
    return json.loads(bytes(d["meta_json"]).decode())


def bdy_block(d):
    """(L (nfpi, n_inters), boundary_id (n_inters)) of the fixture's one boundary-face block"""
    for t in range(3):
        if "bdy%d_L" % t in d:
            return np.asarray(d["bdy%d_L" % t]), np.ravel(d["bdy%d_id" % t])
    raise KeyError("no boundary-face block")


def model_faces(d):
    """indices of the faces of the boundary block whose group is a no-slip wall with use_wm"""
    _, ids = bdy_block(d)
    fl = np.asarray(d["bc_flags"]).reshape(3, -1, order="F")
    return np.array([i for i, g in enumerate(ids) if fl[2, g] and fl[0, g] in (ISOTHERM_WALL, ADIABAT_WALL)], dtype=np.int64)


def input_points(d, first=True):
    """(upt, dist, runner_up) per boundary face (0 on faces without a model).  runner_up: the second-largest dist_min of the face.
    first=False: the LAST point with the largest dist_min (a wrong pick, for the mutation tests)"""
    L, _ = bdy_block(d)
    nfpi, ni = L.shape
    pos_u, pos_f, nrm = d["pos_upts"], d["pos_fpts"], d["norm_fpts"]
    n_upts, n_dims = pos_u.shape[0], pos_u.shape[2]
    n_fpts = pos_f.shape[0]
    upt, dist, second = np.zeros(ni, dtype=np.int32), np.zeros(ni), np.zeros(ni)
    for i in model_faces(d):
        ele = int(L[0, i]) // n_fpts
        dist_max, pick, mins = 0.0, 0, []
        for u in range(n_upts):
            dist_min = 0.0
            for j in range(nfpi):
                f = int(L[j, i]) % n_fpts
                t = 0.0
                for k in range(n_dims):
                    t += (pos_f[f, ele, k] - pos_u[u, ele, k]) * nrm[f, ele, k]
                if j == 0 or t < dist_min:
                    dist_min = t
            mins.append(dist_min)
            if dist_min > dist_max or (not first and dist_min == dist_max):
                dist_max, pick = dist_min, u
        upt[i], dist[i] = pick, dist_max
        second[i] = sorted(mins)[-2]
    return upt, dist, second


def wall_state(flag, bc_par, u_l, gamma, R_ref):
    """sol_spec 2 (src/bdy_inters.cpp:751-762, 826-855): the group's velocity; rho = rho_l; the wall temperature (isothermal) or
    the interior pressure (adiabatic)"""
    nd = len(u_l) - 2
    rho = u_l[0]
    v_l = [u_l[k + 1] / u_l[0] for k in range(nd)]
    v_sq = 0.0
    for k in range(nd):
        v_sq += v_l[k] * v_l[k]
    p_l = (gamma - 1.0) * (u_l[nd + 1] - 0.5 * rho * v_sq)
    v_r = [bc_par[1 + k] for k in range(nd)]
    w_sq = 0.0
    for k in range(nd):
        w_sq += v_r[k] * v_r[k]
    if flag == ISOTHERM_WALL:
        e = rho * (R_ref / (gamma - 1.0) * bc_par[5]) + 0.5 * rho * w_sq
    else:
        e = p_l / (gamma - 1.0) + 0.5 * rho * w_sq
    return [rho] + [rho * v for v in v_r] + [e]


def wall_stress(model, P, u_wm, u_w, dist, n, branch=None):
    """calc_wall_stress (src/wall_model_funcs.cpp:13-119).  P: dict(gamma, prandtl, prandtl_t, Kappa, rt_inf, mu_inf, c_sth, fix_vis).
    Returns (fn, info): info has Rey (model 1) or the |dutau| of every Newton iteration (model 2).
    branch: force model 1's branch ("laminar" / "turbulent"), for the mutation tests"""
    nd = len(n)
    g = P["gamma"]
    rho_wm, rho_w = u_wm[0], u_w[0]
    v_wm_n = 0.0
    for i in range(nd):
        v_wm_n += u_wm[i + 1] / rho_wm * n[i]
    vw, rel = [0.0] * nd, [0.0] * nd
    rel_mag = 0.0
    for i in range(nd):
        par = u_wm[i + 1] / rho_wm - n[i] * v_wm_n
        vw[i] = u_w[i + 1] / rho_w
        rel[i] = par - vw[i]
        rel_mag += rel[i] * rel[i]
    rel_mag = math.sqrt(rel_mag)
    ke_wm = ke_w = 0.0
    for i in range(nd):
        ke_wm += 0.5 * (u_wm[i + 1] / rho_wm) ** 2
        ke_w += 0.5 * vw[i] ** 2
    inte_wm = u_wm[nd + 1] / rho_wm - ke_wm
    inte_w = u_w[nd + 1] / rho_w - ke_w

    def mu_of(inte):
        rt = (g - 1.0) * inte / P["rt_inf"]
        mu = P["mu_inf"] * math.pow(rt, 1.5) * (1 + P["c_sth"]) / (rt + P["c_sth"])
        return mu + P["fix_vis"] * (P["mu_inf"] - mu)

    info = {}
    if model == 1:
        mu_wm = mu_of(inte_wm)
        Rey = rho_wm * rel_mag * dist / mu_wm
        laminar = Rey < REY_C if branch is None else branch == "laminar"
        uplus = math.sqrt(Rey) if laminar else math.pow(8.3, 0.875) * math.pow(Rey, 0.125)
        utau = rel_mag / uplus if rel_mag != 0.0 or uplus != 0.0 else float("nan")
        tw_mag = rho_wm * utau * utau
        if laminar:
            qw = (inte_w - inte_wm) * g * tw_mag / (P["prandtl"] * rel_mag) if rel_mag != 0.0 else float("nan")
        else:
            qw = (inte_w - inte_wm) * g * tw_mag / (P["prandtl_t"] * (rel_mag + utau * 11.81 * (P["prandtl"] / P["prandtl_t"] - 1.0)))
        info["Rey"] = Rey
    elif model == 2:
        B, Cc = math.sqrt(2 * g * inte_w / P["prandtl_t"]), 5.2
        ueq = B * math.asin(rel_mag / B)
        mu_w = mu_of(inte_w)
        utau, steps = 1.0, []
        while True:
            arg = rho_w * dist * utau / mu_w
            lg = math.log(arg) if arg > 0.0 else float("nan")
            dutau = -(utau * (lg / P["Kappa"] + Cc) - ueq) / (1 / P["Kappa"] * (lg + 1.0) + Cc)
            utau += dutau
            steps.append(abs(dutau))
            if not abs(dutau) > 1.0e-6 or len(steps) >= NEWTON_CAP:
                break
        if abs(dutau) > 1.0e-6:
            utau = float("nan")
        tw_mag = rho_w * utau * utau
        qw = 0.0
        info["dutau"] = steps
    else:
        raise ValueError("Wall model not implemented!")
    tw = [tw_mag * rel[i] / rel_mag if rel_mag != 0.0 else float("nan") for i in range(nd)]
    vw_tw = 0.0
    for i in range(nd):
        vw_tw += vw[i] * tw[i]
    return [0.0] + tw + [-qw + vw_tw], info


def phys_of(d):
    P = {k: scalar(d, k) for k in ("gamma", "prandtl", "rt_inf", "mu_inf", "c_sth", "fix_vis")}
    P["prandtl_t"] = scalar(d, "prandtl_t") if "prandtl_t" in d else 0.9
    P["Kappa"] = scalar(d, "Kappa") if "Kappa" in d else 0.41
    return P


def wall_flux(d, u_upts=None, disu_fpts=None, upt=None, dist=None, per_point=False, branch=None):
    """(add, infos): add (n_fpts, n_eles, n_fields) = fn . tdA at the flux points of the wall-model faces, zero elsewhere; infos: one
    dict per model flux point.  u_upts / disu_fpts: the stage's state (default u_init / s0_disu_fpts).
    per_point=True: a WRONG model whose input point is chosen per flux point (the nearest to the face's pick in index + j), and
    branch: a forced Werner-Wengle branch -- both for the mutation tests"""
    meta = meta_of(d)
    model = int(meta["keys"].get("wall_model", 0))
    u_upts = d["u_init"] if u_upts is None else u_upts
    disu_fpts = d["s0_disu_fpts"] if disu_fpts is None else disu_fpts
    if upt is None:
        upt, dist, _ = input_points(d)
    L, ids = bdy_block(d)
    nfpi = L.shape[0]
    n_fpts, n_upts = disu_fpts.shape[0], u_upts.shape[0]
    nd = disu_fpts.shape[2] - 2
    fl = np.asarray(d["bc_flags"]).reshape(3, -1, order="F")
    par = np.asarray(d["bc_params"]).reshape(15, -1, order="F")
    P = phys_of(d)
    R_ref = scalar(d, "bc_R_ref")
    add = np.zeros(disu_fpts.shape)
    infos = []
    for i in model_faces(d):
        g = int(ids[i])
        for j in range(nfpi):
            f, ele = int(L[j, i]) % n_fpts, int(L[j, i]) // n_fpts
            u_l = [float(v) for v in disu_fpts[f, ele, :]]
            n = [float(v) for v in d["norm_fpts"][f, ele, :nd]]
            u_w = wall_state(int(fl[0, g]), par[:, g], u_l, P["gamma"], R_ref)
            p = (int(upt[i]) + j) % n_upts if per_point else int(upt[i])
            u_wm = [float(v) for v in u_upts[p, ele, :]]
            fn, info = wall_stress(model, P, u_wm, u_w, float(dist[i]), n, branch=branch)
            # (inputs: what a stand-alone caller of the library's wall_stress is given for this point)
            info.update(face=int(i), fpt=f, ele=ele, fn=fn, inputs=(model, P, u_wm, u_w, float(dist[i]), n))
            infos.append(info)
            add[f, ele, :] = np.array(fn) * float(d["tdA_fpts"][f, ele])
    return add, infos


def census(d):
    """what tools/capture_wall_model.py asks of a fixture before it writes it: dict(model, n_points, gap (smallest relative
    difference between the largest and second-largest dist_min over the model faces), rey_margin (smallest |Rey / Rey_c - 1|),
    laminar, turbulent, dutau_band (True when a last or next-to-last |dutau| lies in [0.5e-6, 2e-6]), newton_max)"""
    meta = meta_of(d)
    model = int(meta["keys"].get("wall_model", 0))
    upt, dist, second = input_points(d)
    faces = model_faces(d)
    out = dict(model=model, n_faces=len(faces), gap=float(min((dist[i] - second[i]) / dist[i] for i in faces)))
    if not int(scalar(d, "viscous")):
        out.update(n_points=0)
        return out
    _, infos = wall_flux(d, upt=upt, dist=dist)
    out["n_points"] = len(infos)
    if model == 1:
        rey = np.array([q["Rey"] for q in infos])
        out.update(rey_margin=float(np.abs(rey / REY_C - 1.0).min()), laminar=int((rey < REY_C).sum()), turbulent=int((rey >= REY_C).sum()))
    else:
        tail = [s for q in infos for s in q["dutau"][-2:]]
        out.update(dutau_band=any(0.5e-6 <= s <= 2e-6 for s in tail), newton_max=max(len(q["dutau"]) for q in infos),
                   dutau_last=float(max(q["dutau"][-1] for q in infos)))
    return out
