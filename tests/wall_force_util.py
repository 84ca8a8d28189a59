"""What the wall-force tests share (tests/test_wall_force_host.py, tests/test_gpu_wall_force.py): the yardstick, a numpy
restatement in np.longdouble of eles::compute_wall_forces (src/eles.cpp:5704-5990), applied to exactly the arrays the device
gets; the scale of every number it returns; and the bars.

The scale S of a result is the magnitude it would have if nothing cancelled: the SAME formulas, with every subtraction
replaced by the sum of the magnitudes (|p_l| + |p_c_ic| stands for p_l - p_c_ic), every interpolated value replaced by
sum_k |opp(j, k)| |value_k|, every normal component, sine and cosine by its magnitude, and the sums over the points by the sums
of the points' scales.  The bars are derived from it, not measured: the restatement, the device and the reference round the
same sums of at most n_upts terms in different orders, a few ulp of the operands times the number of terms -- about 1e-14 of
S; 1e-12 S leaves two orders of margin.  A bar relative to the value would be wrong where a force is a small difference of
large pressures.
"""
import numpy as np

LD = np.longdouble
BAR = 1e-12

SLIP_WALL, ISOTHERM_WALL, ADIABAT_WALL, SLIP_WALL_DUAL = 6, 8, 9, 11
WALL_FLAGS = (SLIP_WALL, ISOTHERM_WALL, ADIABAT_WALL, SLIP_WALL_DUAL)
LABELS = {SLIP_WALL: "SLIP_WALL", ISOTHERM_WALL: "ISOTHERM_WALL", ADIABAT_WALL: "ADIABAT_WALL", SLIP_WALL_DUAL: "SLIP_WALL_DUAL"}


def wall_forces(face_ele, face_inter, face_flag, opp, weight, detjac, norm, u, grad, phys, ref, scale=False,
                no_dual=False, no_aos=False, third=3.0, slip_viscous=True):
    """eles::compute_wall_forces for one block, in np.longdouble.
    face_ele, face_inter, face_flag (n_faces); opp[l] (n_cubpts, n_upts), weight[l] (n_cubpts) per local face; detjac[f]
    (n_cubpts), norm[f] (n_cubpts, n_dims) per listed face; u (n_upts, n_eles, n_fields); grad (n_upts, n_eles, n_fields,
    n_dims), read on a viscous context only; phys: dict(gamma, rt_inf, mu_inf, c_sth, fix_vis, viscous); ref: dict(rho_c_ic,
    u_c_ic, v_c_ic, w_c_ic, p_c_ic, area_ref).
    -> dict(inv_force (n_dims), vis_force (n_dims), cl, cd, cp, cf (one value per listed face and point, j ascending), first
    (n_faces + 1: where each face's points begin)).  scale=True: the un-cancelled scale of each of these instead.
    The last four arguments move one physics switch each (the tests show the restatement feels every one of them): the dual
    flag read as a plain wall, cos(aos) = 1, the divisor of the trace, no viscous part on slip walls."""
    u = np.asarray(u, dtype=LD)
    nd = u.shape[2] - 2
    viscous = bool(phys["viscous"])
    mag = np.abs if scale else (lambda a: a)
    sub = (lambda a, b: a + b) if scale else (lambda a, b: a - b)
    neg = (lambda a: a) if scale else (lambda a: -a)
    g, rt_inf, mu_inf, c_sth, fix_vis = [LD(phys[k]) for k in ("gamma", "rt_inf", "mu_inf", "c_sth", "fix_vis")]
    rho_c, uc, vc, wc, p_c, area = [LD(ref[k]) for k in ("rho_c_ic", "u_c_ic", "v_c_ic", "w_c_ic", "p_c_ic", "area_ref")]
    aoa = np.arctan2(vc, uc)
    aos = np.arctan2(wc, uc)
    factor = 1 / (LD(0.5) * rho_c * (uc * uc + vc * vc + wc * wc))
    sa, ca = mag(np.sin(aoa)), mag(np.cos(aoa))
    cs = LD(1) if no_aos else mag(np.cos(aos))
    p_c = mag(p_c)

    def lift_drag(F):
        cl = neg(F[0]) * sa + F[1] * ca
        if nd == 2:
            cd = F[0] * ca + F[1] * sa
        else:
            cd = F[0] * ca * cs + F[1] * sa + F[2] * sa * cs
        return cl, cd

    inv_force, vis_force = np.zeros(nd, dtype=LD), np.zeros(nd, dtype=LD)
    cl_sum, cd_sum = LD(0), LD(0)
    cps, cfs, first = [], [], [0]
    for f in range(len(face_ele)):
        ele, l, flag = int(face_ele[f]), int(face_inter[f]), int(face_flag[f])
        O = mag(np.asarray(opp[l], dtype=LD))
        w = np.asarray(weight[l], dtype=LD).ravel()
        dj = np.asarray(detjac[f], dtype=LD).ravel()
        n = mag(np.asarray(norm[f], dtype=LD).reshape((len(w), nd), order="F"))
        ul = O @ mag(u[:, ele, :])                       # (n_cubpts, n_fields)
        rho, mom, E = ul[:, 0], [ul[:, 1 + m] for m in range(nd)], ul[:, nd + 1]
        if flag == SLIP_WALL_DUAL and not no_dual:
            vn = sum(mom[m] * n[:, m] for m in range(nd)) / rho
            mom = [sub(mom[m], vn * n[:, m]) for m in range(nd)]
        v_sq = sum(mom[m] * mom[m] for m in range(nd))
        p = (g - 1) * sub(E, LD(0.5) * v_sq / rho)
        dp_ = sub(p, p_c)
        cp = dp_ * factor
        Finv = [w * dp_ * n[:, m] * dj * factor / area for m in range(nd)]
        cl, cd = lift_drag(Finv)
        cf = np.zeros(len(w), dtype=LD)
        Fvis = [np.zeros(len(w), dtype=LD) for m in range(nd)]
        if viscous and (slip_viscous or flag in (ISOTHERM_WALL, ADIABAT_WALL)):
            gl = np.einsum("jk,kmn->jmn", O, mag(np.asarray(grad, dtype=LD)[:, ele, :, :]))  # (n_cubpts, n_fields, n_dims)
            drho = [gl[:, 0, m] for m in range(nd)]
            dv = [[sub(gl[:, a + 1, m], drho[m] * mom[a] / rho) / rho for m in range(nd)] for a in range(nd)]  # dv[a][m]
            diag = sum(dv[m][m] for m in range(nd)) / LD(third)
            inte = E / rho
            for m in range(nd):
                inte = sub(inte, LD(0.5) * mom[m] * mom[m] / rho / rho)
            rt_ratio = (g - 1) * inte / rt_inf
            mu = mu_inf * rt_ratio ** LD(1.5) * (1 + c_sth) / (rt_ratio + c_sth)
            mu = mu + fix_vis * sub(mu_inf, mu)
            taun = []
            for m in range(nd):
                t = 0
                for k in range(nd):
                    S = LD(0.5) * (dv[m][k] + dv[k][m])
                    if m == k:
                        S = sub(S, diag)
                    t = t + 2 * mu * S * n[:, k]
                taun.append(t)
            tdn = sum(taun[m] * n[:, m] for m in range(nd))
            tautan = [sub(taun[m], tdn * n[:, m]) for m in range(nd)]
            cf = np.sqrt(sum(t * t for t in tautan)) * factor
            Fvis = [neg(w * taun[m] * dj * factor / area) for m in range(nd)]
            a, b = lift_drag(Fvis)
            cl, cd = cl + a, cd + b
        for m in range(nd):
            inv_force[m] += Finv[m].sum()
            vis_force[m] += Fvis[m].sum()
        cl_sum += cl.sum()
        cd_sum += cd.sum()
        cps.append(cp)
        cfs.append(cf)
        first.append(first[-1] + len(w))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=LD)
    return {"inv_force": inv_force, "vis_force": vis_force, "cl": cl_sum, "cd": cd_sum, "cp": cat(cps), "cf": cat(cfs),
            "first": np.array(first)}


def both(*args, **kw):
    """(values, scales) of wall_forces"""
    return wall_forces(*args, **kw), wall_forces(*args, scale=True, **kw)


KEYS = ("inv_force", "vis_force", "cl", "cd", "cp", "cf")


def worst_ratio(got, want, S, keys=KEYS, rel=0.0):
    """max over `keys` of |got - want| / (S + rel |want| / BAR): the miss in units of the scale (the bar is BAR of it); printed
    by the callers before they assert"""
    worst = LD(0)
    for k in keys:
        gk, wk, sk = [np.atleast_1d(np.asarray(a[k], dtype=LD)) for a in (got, want, S)]
        if gk.size == 0:
            continue
        den = sk + LD(rel) / LD(BAR) * np.abs(wk)
        miss = np.abs(gk - wk)
        r = np.where(den > 0, miss / np.where(den > 0, den, 1), np.where(miss > 0, np.inf, 0))
        worst = max(worst, r.max())
    return float(worst)


def assert_at_the_bar(got, want, S, what="", bar=BAR, keys=KEYS):
    """every number of `got` within bar x S of `want`; the worst ratio is printed before it is asserted"""
    r = worst_ratio(got, want, S, keys)
    print("%s: worst |got - want| / S = %.2e (bar %.0e)" % (what, r, bar))
    assert r <= bar, (what, r, bar)
