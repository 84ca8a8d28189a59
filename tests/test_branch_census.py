"""Which branch of the pointwise face physics every face point of the transonic fixtures takes.

Plain numpy on the fixtures' own face states (`s0_disu_fpts`, `norm_fpts`, the face tables, the boundary records): the
wave-speed estimates of HLLC (S_L, S_*, S_R), the clipped wave speeds of RoeM (b1, b2) and the switches of the boundary
ghost states (normal Mach number, sign of u.n) are written out below as the reference states them (src/inters.cpp:327-532,
src/bdy_inters.cpp:404-468, :475-590, :863-960).  The library is not imported: these are conditions on the INPUTS of the
tests that run the fixtures through the oracle and the kernels (test_oracle_vs_golden.py, test_gpu_*.py) -- a branch that
no fixture point takes is a branch whose copies in the kernels nothing checks.

HLLC and RoeM are continuous across their switches (at S_L = 0 the star-state flux equals the left flux, and so on; a
clipped wave speed is a max / min), so a point that rounding moves across a switch changes the flux by rounding only: no
margin is asked there.  The boundary ghost states are NOT continuous across theirs (sub_out_simp jumps from the back
pressure to the interior's, "char" swaps whole Riemann invariants), so every boundary point has to stay clear of every
switch by 1e-6 of the sound speed -- seven orders above what differently rounded arithmetic can move it.

The same argument for what does not depend on the data: the run-wide switches (Riemann solver, Sutherland's law, the LDG
penalty and switch, viscous or not) on every element class, every boundary type in 2-D and in 3-D with its viscous sweep, and
the branches of the total-pressure ramp at the ramp counter of every stored step (test_switch_table,
test_every_boundary_type_in_each_dimension, test_ramp_takes_every_branch).  tests/test_gpu_physics_matrix.py runs the same
switches through every kernel family against the oracle, which is trusted where these fixtures pin it.
"""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HLLC = ["hex_p2_transonic", "quad_p3_transonic", "tet_p2_transonic", "pri_p2_transonic", "hex_p1_bdy_supersonic",
        "hex_p2_bdy_transonic"]
ROEM = ["hex_p2_transonic_roem"]
# RoeM on the other element classes: each has its own face kernels, each sees both clips
ROEM_CLASSES = ["quad_p3_roem_sutherland", "tet_p2_roem_sutherland", "pri_p2_roem_sutherland"]
SUTHERLAND = {"quad_p3_roem_sutherland": "u_step2_stage3", "tet_p2_roem_sutherland": "u_step0_stage3",
              "pri_p2_roem_sutherland": "u_step1_stage3"}  # fixture -> the state that enters its last stored stage
BDY = ["hex_p1_bdy_supersonic", "hex_p2_bdy_transonic"]
BDY2 = ["quad_p3_bdy_supersonic", "quad_p3_bdy_transonic", "quad_p3_ramp_clamp"]
SUB_OUT_SIMP, SUB_IN_CHAR, CHAR = 1, 2, 10  # bc flags of the boundary records (include/hfx.h)
# hfx_bc_flag by name (include/hfx.h; the reference's bc type names)
BC_FLAGS = {"sub_in_simp": 0, "sub_out_simp": 1, "sub_in_char": 2, "sub_out_char": 3, "sup_in": 4, "sup_out": 5, "slip_wall": 6,
            "cyclic": 7, "isotherm_wall": 8, "adiabat_wall": 9, "char": 10, "slip_wall_dual": 11}
ELE_CLASSES = {1: "quad", 4: "hex", 2: "tet", 3: "prism"}  # sizes[6], the reference's ele_type
MIN_POINTS = 8
MARGIN = 1e-6


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def face_points(d, table):
    """conserved state and unit normal at the flux points a face table lists (offsets into the field-0 plane)"""
    nd = d["norm_fpts"].shape[2]
    # a fixture that holds states only: the reference's own extrapolation operator on its initial state
    u = d["s0_disu_fpts"] if "s0_disu_fpts" in d else np.einsum("fu,uek->fek", d["opp_0"], d["u_init"])
    plane = u.shape[0] * u.shape[1]
    idx = np.ravel(table, order="F")
    return u.reshape(plane, nd + 2, order="F")[idx], idx


def primitives(gamma, u, n):
    nd = n.shape[1]
    rho = u[:, 0]
    v = u[:, 1:nd + 1] / rho[:, None]
    vn = (v * n).sum(axis=1)
    p = (gamma - 1.0) * (u[:, nd + 1] - 0.5 * rho * (v * v).sum(axis=1))
    h = (u[:, nd + 1] + p) / rho
    return rho, v, vn, p, h


def interior_pairs(d):
    """left state, right state and the left element's normal of every interior flux-point pair"""
    nd = d["norm_fpts"].shape[2]
    norm = d["norm_fpts"].reshape(-1, nd, order="F")
    ul, ur, n = [], [], []
    for t in range(3):
        if "int%d_L" % t in d:
            a, idx = face_points(d, d["int%d_L" % t])
            b, _ = face_points(d, d["int%d_R" % t])
            ul.append(a); ur.append(b); n.append(norm[idx])
    return np.concatenate(ul), np.concatenate(ur), np.concatenate(n)


def boundary_points(d):
    """interior state, normal and boundary record index of every boundary flux point"""
    nd = d["norm_fpts"].shape[2]
    norm = d["norm_fpts"].reshape(-1, nd, order="F")
    ul, n, bc = [], [], []
    for t in range(3):
        if "bdy%d_L" % t in d:
            L = d["bdy%d_L" % t]
            a, idx = face_points(d, L)
            ul.append(a); n.append(norm[idx])
            bc.append(np.repeat(np.ravel(d["bdy%d_id" % t]), L.shape[0]))
    return np.concatenate(ul), np.concatenate(n), np.concatenate(bc)


def hllc_census(d):
    gamma = float(np.ravel(d["gamma"])[0])
    ul, ur, n = interior_pairs(d)
    rl, _, vnl, pl, hl = primitives(gamma, ul, n)
    rr, _, vnr, pr, hr = primitives(gamma, ur, n)
    sq = np.sqrt(rr / rl)
    rrho = 1.0 / (sq + 1.0)
    vn_m = rrho * (vnl + sq * vnr)
    h_m = rrho * (hl + sq * hr)
    a_m = np.sqrt((gamma - 1.0) * (h_m - 0.5 * vn_m * vn_m))
    S_R, S_L = vn_m + a_m, vn_m - a_m
    S_star = (pr - pl + rl * vnl * (S_L - vnl) - rr * vnr * (S_R - vnr)) / (rl * (S_L - vnl) - rr * (S_R - vnr))
    left = S_L >= 0
    star_l = ~left & (S_star >= 0)
    star_r = ~left & ~star_l & (S_R >= 0)
    right = ~left & ~star_l & ~star_r
    return dict(left=int(left.sum()), star_left=int(star_l.sum()), star_right=int(star_r.sum()), right=int(right.sum()))


def roem_census(d):
    gamma = float(np.ravel(d["gamma"])[0])
    ul, ur, n = interior_pairs(d)
    rl, vl, vnl, pl, hl = primitives(gamma, ul, n)
    rr, vr, vnr, pr, hr = primitives(gamma, ur, n)
    sq = np.sqrt(rr / rl)
    rrho = 1.0 / (1.0 + sq)
    ratr = sq * rrho
    ha = hl * rrho + hr * ratr
    va = vl * rrho[:, None] + vr * ratr[:, None]
    va_n = (va * n).sum(axis=1)
    aa = np.sqrt((gamma - 1.0) * (ha - 0.5 * (va * va).sum(axis=1)))
    b1 = np.maximum(va_n + aa, vnr + aa)  # b1 = max(0, this)
    b2 = np.minimum(va_n - aa, vnl - aa)  # b2 = min(0, this)
    return dict(b1_clipped=int((b1 < 0).sum()), b2_clipped=int((b2 > 0).sum()), unclipped=int(((b1 >= 0) & (b2 <= 0)).sum()))


def bdy_census(d):
    """-> {branch: count}, the smallest distance of any point from a switch (relative to the sound speed)"""
    gamma = float(np.ravel(d["gamma"])[0])
    gm1 = gamma - 1.0
    R_ref = float(np.ravel(d["bc_R_ref"])[0])
    flags = d["bc_flags"].reshape(3, -1, order="F")[0]
    par = d["bc_params"].reshape(15, -1, order="F")
    ul, n, bc = boundary_points(d)
    rho, _, vn, p, _ = primitives(gamma, ul, n)
    c = np.sqrt(gamma * p / rho)
    machn = np.abs(vn) / c
    fl = flags[bc]
    out, gap = {}, np.inf

    m = fl == SUB_OUT_SIMP
    out["sub_out_simp reverse flow"] = int((m & (vn < 0)).sum())
    out["sub_out_simp machn >= 1"] = int((m & (vn >= 0) & (machn >= 1)).sum())
    out["sub_out_simp subsonic"] = int((m & (vn >= 0) & (machn < 1)).sum())
    # the Mach switch is only consulted when the flow leaves
    for g in (machn[m], np.abs(machn[m & (vn >= 0)] - 1.0)):
        gap = min(gap, g.min()) if g.size else gap

    m = fl == CHAR
    sup = machn >= 1
    out["char supersonic inflow"] = int((m & sup & (vn < 0)).sum())
    out["char supersonic outflow"] = int((m & sup & (vn >= 0)).sum())
    out["char subsonic inflow"] = int((m & ~sup & (vn < 0)).sum())
    out["char subsonic outflow"] = int((m & ~sup & (vn >= 0)).sum())
    for g in (machn[m], np.abs(machn[m] - 1.0)):
        gap = min(gap, g.min()) if g.size else gap

    m = fl == SUB_IN_CHAR
    if m.any():
        # the ghost speed from the total temperature and the outgoing invariant: root of a quadratic
        T0 = par[7][bc][m]
        ramped = d["bc_flags"].reshape(3, -1, order="F")[1][bc][m] != 0
        if ramped.any():  # a ramped inlet: the total temperature of the fixture's first step (src/bdy_inters.cpp:482-504)
            counter = int(np.ravel(d["ramp_counter"])[0])
            T_l = p[m] / (rho[m] * R_ref)
            T0 = np.where(ramped, [ramp_totals(par[:, b], counter, t, q)[1] for b, t, q in zip(bc[m], T_l, p[m])], T0)
        dirn = par[8:8 + n.shape[1]][:, bc].T[m]
        alpha = (n[m] * dirn).sum(axis=1)
        R_plus = vn[m] + 2.0 * c[m] / gm1
        c0sq = gamma * R_ref * T0
        qa = 1.0 + 0.5 * gm1 * alpha * alpha
        qb = -gm1 * alpha * R_plus
        qc = 0.5 * gm1 * R_plus * R_plus - 2.0 * c0sq / gm1
        disc = qb * qb - 4.0 * qa * qc
        speed = (-qb + np.sqrt(np.maximum(disc, 0.0))) / (2.0 * qa)
        # the earlier clamps of the same branch (disc > 0, speed > 0) stay as untaken as they are anywhere
        assert (disc > 0).all() and (speed > 0).all()
        M2 = speed * speed / (c0sq - 0.5 * gm1 * speed * speed)
        out["sub_in_char M2 clamped"] = int((M2 >= 1).sum())
        out["sub_in_char M2 < 1"] = int((M2 < 1).sum())
        gap = min(gap, np.abs(np.sqrt(M2) - 1.0).min())
    return out, gap


def ramp_totals(q, counter, T_l=None, p_l=None, gamma=1.4):
    """(p_total_temp, T_total_temp, the branches taken) of a ramped sub_in_char record at a ramp counter
    (src/bdy_inters.cpp:482-504); q is the record's column of `bc_params`"""
    p_total, T_total, p_coeff, T_coeff, p_old, T_old = q[6], q[7], q[11], q[12], q[13], q[14]
    taken = []
    if p_coeff:
        p0 = p_old + (p_total - p_old) * p_coeff * counter
        taken.append("p clamped" if p0 >= p_total else "p ramping")
        p0 = min(p0, p_total)
    else:
        p0 = p_total
        taken.append("p_ramp_coeff == 0")
    if T_coeff > 0:
        T0 = T_old + (T_total - T_old) * T_coeff * counter
        taken.append("T clamped" if T0 >= T_total else "T ramping")
        T0 = min(T0, T_total)
    elif T_coeff < 0:
        T0 = T_l * (p0 / p_l) ** ((gamma - 1.0) / gamma) if T_l is not None else None
        taken.append("T isentropic")
    else:
        T0 = T_total
        taken.append("T_ramp_coeff == 0")
    return p0, T0, taken


def fixtures(keep):
    """every single-class fixture that carries a residual's inputs (name, arrays), filtered by keep(arrays)"""
    import glob
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        name = os.path.basename(path)[:-4]
        if name.startswith("mixed_") or "_tgv" in name:
            continue
        d = np.load(path)
        if "sizes" in d.files and "riemann_solve_type" in d.files and keep(d):
            yield name, d


def report(name, census):
    print("%-24s %s" % (name, "  ".join("%s %d" % kv for kv in census.items())))


def test_hllc_takes_all_four_branches():
    best = {}
    for name in HLLC:
        d = load(name)
        assert int(np.ravel(d["riemann_solve_type"])[0]) == 3
        c = hllc_census(d)
        report(name, c)
        for k, v in c.items():
            best[k] = max(best.get(k, 0), v)
    # S_L >= 0 and S_R < 0 (the whole left / right flux) are the two that no subsonic fixture reaches
    for k in ("left", "star_left", "star_right", "right"):
        assert best[k] >= MIN_POINTS, (k, best)


@pytest.mark.parametrize("name", ["hex_p2_transonic", "quad_p3_transonic", "tet_p2_transonic", "pri_p2_transonic"])
def test_hllc_supersonic_branches_on_every_element_class(name):
    """each element class has its own face kernels (split 2-D / 3-D, general): each sees both one-sided branches"""
    c = hllc_census(load(name))
    assert c["left"] >= MIN_POINTS and c["right"] >= MIN_POINTS, c


def test_roem_clips_both_wave_speeds():
    best = {}
    for name in ROEM:
        d = load(name)
        assert int(np.ravel(d["riemann_solve_type"])[0]) == 2
        c = roem_census(d)
        report(name, c)
        for k, v in c.items():
            best[k] = max(best.get(k, 0), v)
    for k in ("b1_clipped", "b2_clipped", "unclipped"):
        assert best[k] >= MIN_POINTS, (k, best)


def test_boundary_states_take_every_branch_clear_of_the_switches():
    best = {}
    for name in BDY:
        c, gap = bdy_census(load(name))
        report(name, c)
        print("%-24s smallest distance from a switch: %.3e of the sound speed" % (name, gap))
        assert gap > MARGIN, (name, gap)
        for k, v in c.items():
            best[k] = max(best.get(k, 0), v)
    for k in ("sub_out_simp reverse flow", "sub_out_simp machn >= 1", "char supersonic inflow", "char supersonic outflow",
              "char subsonic inflow", "char subsonic outflow", "sub_in_char M2 clamped", "sub_in_char M2 < 1"):
        assert best[k] >= MIN_POINTS, (k, best)


def test_sutherland_fixture_has_a_temperature_field():
    """hex_p1_transonic_sutherland: the state that enters the last stored stage is not isothermal (the initial one is)"""
    d = load("hex_p1_transonic_sutherland")
    assert int(np.ravel(d["fix_vis"])[0]) == 0
    gamma, R_ref = float(np.ravel(d["gamma"])[0]), float(np.ravel(d["R_ref"])[0])

    def spread(u):
        rho = u[..., 0]
        p = (gamma - 1.0) * (u[..., 4] - 0.5 * (u[..., 1] ** 2 + u[..., 2] ** 2 + u[..., 3] ** 2) / rho)
        T = p / (rho * R_ref)
        return (T.max() - T.min()) / T.mean()

    assert spread(d["u_init"]) < 1e-12
    assert spread(d["u_step2_stage3"]) > 1e-2


def test_roem_clips_both_wave_speeds_on_every_element_class():
    """roeM_flux<ND> is compiled into the 2-D split kernels and the general stage's face kernels separately"""
    for name in ROEM_CLASSES:
        d = load(name)
        assert int(np.ravel(d["riemann_solve_type"])[0]) == 2
        c = roem_census(d)
        report(name, c)
        for k in ("b1_clipped", "b2_clipped", "unclipped"):
            assert c[k] >= MIN_POINTS, (name, k, c)


@pytest.mark.parametrize("name", sorted(SUTHERLAND))
def test_new_sutherland_fixtures_have_a_temperature_field(name):
    """as test_sutherland_fixture_has_a_temperature_field, on each class's fix_vis = 0 fixture"""
    d = load(name)
    assert int(np.ravel(d["fix_vis"])[0]) == 0
    gamma, R_ref, nd = float(np.ravel(d["gamma"])[0]), float(np.ravel(d["R_ref"])[0]), int(d["sizes"][4])

    def spread(u):
        rho = u[..., 0]
        p = (gamma - 1.0) * (u[..., nd + 1] - 0.5 * (u[..., 1:nd + 1] ** 2).sum(axis=-1) / rho)
        T = p / (rho * R_ref)
        return (T.max() - T.min()) / T.mean()

    last = max(k for k in d if k.startswith("u_step") and k.endswith("stage3"))
    assert SUTHERLAND[name] == last
    print("%-24s T spread %.3e at the start, %.3e entering the last stored stage" % (name, spread(d["u_init"]), spread(d[last])))
    assert spread(d["u_init"]) < 1e-12
    assert spread(d[last]) > 1e-2


def test_boundary_states_take_every_branch_in_two_dimensions():
    """bc_state<2> and bc_gradients<2> are instantiations of their own: the same branches as in 3-D, the same margin"""
    best = {}
    for name in BDY2:
        d = load(name)
        assert int(d["sizes"][4]) == 2 and int(np.ravel(d["viscous"])[0]) == 1
        c, gap = bdy_census(d)
        report(name, c)
        print("%-24s smallest distance from a switch: %.3e of the sound speed" % (name, gap))
        assert gap > MARGIN, (name, gap)
        for k, v in c.items():
            best[k] = max(best.get(k, 0), v)
    for k in ("sub_out_simp reverse flow", "sub_out_simp machn >= 1", "sub_out_simp subsonic", "char supersonic inflow",
              "char supersonic outflow", "char subsonic inflow", "char subsonic outflow", "sub_in_char M2 clamped",
              "sub_in_char M2 < 1"):
        assert best[k] >= MIN_POINTS, (k, best)


@pytest.mark.parametrize("nd", [2, 3])
def test_every_boundary_type_in_each_dimension(nd):
    """every hfx_bc_flag but `cyclic` on at least MIN_POINTS boundary flux points of some fixture, and -- the viscous sweep
    (bdy_viscflux_kernel, bc_gradients<ND>) -- of some VISCOUS fixture; slip_wall is the one flag that sweep returns on"""
    any_run, viscous_run = {}, {}
    for name, d in fixtures(lambda d: "bc_flags" in d.files and int(d["sizes"][4]) == nd):
        flags = d["bc_flags"].reshape(3, -1, order="F")[0]
        for t in range(3):
            if "bdy%d_L" % t in d.files:
                n_fpts = d["bdy%d_L" % t].shape[0]
                for fl, cnt in zip(*np.unique(flags[np.ravel(d["bdy%d_id" % t])], return_counts=True)):
                    for table in (any_run, viscous_run) if int(np.ravel(d["viscous"])[0]) else (any_run,):
                        if cnt * n_fpts > table.get(int(fl), (0, ""))[0]:
                            table[int(fl)] = (int(cnt * n_fpts), name)
    for bc, fl in BC_FLAGS.items():
        if bc != "cyclic":
            print("ND %d %-15s %-32s viscous: %s" % (nd, bc, any_run.get(fl), viscous_run.get(fl)))
    for bc, fl in BC_FLAGS.items():
        if bc != "cyclic":
            assert any_run.get(fl, (0,))[0] >= MIN_POINTS, (nd, bc)
            assert viscous_run.get(fl, (0,))[0] >= MIN_POINTS, (nd, bc, "viscous sweep")


def test_ramp_takes_every_branch():
    """the total-pressure / total-temperature ramp of sub_in_char (src/bdy_inters.cpp:482-504) at the ramp counter of every
    stored step (the counter advances after each step, src/HiFiLES.cpp:224-225)"""
    taken = {}
    for name, d in fixtures(lambda d: "bc_flags" in d.files and d["bc_flags"].reshape(3, -1, order="F")[1].any()):
        fl = d["bc_flags"].reshape(3, -1, order="F")
        par = d["bc_params"].reshape(15, -1, order="F")
        steps = sorted({int(k.split("_")[1][4:]) for k in d.files if k.startswith("u_step")})
        for st in steps:
            counter = int(np.ravel(d["ramp_counter"])[0]) + st
            for b in np.flatnonzero(fl[1]):
                assert fl[0][b] == SUB_IN_CHAR
                p0, _, branches = ramp_totals(par[:, b], counter)
                print("%-20s step %d counter %d: %s" % (name, st, counter, ", ".join(branches)))
                for k in branches:
                    taken.setdefault(k, set()).add(name)
    for k in ("p ramping", "p clamped", "T ramping", "T clamped", "T isentropic", "p_ramp_coeff == 0"):
        assert taken.get(k), (k, taken)


# class / switch pairs that the reference itself refuses: none.  (It refuses Lax-Friedrichs on a Navier-Stokes run,
# src/input.cpp:546, which is no row of this table.)  The tetrahedron / prism inviscid row is filled by captures
# (tet_p2_inviscid, pri_p2_inviscid), not by an override.
REFUSED_BY_THE_REFERENCE = set()
SWITCHES = {
    "RoeM": lambda s: s["riemann_solve_type"] == 2,
    "Rusanov": lambda s: s["riemann_solve_type"] == 0,
    "fix_vis=0": lambda s: s["viscous"] == 1 and s["fix_vis"] == 0,
    "ldg_tau, |ldg_beta| != 1/2": lambda s: s["viscous"] == 1 and s["ldg_tau"] != 0 and abs(s["ldg_beta"]) != 0.5,
    "viscous=0": lambda s: s["viscous"] == 0,
}


def test_switch_table():
    """every run-wide switch of the face-point physics on every element class, in at least one fixture that carries stage
    states: the pairwise kernels take the solver as a template argument, so every (class, switch) is machine code of its own"""
    table = {}
    for name, d in fixtures(lambda d: any(k.startswith("u_step") for k in d.files) and "detjac_upts" in d.files):
        cls = ELE_CLASSES[int(d["sizes"][6])]
        s = {k: float(np.ravel(d[k])[0]) for k in ("riemann_solve_type", "fix_vis", "ldg_tau", "ldg_beta", "viscous")}
        for sw, has in SWITCHES.items():
            if has(s):
                table.setdefault((cls, sw), []).append(name)
    missing = []
    for cls in ELE_CLASSES.values():
        for sw in SWITCHES:
            print("%-6s %-28s %s" % (cls, sw, ", ".join(table.get((cls, sw), [])) or "-"))
            if not table.get((cls, sw)) and (cls, sw) not in REFUSED_BY_THE_REFERENCE:
                missing.append((cls, sw))
    assert not missing, missing
