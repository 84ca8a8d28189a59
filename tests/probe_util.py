"""What the probe tests share (tests/test_probes_host.py, tests/test_gpu_probes.py): the fixtures, the host mirror of each
element class, a plain-numpy statement of the six probe fields (src/output.cpp:1479-1538) and of the linear shape functions."""
import json
import os

import numpy as np

import hfx_host as H

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL_SIX = ["rho", "u", "v", "w", "specific_total_energy", "pressure"]  # the order of src/output.cpp:1482-1522
# plot fixture -> a fixture of the same mesh and order that holds the shape nodes (simplex classes: the mirror is built from them)
BLOCK_OF = {"hex_p3_plot": "hex_p3_n3_deformed", "tet_p2_plot": "tet_p2_n2_deformed", "pri_p2_plot": "pri_p2_n2_deformed"}
PLOT_FIXTURES = ["hex_p3_plot", "quad_p2_plot", "tet_p2_plot", "pri_p2_plot"]


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def meta(d):
    return json.loads(bytes(d["meta_json"]).decode())


def field_names(n_dims):
    return [f for f in ALL_SIX if n_dims == 3 or f != "w"]


def probe_fields(state, names, gamma):
    """state (n, n_fields): the interpolated conservative state of n probes -> (len(names), n), src/output.cpp:1479-1538"""
    n_dims = state.shape[1] - 2
    rho, E = state[:, 0], state[:, n_dims + 1]
    out = []
    for name in names:
        if name == "rho":
            out.append(rho)
        elif name in ("u", "v", "w"):
            out.append(state[:, 1 + "uvw".index(name)] / rho)
        elif name == "specific_total_energy":
            out.append(E / rho)
        else:
            v_sq = np.zeros_like(rho)
            for m in range(n_dims):
                v_sq = v_sq + state[:, m + 1] * state[:, m + 1]
            v_sq = v_sq / (rho * rho)
            out.append((gamma - 1.0) * (E - 0.5 * rho * v_sq))
    return np.array(out)


def interpolate(opp, ele, u):
    """opp (n_upts, n) operator rows as columns, ele (n), u (n_upts, n_eles, n_fields) -> (n, n_fields), summed in ascending
    order of the solution points as the reference's loop does"""
    out = np.zeros((opp.shape[1], u.shape[2]))
    for k in range(opp.shape[0]):
        out += opp[k, :, None] * u[k, ele, :]
    return out


def interpolate_reversed(opp, ele, u):
    out = np.zeros((opp.shape[1], u.shape[2]))
    for k in range(opp.shape[0] - 1, -1, -1):
        out += opp[k, :, None] * u[k, ele, :]
    return out


def field_rel(got, want):
    """per field: the largest difference over the field's largest magnitude over the probes.  A field that is zero at every
    probe (w of the fixtures' Taylor-Green state) has no magnitude to measure against: it must be reproduced exactly"""
    out = []
    for i in range(want.shape[0]):
        diff, scale = float(np.abs(got[i] - want[i]).max()), float(np.abs(want[i]).max())
        out.append(diff / scale if scale > 0 else (0.0 if diff == 0 else np.inf))
    return out


def mirror(name):
    """the host mirror of a plot fixture's element class on the fixture's mesh: an hfx_host.Case (hexahedra, quads) or an
    hfx_host.Simplex (tetrahedra, prisms); both have locate / calc_pos / pos_to_loc / opp_probe.  Returns (mirror, shape
    (n_dims, n_spts, n_eles), ele_type)"""
    d = load(name)
    m = meta(d)
    kk = m["keys"]
    et = int(d["sizes"][6])
    if et in (1, 4):
        n = m["n"] if isinstance(m["n"], list) else [m["n"]] * m["dims"]
        c = H.Case(n + [1] * (3 - len(n)), xv=d["xv"], dims=m["dims"], order=kk["order"], p_res=kk["p_res"], T_c_ic=kk["T_c_ic"])
        return c, c.array("shape"), et
    shape = load(BLOCK_OF[name])["shape"]
    return H.Simplex(et, kk["order"], shape), shape, et


# ---- the linear shape functions and their derivatives, restated (eles_hexas.cpp:1198, eles_quads, eles_tets.cpp:1030, eles_pris.cpp:1100)
def shape_basis(ele_type, loc):
    """-> (N (n_spts), dN (n_spts, n_dims)) at loc"""
    if ele_type in (1, 4):  # node = r + 2 s (+ 4 t), nodes at -1 and 1
        nd = 2 if ele_type == 1 else 3
        l = [np.array([(1 - loc[d]) / 2, (1 + loc[d]) / 2]) for d in range(nd)]
        dl = np.array([-0.5, 0.5])
        N, dN = np.zeros(2 ** nd), np.zeros((2 ** nd, nd))
        for m in range(2 ** nd):
            idx = [(m >> d) & 1 for d in range(nd)]
            N[m] = np.prod([l[d][idx[d]] for d in range(nd)])
            for c in range(nd):
                dN[m, c] = np.prod([dl[idx[d]] if d == c else l[d][idx[d]] for d in range(nd)])
        return N, dN
    r, s, t = loc
    if ele_type == 2:
        N = np.array([-(1 + r + s + t) / 2, (1 + r) / 2, (1 + s) / 2, (1 + t) / 2])
        dN = np.array([[-0.5, -0.5, -0.5], [0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5]])
        return N, dN
    N = np.array([(r + s) * (t - 1), -(r + 1) * (t - 1), -(s + 1) * (t - 1), -(r + s) * (t + 1), (r + 1) * (t + 1), (s + 1) * (t + 1)]) / 4
    dN = np.array([[t - 1, t - 1, r + s], [-(t - 1), 0, -(r + 1)], [0, -(t - 1), -(s + 1)],
                   [-(t + 1), -(t + 1), -(r + s)], [t + 1, 0, r + 1], [0, t + 1, s + 1]]) / 4
    return N, dN


def newton(ele_type, nodes, pos, max_iterations=50):
    """eles::pos_to_loc (src/eles.cpp:5992-6020) restated: nodes (n_dims, n_spts) of one element"""
    nd = nodes.shape[0]
    loc = np.zeros(nd)
    for _ in range(max_iterations):
        N, dN = shape_basis(ele_type, loc)
        dx = np.linalg.solve(nodes @ dN, pos - nodes @ N)
        loc = loc + dx
        if not np.sqrt(dx @ dx) > 1e-6:
            return loc
    raise RuntimeError("no convergence")


def inside_reference_element(ele_type, loc, margin=0.2):
    """strictly inside the reference element, `margin` away from its faces"""
    if ele_type in (1, 4):
        return bool(np.all(np.abs(loc) <= 1 - margin))
    if ele_type == 2:
        return bool(np.all(loc >= -1 + margin) and loc.sum() <= -1 - margin)
    return bool(loc[0] >= -1 + margin and loc[1] >= -1 + margin and loc[0] + loc[1] <= -margin and abs(loc[2]) <= 1 - margin)


def random_interior_locs(ele_type, n, seed):
    """n seeded reference locations with |loc_i| <= 0.6 that lie inside the reference element of the class (the simplex classes do
    not fill the cube: points outside are drawn again)"""
    rng = np.random.default_rng(seed)
    nd = 2 if ele_type == 1 else 3
    out = []
    while len(out) < n:
        l = rng.uniform(-0.6, 0.6, nd)
        if inside_reference_element(ele_type, l):
            out.append(l)
    return np.array(out).T.copy(order="F")
