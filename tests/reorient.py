"""Elements of mixed orientation, made in test code: TEST INFRASTRUCTURE.

Every quadrilateral and hexahedral mesh of the host mirror and of oracle/gen_neu_mesh.py is a structured box whose cells are all
numbered alike, so every element has the same orientation: a local face is the left side of its pair in every element or in none,
the points of a face meet their partners in one in-face order, JGinv of a Cartesian box is diagonal and positive.  `reorient`
describes element e of a one-block registration dict in the reference coordinates xi' = G_e xi, G_e one of the 24 proper rotations
of the reference cube (4 of the square).  The physical mesh, the face pairs and their left / right sides stay as they are.

The solution and flux point sets of the tensor classes are invariant under the cube group, so the class-level operators (opp_*)
are those of the input; per element

    arrays over points           permuted along the point axis, values copied (norm_fpts keeps its rounding noise bit for bit)
    JGinv_*  (ref, phys, pt, e)  permuted; |J| dxi'/dx = G |J| dxi/dx (csrc/host/eles.cpp, set_transforms_pts: first index reference)
                                 (JGinv_over_int_cubpts: through the permutation of the over-integration cubature points, a tensor
                                 Gauss set and as invariant as the solution points; the class-level matrices of over-integration and
                                 shock capturing are those of the input)
    Jacobian_fpts (phys, ref)    permuted; dx/dxi' = dx/dxi G^T
    int*_L, int*_R, bdy*_L       renumbered through the flux-point permutation, every column sorted again so that the left side's
                                 offsets ascend (the reference's tables), the R column carried along

G is a signed permutation: its products select and negate, nothing is rounded.
"""
import itertools
import re

import numpy as np

from ragged_partition import ELEMENT_AXIS, F32, face_types

UPTS_ARRAYS = ("detjac_upts", "u_init", "wall_distance")
FPTS_ARRAYS = ("detjac_fpts", "tdA_fpts", "norm_fpts")
# what a registration may hold besides: class-level operators, run-wide scalars, boundary groups
CLASS_LEVEL = re.compile(r"^(sizes|opp_[0-6](_[0-2])?|gamma|prandtl|rt_inf|mu_inf|c_sth|fix_vis|ldg_beta|ldg_tau|dt|viscous|"
                         r"riemann_solve_type|vis_riemann_solve_type|adv_type|dt_type|RK_a|RK_b|bc_flags|bc_params|bc_R_ref|"
                         r"ramp_counter|LES|SGS_model|C_s|filter_ratio|Kappa|prandtl_t|(int|bdy)[0-2]_(L|R|id)|"
                         r"over_int|opp_over_int_cubpts|over_int_filter|shock_cap|inv_vandermonde|exp_filter|norm_basis_persson|"
                         r"persson_high_modes|s0|shock_det_field)$")

_upts_perm = {}  # (n_dims, n_upts) -> (n_rot, n_upts): what `back` reads


def rotations(n_dims):
    """the proper rotations of the reference square / cube as integer matrices, the identity first"""
    out = []
    for p in itertools.permutations(range(n_dims)):
        for s in itertools.product((1, -1), repeat=n_dims):
            G = np.zeros((n_dims, n_dims), dtype=np.int64)
            for k in range(n_dims):
                G[k, p[k]] = s[k]
            if round(np.linalg.det(G)) == 1:
                out.append(G)
    assert len(out) == (4 if n_dims == 2 else 24) and np.array_equal(out[0], np.eye(n_dims, dtype=np.int64))
    return out


def point_perm(G, loc):
    """perm[j'] = j with G loc[:, j] = loc[:, j'] (to 1e-12: the reference's abscissae are symmetric only to rounding)"""
    loc = np.asarray(loc, dtype=np.float64)
    d = np.abs((G @ loc)[:, :, None] - loc[:, None, :]).max(axis=0)  # d[j, j']
    hit = d < 1e-12
    assert (hit.sum(axis=0) == 1).all() and (hit.sum(axis=1) == 1).all(), "the point set is not invariant under the rotation"
    return np.argmax(hit, axis=0)


def signed_rows(G):
    """[(k, sign)] per row k' of G: (G a)[k'] = sign * a[k]"""
    return [(int(np.flatnonzero(G[k])[0]), int(G[k].sum())) for k in range(G.shape[0])]


def orientation_vector(n_eles, n_dims, seed):
    """seeded: the first 24 (4) elements get every rotation once, in a seeded order; the others random rotations"""
    rng = np.random.RandomState(seed)
    n_rot = 4 if n_dims == 2 else 24
    rot = rng.randint(n_rot, size=n_eles)
    first = rng.permutation(n_rot)[:n_eles]
    rot[:first.size] = first
    return rot


def reorient(reg, rot, loc_upts, tloc_fpts, loc_over_int_cubpts=None):
    """the registration dict `reg` with element e in the coordinates G_rot[e] xi; loc_upts / tloc_fpts: (n_dims, n_points)
    reference locations of the solution and flux points (hfx_host.Case.array); loc_over_int_cubpts: those of the over-integration
    cubature points, needed where `reg` holds JGinv_over_int_cubpts"""
    sz = [int(v) for v in reg["sizes"]]
    ne, nu, nfp, nd = sz[0], sz[1], sz[2], sz[4]
    rot = np.asarray(rot)
    assert rot.shape == (ne,)
    assert np.shape(loc_upts) == (nd, nu) and np.shape(tloc_fpts) == (nd, nfp)
    for k in reg:
        assert k in ELEMENT_AXIS or CLASS_LEVEL.match(k), "no rule for %s" % k
    Gs = rotations(nd)
    pu = np.stack([point_perm(G, loc_upts) for G in Gs])
    pf = np.stack([point_perm(G, tloc_fpts) for G in Gs])
    assert np.array_equal(_upts_perm.setdefault((nd, nu), pu), pu)
    pc = None
    oi_keys = [k in reg for k in ("over_int", "opp_over_int_cubpts", "over_int_filter", "JGinv_over_int_cubpts")]
    assert all(oi_keys) or not any(oi_keys), "over-integration: the class-level matrices and the metrics at the cubature points go together"
    if "JGinv_over_int_cubpts" in reg:
        assert loc_over_int_cubpts is not None, "JGinv_over_int_cubpts needs the cubature locations"
        assert np.shape(loc_over_int_cubpts) == (nd, np.shape(reg["JGinv_over_int_cubpts"])[2])
        pc = np.stack([point_perm(G, loc_over_int_cubpts) for G in Gs])
    out = dict(reg)
    for k, axis in ELEMENT_AXIS.items():
        if k not in reg:
            continue
        a = np.asarray(reg[k])
        assert a.shape[axis] == ne
        new = np.array(a, order="F")
        for r in np.unique(rot):
            el = np.flatnonzero(rot == r)
            rows = signed_rows(Gs[r])
            if k in UPTS_ARRAYS or k in FPTS_ARRAYS:
                new[:, el] = a[(pu if k in UPTS_ARRAYS else pf)[r]][:, el]
            elif k in ("JGinv_upts", "JGinv_fpts", "JGinv_over_int_cubpts"):
                p = (pu if k == "JGinv_upts" else pf if k == "JGinv_fpts" else pc)[r]
                for k2, (k1, s) in enumerate(rows):
                    new[k2][:, :, el] = (a[k1] if s > 0 else -a[k1])[:, p][:, :, el]
            else:
                assert k == "Jacobian_fpts"
                for k2, (k1, s) in enumerate(rows):
                    new[:, k2][:, :, el] = (a[:, k1] if s > 0 else -a[:, k1])[:, pf[r]][:, :, el]
        out[k] = new
    inv = np.argsort(pf, axis=1)  # inv[r, j] = j'

    def renum(tab):
        tab = np.asarray(tab).astype(np.int64)
        return inv[rot[tab // nfp], tab % nfp] + nfp * (tab // nfp)

    for t in face_types(reg):
        L, R = renum(reg["int%d_L" % t]), renum(reg["int%d_R" % t])
        order = np.argsort(L, axis=0, kind="stable")
        out["int%d_L" % t], out["int%d_R" % t] = F32(np.take_along_axis(L, order, axis=0)), F32(np.take_along_axis(R, order, axis=0))
    for t in face_types(reg, "bdy"):
        out["bdy%d_L" % t] = F32(np.sort(renum(reg["bdy%d_L" % t]), axis=0))
    return out


def back(arr, rot):
    """a per-point result (n_upts, n_eles, n_fields) of a re-oriented registration in the original point order"""
    arr = np.asarray(arr)
    pu = _upts_perm[(arr.shape[2] - 2, arr.shape[0])]
    out = np.empty_like(arr, order="F")
    for r in np.unique(rot):
        el = np.flatnonzero(np.asarray(rot) == r)
        out[pu[r][:, None], el[None, :]] = arr[:, el]
    return out

