"""The tensor-element path on meshes of MIXED element orientation (reorient.py), without a device.

Every box of the host mirror numbers its cells alike; here the registration of such a box is rewritten in test code so that every
element lives in reference coordinates of its own, one of the 24 proper rotations of the cube (4 of the square).  Three things are
held: (a) the oracle's result does not depend on the orientation -- which proves the transform, the index conventions of JGinv_* and
Jacobian_fpts included; (b) the re-oriented tables offer what a uniformly oriented box never does (stated on the tables alone);
(c) the comparison of (a) notices face tables that pair the points of rotated faces as if they were aligned.
tests/test_gpu_element_orientation.py runs the same registrations through every kernel form of the device."""
import numpy as np
import pytest

import ragged_partition as RP
import reorient as RO

TOL_U, TOL_DIV = 1e-12, 1e-11
STEPS = 2
MACH, MU_GAS = 0.5, 1.827e-03  # (tests/test_gpu_physics_matrix.py: the viscous switches move the result within two steps)
WALE = dict(LES=1, SGS_model=1, C_s=0.325, filter_ratio=1.0)


def walls_case():
    from test_partition_ragged import walls_kw, BOX
    return dict(n=BOX, **walls_kw())


# geometry -> keywords of hfx_host.Case
GEOMETRIES = {
    "hex_p2": lambda: dict(n=[3, 3, 3], order=2, amp=0.05),
    "hex_p2_box": lambda: dict(n=[3, 3, 3], order=2, amp=0.0),
    "quad_p3": lambda: dict(n=[5, 3, 1], dims=2, order=3, amp=0.05),
    "quad_p7": lambda: dict(n=[5, 3, 1], dims=2, order=7, amp=0.05),
    "hex_p4": lambda: dict(n=[3, 3, 3], order=4, amp=0.05),
    "hex_p4_box": lambda: dict(n=[3, 3, 3], order=4, amp=0.0),
    "hex_p4_sheared": lambda: dict(n=[3, 3, 3], order=4, amp=0.0, sheared=True),
    "hex_p6": lambda: dict(n=[3, 3, 3], order=6, amp=0.05),
    "walls": walls_case,
}
# seeds of orientation_vector: test_census_* state what they have to deliver
SEED = {"hex_p2": 1, "hex_p2_box": 1, "quad_p3": 3, "quad_p7": 3, "hex_p4": 1, "hex_p4_box": 1, "hex_p4_sheared": 1, "hex_p6": 1,
        "walls": 1, "ragged": 9}
ROWS = {
    "hllc_beta_plus": dict(riemann_solve_type=3, viscous=1, ldg_beta=0.5, ldg_tau=0.0),
    "hllc_beta_minus": dict(riemann_solve_type=3, viscous=1, ldg_beta=-0.5, ldg_tau=0.0),
    "ldg_tau": dict(riemann_solve_type=3, viscous=1, ldg_beta=0.25, ldg_tau=0.3),
    "rusanov_inviscid": dict(riemann_solve_type=0, viscous=0, ldg_beta=0.5, ldg_tau=0.0),
    "wale": dict(riemann_solve_type=3, viscous=1, ldg_beta=0.5, ldg_tau=0.0),  # (registration built with the closure)
}
VISCOUS_ROWS = ["hllc_beta_plus", "hllc_beta_minus", "ldg_tau"]
# the box of walls_kw() has an isothermal and an adiabatic wall, refused on an inviscid run (tests/test_gpu_physics_matrix.py, REFUSED)
CPU_MATRIX = [("hex_p2", r) for r in VISCOUS_ROWS + ["rusanov_inviscid", "wale"]] + \
             [("hex_p2_box", r) for r in VISCOUS_ROWS + ["rusanov_inviscid"]] + \
             [("quad_p3", r) for r in VISCOUS_ROWS + ["rusanov_inviscid"]] + \
             [("walls", r) for r in VISCOUS_ROWS]


def relerr(a, b):
    scale = np.abs(b).max()
    return np.abs(a - b).max() / (scale if scale > 0 else 1.0)


# ---- registrations and the oracle's results: computed once, never written to ----------------------------------------------------

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def plain(geometry, les=False):
    """(registration dict, loc_upts, tloc_fpts) of the uniformly oriented box"""
    def make():
        import hfx_host as H
        g = GEOMETRIES[geometry]()
        n = g.pop("n")
        if g.pop("sheared", False):
            from test_gpu_affine_metrics import sheared_xv
            g["xv"] = sheared_xv(n)
        if "bcs" not in g:
            g.update(Mach_c_ic=MACH, mu_gas=MU_GAS)
        c = H.Case(n, **dict(g, **(WALE if les else {})))
        out = c.registration(), c.array("loc_upts"), c.array("tloc_fpts")
        c.close()
        return out
    return cached(("plain", geometry, les), make)


def rot_of(geometry):
    reg = plain(geometry)[0]
    return RO.orientation_vector(int(reg["sizes"][0]), int(reg["sizes"][4]), SEED[geometry])


def oriented(geometry, les=False):
    return cached(("oriented", geometry, les), lambda: RO.reorient(plain(geometry, les)[0], rot_of(geometry), *plain(geometry, les)[1:]))


def with_row(reg, row):
    reg = dict(reg)
    for k, v in ROWS[row].items():
        reg[k] = np.array([float(v)])
    return reg


def registration(geometry, row, turned):
    les = row == "wale"
    return with_row(oriented(geometry, les) if turned else plain(geometry, les)[0], row)


def oracle_result(geometry, row, turned):
    """(u, div) of the oracle after STEPS steps, in the point order of the registration it ran on"""
    def make():
        import oracle_py as O
        O.load().orc_set_threads(4)  # (the same bits with any number of threads: tests/test_oracle_vs_golden.py)
        try:
            u, div = RP.undivided_oracle(registration(geometry, row, turned), STEPS)
        finally:
            O.load().orc_set_threads(1)
        u, div = u.copy(), div.copy()
        assert np.isfinite(u).all() and np.isfinite(div).all()
        u.setflags(write=False)
        div.setflags(write=False)
        return u, div
    return cached(("oracle", geometry, row, turned), make)


# ---- the transform itself --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geometry", ["hex_p2", "quad_p3", "walls"])
def test_identity_returns_the_input_bit_for_bit(geometry):
    reg, lu, lf = plain(geometry)
    out = RO.reorient(reg, np.zeros(int(reg["sizes"][0]), dtype=int), lu, lf)
    assert set(out) == set(reg)
    for k in reg:
        a, b = np.asarray(reg[k]), np.asarray(out[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes(order="F") == b.tobytes(order="F"), k
    u = np.asarray(reg["u_init"])
    assert np.array_equal(RO.back(u, np.zeros(u.shape[1], dtype=int)), u)


def test_back_inverts_the_point_permutation():
    reg = plain("hex_p2")[0]
    rot = rot_of("hex_p2")
    assert np.array_equal(RO.back(oriented("hex_p2")["u_init"], rot), reg["u_init"])
    assert not np.array_equal(oriented("hex_p2")["u_init"], reg["u_init"])


def test_values_are_copied_not_recomputed():
    """every metric value of the output is a value of the input, up to the sign G gives: norm_fpts keeps the rounding noise that
    decides the LDG switch on axis-aligned faces"""
    reg, out = plain("hex_p2_box")[0], oriented("hex_p2_box")
    for k in RP.ELEMENT_AXIS:
        if k in reg:
            signed = k.startswith(("JGinv", "Jacobian"))
            a, b = np.asarray(reg[k]), np.asarray(out[k])
            for e in range(int(reg["sizes"][0])):
                va, vb = np.take(a, e, axis=RP.ELEMENT_AXIS[k]), np.take(b, e, axis=RP.ELEMENT_AXIS[k])
                va, vb = (np.abs(va), np.abs(vb)) if signed else (va, vb)
                assert np.array_equal(np.sort(va, axis=None), np.sort(vb, axis=None)), (k, e)
    noise = np.asarray(out["norm_fpts"])
    assert ((noise != 0.0) & (np.abs(noise) < 1e-12)).any()  # (it is there to be kept)


def test_refuses_an_element_array_without_a_rule():
    reg, lu, lf = plain("hex_p2")
    rot = rot_of("hex_p2")
    sz = [int(v) for v in reg["sizes"]]
    for k, shape in (("JGinv_over_int_cubpts", (3, 3, 64, sz[0])), ("opp_over_int_cubpts", (64, sz[1])), ("sensor", (sz[0],))):
        with pytest.raises(AssertionError):
            RO.reorient(dict(reg, **{k: np.zeros(shape)}), rot, lu, lf)


def test_orientation_vector_is_seeded_and_complete():
    for nd, n_rot in ((2, 4), (3, 24)):
        a, b = RO.orientation_vector(40, nd, 11), RO.orientation_vector(40, nd, 11)
        assert np.array_equal(a, b) and not np.array_equal(a, RO.orientation_vector(40, nd, 12))
        assert sorted(a[:n_rot]) == list(range(n_rot)) and len(RO.rotations(nd)) == n_rot


# ---- the transform against the genuine reference's own preprocessor ----------------------------------------------------------------

@pytest.mark.parametrize("name,seed", [("hex_p2_scrambled", 1), ("quad_p3_scrambled", 3)])
def test_reorient_reproduces_the_reference_preprocessor(name, seed):
    """The fixtures *_scrambled were captured from the genuine reference on a mesh whose cells oracle/gen_neu_mesh.py wrote
    rotated (orient_seed; the same seeded vector and the same list of rotations as orientation_vector / rotations).  The host
    mirror's box of the same size, re-oriented here, has the reference's face tables pair for pair and its metrics to rounding
    (they are evaluated from rotated shape functions there, copied here)."""
    import json
    import os
    import hfx_host as H
    d = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")))
    meta = json.loads(bytes(d["meta_json"]).decode())
    assert meta["orient_seed"] == seed
    n, nd = meta["n"], meta["dims"]
    n = [n] * 3 if isinstance(n, int) else list(n) + [1] * (3 - len(n))
    c = H.Case(n, dims=nd, order=meta["keys"]["order"], amp=meta["amp"])
    reg, lu, lf = c.registration(), c.array("loc_upts"), c.array("tloc_fpts")
    c.close()
    assert np.abs(lu - d["loc_upts"]).max() < 1e-14 and np.abs(lf - d["tloc_fpts"]).max() < 1e-14
    out = RO.reorient(reg, RO.orientation_vector(int(reg["sizes"][0]), nd, seed), lu, lf)
    t = RP.face_types(reg)[0]
    pairs = lambda r: {tuple(a) + tuple(b) for a, b in zip(np.asarray(r["int%d_L" % t]).T, np.asarray(r["int%d_R" % t]).T)}
    assert pairs(out) == pairs(d) and len(pairs(d)) == d["int%d_L" % t].shape[1]
    assert pairs(reg) != pairs(d)
    for k in RP.ELEMENT_AXIS:
        if k in out:
            print("%s %s: %.3e" % (name, k, relerr(out[k], d[k])))
            assert relerr(out[k], d[k]) < 1e-13, k


# ---- a. invariance on the oracle -------------------------------------------------------------------------------------------------

def check_invariance(geometry, row, u, div):
    """u, div: results on the re-oriented registration"""
    rot = rot_of(geometry)
    u1, div1 = oracle_result(geometry, row, False)
    eu, ed = relerr(RO.back(u, rot), u1), relerr(RO.back(div, rot), div1)
    print("%s / %s: state %.3e, residual %.3e" % (geometry, row, eu, ed))
    return eu, ed


@pytest.mark.parametrize("geometry,row", CPU_MATRIX, ids=["%s-%s" % gr for gr in CPU_MATRIX])
def test_oracle_does_not_depend_on_the_orientation(geometry, row):
    u, div = oracle_result(geometry, row, True)
    eu, ed = check_invariance(geometry, row, u, div)
    assert relerr(oracle_result(geometry, row, False)[0], plain(geometry)[0]["u_init"]) > 1e-8  # (the state moved)
    assert eu < TOL_U and ed < TOL_DIV


# ---- b. what the re-oriented meshes offer (conditions on the tables) -------------------------------------------------------------

def face_sizes(reg):
    sz = [int(v) for v in reg["sizes"]]
    n_faces = 2 * sz[4]
    return sz[0], sz[2], sz[2] // n_faces, n_faces


def int_tables(reg):
    t = RP.face_types(reg)[0]
    return np.asarray(reg["int%d_L" % t]).astype(np.int64), np.asarray(reg["int%d_R" % t]).astype(np.int64)


def in_face_map(slots, nd):
    """which of the 8 symmetries of the n x n grid of a quadrilateral face (index a + n b) takes slot m to slots[m]; on an edge
    (nd = 2) 0 = same direction, 1 = reversed"""
    slots = np.asarray(slots)
    m = np.arange(slots.size)
    if nd == 2:
        return [np.array_equal(slots, m), np.array_equal(slots, m[::-1])].index(True)
    n = int(round(np.sqrt(slots.size)))
    a, b = m % n, m // n
    maps = []
    for swap in (False, True):
        for fa in (False, True):
            for fb in (False, True):
                p, q = (b, a) if swap else (a, b)
                maps.append((n - 1 - p if fa else p) + n * (n - 1 - q if fb else q))
    hit = [np.array_equal(slots, x) for x in maps]
    assert sum(hit) == 1, slots
    return hit.index(True)


def pair_census(reg):
    """{(left local face, right local face): set of in-face maps} of the interior faces"""
    ne, nfp, nff, n_faces = face_sizes(reg)
    L, R = int_tables(reg)
    assert (np.diff(L, axis=0) == 1).all() and (L[0] % nff == 0).all()  # the left side lists a whole local face, ascending
    out = {}
    for i in range(L.shape[1]):
        fl, fr = int(L[0, i] % nfp) // nff, int(R[0, i] % nfp) // nff
        assert ((R[:, i] % nfp) // nff == fr).all() and (R[:, i] // nfp == R[0, i] // nfp).all()
        out.setdefault((fl, fr), set()).add(in_face_map(R[:, i] % nfp % nff, n_faces // 2))
    return out


def sides_census(reg):
    """per local face: (elements where it is a left side, elements where it is a right side)"""
    ne, nfp, nff, n_faces = face_sizes(reg)
    L, R = int_tables(reg)
    fl, fr = (L[0] % nfp) // nff, (R[0] % nfp) // nff
    return [(int((fl == f).sum()), int((fr == f).sum())) for f in range(n_faces)]


@pytest.mark.parametrize("geometry", ["hex_p2", "hex_p2_box", "hex_p4", "hex_p4_box", "hex_p4_sheared", "hex_p6", "quad_p3", "quad_p7", "walls"])
def test_census_of_the_interior_faces(geometry):
    reg, box = oriented(geometry), plain(geometry)[0]
    nd = int(reg["sizes"][4])
    assert sorted(set(rot_of(geometry))) == list(range(4 if nd == 2 else 24))
    # the box: a local face meets the opposite one only, in one in-face order (and without periodic faces it is the left side in
    # every element or in none)
    assert all(len(v) == 1 for v in pair_census(box).values()) and len(pair_census(box)) <= 2 * nd
    assert all(abs(fl - fr) in (2, 5 if nd == 3 else 2) for fl, fr in pair_census(box))
    if geometry == "walls":
        assert all(l == 0 or r == 0 for l, r in sides_census(box))
    sides, pairs = sides_census(reg), pair_census(reg)
    print("%s: (left, right) per local face %s; %d pairs of local faces, in-face maps %s" %
          (geometry, sides, len(pairs), sorted(set().union(*pairs.values()))))
    assert all(l > 0 and r > 0 for l, r in sides)
    if nd == 3:
        # a pair of local faces admits four of the eight maps (which four: the local faces' own numbering); all four occur in
        # some pair, and more pairs of local faces occur than the box's three
        assert max(len(v) for v in pairs.values()) == 4 and len(pairs) > 4 * nd
    else:
        # edges of two counter-clockwise elements always meet reversed; the combinations of local faces are what varies
        assert set().union(*pairs.values()) == {1} and len(pairs) > 2 * nd


@pytest.mark.parametrize("geometry", ["hex_p4_box", "hex_p4_sheared"])
@pytest.mark.parametrize("beta", [0.5, -0.5])
def test_census_of_the_two_wave_need(geometry, beta):
    """|beta| = 1/2: on the box need[f] is 0 or n_eles (tests/test_gpu_flux_two_wave.py asserts it), here strictly in between"""
    from test_gpu_flux_two_wave import need_per_face
    ne = int(plain(geometry)[0]["sizes"][0])
    if geometry == "hex_p4_box":
        assert sorted(need_per_face(dict(plain(geometry)[0], ldg_beta=np.array([beta])))) == [0, 0, 0, ne, ne, ne]
    need = need_per_face(dict(oriented(geometry), ldg_beta=np.array([beta])))
    print("%s beta %+.1f: need per face %s of %d" % (geometry, beta, need, ne))
    assert all(0 < v < ne for v in need)


def test_census_of_the_walls():
    """every boundary group on at least three local face numbers (the box: one each)"""
    for reg, least in ((plain("walls")[0], 1), (oriented("walls"), 3)):
        ne, nfp, nff, _ = face_sizes(reg)
        L, ids = np.asarray(reg["bdy2_L"]).astype(np.int64), np.ravel(reg["bdy2_id"])
        assert (np.diff(L, axis=0) == 1).all() and (L[0] % nff == 0).all()
        faces = {int(g): sorted({int(f) for f in (L[0, ids == g] % nfp) // nff}) for g in np.unique(ids)}
        print("local faces per boundary group: %s" % faces)
        assert len(faces) == 6 and all(len(v) >= least for v in faces.values())
        if least == 1:
            assert all(len(v) == 1 for v in faces.values())
        seen = np.concatenate([np.ravel(reg["int2_L"]), np.ravel(reg["int2_R"]), np.ravel(reg["bdy2_L"])])
        assert np.array_equal(np.sort(seen), np.arange(nfp * ne))


def test_census_of_the_metrics():
    """JGinv of the Cartesian P4 box: diagonal and positive as built; re-oriented, a signed permutation -- some element has a zero
    on the diagonal and a negative entry off it"""
    box, reg = np.asarray(plain("hex_p4_box")[0]["JGinv_upts"]), np.asarray(oriented("hex_p4_box")["JGinv_upts"])
    off = ~np.eye(3, dtype=bool)
    assert (np.abs(box[off]) < 1e-12).all() and (box[~off] > 0).all()
    found = [e for e in range(reg.shape[3]) if (np.abs(reg[~off][:, 0, e]) < 1e-12).any() and (reg[off][:, 0, e] < -1e-3).any()]
    print("elements with a zero diagonal entry and a negative off-diagonal one: %d of %d" % (len(found), reg.shape[3]))
    assert found
    # a face normal that points along -x on local face "x+" (hfx_host.SIDES3: local face 2)
    n = np.asarray(oriented("hex_p4_box")["norm_fpts"])
    assert (n[2 * 25:3 * 25, :, 0] < -0.99).any() and not (np.asarray(plain("hex_p4_box")[0]["norm_fpts"])[2 * 25:3 * 25, :, 0] < 0.99).any()


def ragged_registration(turned):
    """the 4 x 4 x 4 box of tests/test_partition_ragged.py, (registration, rot)"""
    import test_partition_ragged as TR
    kw = dict(TR.CFG, riemann_solve_type=3)

    def make():
        import hfx_host as H
        c = H.Case(TR.BOX, **kw)
        out = c.registration(), c.array("loc_upts"), c.array("tloc_fpts")
        c.close()
        return out
    reg, lu, lf = cached(("ragged", "plain"), make)
    rot = RO.orientation_vector(int(reg["sizes"][0]), 3, SEED["ragged"])
    if not turned:
        return reg, rot
    return cached(("ragged", "oriented"), lambda: RO.reorient(reg, rot, lu, lf)), rot


def partition_maps(parts, nff):
    """in-face maps of the partition faces as their left sides see them (Rlut: the slot in the peer's record)"""
    return {in_face_map(P.Rlut[:, i], 3) for P in parts for i, (_, left) in enumerate(P.faces) if left}


@pytest.mark.parametrize("name", ["ragged4", "ragged6"])
def test_census_of_the_partition_faces(name):
    """some partition-face pair has a relative rotation other than the box's"""
    import test_partition_ragged as TR
    box = partition_maps(RP.cut(ragged_registration(False)[0], TR.part_vector(name)), 9)
    got = partition_maps(RP.cut(ragged_registration(True)[0], TR.part_vector(name)), 9)
    print("%s: in-face maps of the partition faces %s (box %s)" % (name, sorted(got), sorted(box)))
    assert len(got) >= 4 and got - box


# ---- c. the comparison sees it ---------------------------------------------------------------------------------------------------

def aligned_pairs(reg_box, rot, lu, lf):
    """reorient's tables with the in-face permutation left out of the pairing: the left column sorted as it has to be, the right
    column renumbered but left in the row order of the box"""
    good = RO.reorient(reg_box, rot, lu, lf)
    t = RP.face_types(reg_box)[0]
    nfp = int(reg_box["sizes"][2])
    inv = np.argsort(np.stack([RO.point_perm(G, lf) for G in RO.rotations(int(reg_box["sizes"][4]))]), axis=1)
    R = np.asarray(reg_box["int%d_R" % t]).astype(np.int64)
    bad = dict(good)
    bad["int%d_R" % t] = RP.F32(inv[rot[R // nfp], R % nfp] + nfp * (R // nfp))
    assert np.array_equal(np.sort(bad["int%d_R" % t], axis=0), np.sort(good["int%d_R" % t], axis=0))  # the same points, face by face
    assert not np.array_equal(bad["int%d_R" % t], good["int%d_R" % t])
    return bad


@pytest.mark.parametrize("geometry", ["hex_p2", "walls"])
def test_faces_paired_as_if_aligned_miss_the_comparison(geometry):
    """(hexahedra: a rotation of the square takes an edge to an edge in the same sense, so a quadrilateral has no in-face
    permutation to leave out -- what varies in 2-D is which local faces meet)"""
    reg, lu, lf = plain(geometry)
    rot = rot_of(geometry)
    bad = with_row(aligned_pairs(reg, rot, lu, lf), "hllc_beta_plus")
    u, div = RP.undivided_oracle(bad, STEPS)
    eu, ed = check_invariance(geometry, "hllc_beta_plus", u, div)
    assert eu > 1e-6 and ed > 1e-6
