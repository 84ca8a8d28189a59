"""The mass-flux body force of driven periodic channels on the device (csrc/forcing.hip: hfx_eles_set_body_force,
hfx_eles_evaluate_body_force, the hook of the step loops) and through the host mirror.

The genuine reference cannot be made to dump this path, so the yardstick is `restatement` below -- src/eles.cpp:5340-5428 line
by line in NumPy -- together with the CPU oracle, which honours src_upts: the lockstep reference computes the force from the
oracle's own state before every step, adds it to src_upts and lets the oracle run the five stages.

The case: 4 x 3 x 3 P2 hexes from the host mirror (x and z periodic, isothermal walls in y; the mirror's periodic matching needs
three cells in z), smoothly deformed, and an affine copy on which the affine split kernels see the source term.  On the deformed
box the inflow plane is warped, the reference's rule (normal == -x exactly) selects nothing there, and the x-min faces are
registered explicitly; on the affine box the mirror's own selection is used.  The initial state is the Taylor-Green state plus
a streamwise velocity that varies across the channel; mdot0 = 1.1 x the initial mass flux and area = the true inflow area, so
no step's increment is a cancellation to zero.  RK45, dt_type 0.

Bounds.  integral(m): device and restatement add the same n = faces x cubature points x solution points products
w_j detjac_j opp_jk u_k in different orders, so |dev - ref| <= 4 n eps S_m with S_m the sum of their magnitudes (computed here);
the force is held to the same bound divided by area dt.  States: 1e-11, the project's standing figure.
"""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import hfx
import hfx_host as H
import oracle_py as O
import partition_util as PU
from test_gpu_methods_vs_golden import build, GOLDEN

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
N = [4, 3, 3]
LEN = 6.2831853071795862
WALLS = dict(bcs=[dict(type="isotherm_wall", T_static=310.0)], sides={"y-": 0, "y+": 0})
CFG = dict(order=2, length=LEN, T_c_ic=300.0, dt=1e-4, riemann_solve_type=3, body_forcing=1, **WALLS)
TOL = 1e-11


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def rel(a, b):
    s = np.abs(b).max()
    return float(np.abs(a - b).max() / (s if s > 0 else 1.0))


def col_rel(a, b):
    """rows of (mass_flux, ubulk, body_force(1)): the largest difference of every column over the column's largest magnitude (the
    force of a step on which the controller has converged is a small difference of large numbers)"""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    return float((np.abs(a - b).max(axis=0) / np.abs(b).max(axis=0)).max())


def driven_state(u0, pos):
    """the case's initial state plus a streamwise velocity that varies across the channel (same pressure)"""
    u = np.array(u0, order="F")
    rho = u[:, :, 0]
    vel = u[:, :, 1] / rho
    V = 2.0 * np.abs(vel).max()
    new = vel + V * (1.0 + 0.3 * np.cos(pos[:, :, 1]) + 0.1 * np.sin(2.0 * pos[:, :, 2]))
    u[:, :, 4] += 0.5 * rho * (new ** 2 - vel ** 2)
    u[:, :, 1] = rho * new
    return u


class Forcing:
    """the registered arrays of one block: faces as (element, local face), per local face opp and weights, per face detjac"""

    def __init__(self, ele, inter, opp, wgt, detjac, area):
        self.ele, self.inter, self.opp, self.wgt, self.detjac, self.area = list(ele), list(inter), opp, wgt, detjac, area

    def register(self, e, mdot0, capacity=64):
        e.set_body_force(self.ele, self.inter, self.opp, self.wgt, self.detjac, self.area, mdot0, capacity)

    def n_terms(self, n_upts):
        return sum(len(d) for d in self.detjac) * n_upts

    def integrals(self, u):
        """src/eles.cpp:5340-5373, the loops as written; also the sums of the magnitudes of the terms"""
        integral, mag = np.zeros(4), np.zeros(4)
        for f, (ele, l) in enumerate(zip(self.ele, self.inter)):
            for j in range(len(self.wgt[l])):
                wgt, detjac = self.wgt[l][j], self.detjac[f][j]
                disu_cubpt, m = np.zeros(4), np.zeros(4)
                for k in range(u.shape[0]):
                    disu_cubpt += self.opp[l][j, k] * u[k, ele, :4]
                    m += np.abs(self.opp[l][j, k] * u[k, ele, :4])
                integral += wgt * disu_cubpt * detjac
                mag += np.abs(wgt * detjac) * m
        return integral, mag


def restatement(F, u, mdot0, mdot_old, dt):
    """src/eles.cpp:5340-5428 -> dict(integral, magnitudes, ubulk, mass_flux, body_force(1), body_force(4))"""
    integral, mag = F.integrals(u)
    ubulk = 0.0 if integral[0] == 0 else integral[1] / integral[0]
    mass_flux = ubulk * integral[0]
    bf1 = 1.0 / F.area / dt * (mdot0 - 2.0 * mass_flux + mdot_old)
    return dict(integral=integral, mag=mag, ubulk=ubulk, mass_flux=mass_flux, bf1=bf1, bf4=bf1 * ubulk)


def forcing_of_case(c, deformed):
    """deformed: the x-min faces (local face 4 of the cells i = 0) by hand; affine: what the mirror's rule selects"""
    if deformed:
        nx, ny, nz = N
        ele = [nx * (j + ny * k) for k in range(nz) for j in range(ny)]
        inter = [4] * len(ele)
        assert len(c.inflow_faces()[0]) == 0
    else:
        ele, inter = (a.tolist() for a in c.inflow_faces())
        assert len(ele) == N[1] * N[2] and set(inter) == {4}
    opp = [c.array("opp_inters_cubpts_%d" % l) for l in range(6)]
    wgt = [c.array("weight_inters_cubpts_%d" % l) for l in range(6)]
    dj_all = c.array("inter_detjac_inters_cubpts_4")
    detjac = [dj_all[:, e].copy() for e in ele]
    area = float(sum(wgt[4] @ d for d in detjac))
    if not deformed:
        assert abs(area / LEN ** 2 - 1.0) < 1e-13
    return Forcing(ele, inter, opp, wgt, detjac, area)


class Fixture:
    """everything a test needs of one box, made once: registration data, forcing arrays, initial state, mdot0 and the lockstep
    CPU reference after one..four steps (states, src_upts and the controller's rows)"""

    def __init__(self, deformed):
        self.deformed = deformed
        self.cfg = dict(CFG, amp=0.05 if deformed else 0.0)
        c = H.Case(N, **self.cfg)
        self.reg = c.registration()
        self.F = forcing_of_case(c, deformed)
        self.u_init = driven_state(self.reg["u_init"], c.array("pos_upts"))
        self.reg["u_init"] = self.u_init
        self.dt = float(np.ravel(self.reg["dt"])[0])
        c.close()
        first = restatement(self.F, self.u_init, 0.0, 0.0, self.dt)
        assert first["integral"][1] > 0.1 * first["mag"][1]  # a mass flux, not a cancellation
        self.mdot0 = 1.1 * first["mass_flux"]
        self._ref = None

    def reference(self):
        if self._ref is None:
            o = O.load()
            oc = O.Case(self.reg, u_init=self.u_init)
            ce, (cf, nf), (cb, nb) = oc.c_eles(), oc.c_faces(), oc.c_bdy()
            src = np.zeros(self.u_init.shape, order="F")
            ce.src_upts = O.fptr(src)
            states, srcs, rows, mdot_old = [], [], [], self.mdot0
            for _ in range(4):
                r = restatement(self.F, oc.arr["u0"], self.mdot0, mdot_old, self.dt)
                src[:, :, 1] += r["bf1"]
                src[:, :, 4] += r["bf4"]
                mdot_old = r["mass_flux"]
                assert o.orc_rk_step_bdy(C.byref(ce), cf, nf, cb, nb, C.byref(oc.params)) < 0
                states.append(oc.arr["u0"].copy(order="F"))
                srcs.append(src.copy(order="F"))
                rows.append((r["mass_flux"], r["ubulk"], r["bf1"]))
            self._ref = (states, srcs, np.array(rows))
        return self._ref

    def device(self, ctx=None, register=True):
        ctx = ctx or hfx.Context(0)
        e, faces = build(ctx, self.reg)
        if register:
            self.F.register(e, self.mdot0)
        return ctx, e, faces

    def mirror(self, **kw):
        c = H.Case(N, **dict(self.cfg, forcing_area=self.F.area, forcing_mdot0=self.mdot0, **kw))
        c.to_device(0)
        upload_state(c, self.u_init)
        return c


def upload_state(c, u):
    e = c.handles()[1]
    u = np.asfortranarray(u)
    hfx.check(hfx.lib().hfx_eles_upload(e, C.c_int(hfx.DISU_UPTS0), u.ctypes.data_as(hfx.dp)))


def download_state(c):
    e = c.handles()[1]
    u = np.zeros((c.n_upts, c.n_eles, c.n_fields), order="F")
    hfx.check(hfx.lib().hfx_eles_download(e, C.c_int(hfx.DISU_UPTS0), u.ctypes.data_as(hfx.dp)))
    return u


_FIX = {}


def fixture(deformed):
    if deformed not in _FIX:
        _FIX[deformed] = Fixture(deformed)
    return _FIX[deformed]


def close(ctx, e, faces):
    for f in faces:
        f.close()
    e.close()
    ctx.close()


# ---- 1. the integral -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deformed", [True, False])
def test_integral_and_force(deformed):
    X = fixture(deformed)
    ctx, e, faces = X.device()
    assert len(X.F.ele) == 9  # three workgroups of four faces, the last one with a single face
    u = e.download(hfx.DISU_UPTS0)
    e.evaluate_body_force()
    s = e.body_force_state()
    r = restatement(X.F, u, X.mdot0, X.mdot0, X.dt)
    n = X.F.n_terms(e.n_upts)
    bound = 4 * n * EPS * r["mag"]
    for m in (0, 1):
        print("integral(%d): dev %.17g ref %.17g |diff| %.3g bound %.3g" % (m, s["integral"][m], r["integral"][m],
                                                                           abs(s["integral"][m] - r["integral"][m]), bound[m]))
        assert abs(s["integral"][m] - r["integral"][m]) <= bound[m]
    fb = bound[1] / (X.F.area * X.dt)
    print("force: dev %.17g ref %.17g |diff| %.3g bound %.3g" % (s["body_force_x"], r["bf1"], abs(s["body_force_x"] - r["bf1"]), fb))
    assert abs(s["body_force_x"] - r["bf1"]) <= fb
    assert s["n_steps"] == 1 and abs(s["mass_flux"] - r["mass_flux"]) <= bound[1] + 4 * EPS * abs(r["mass_flux"])
    # the source term is the force, on fields 1 and 4 alone
    src = e.download(hfx.SRC_UPTS)
    assert np.all(src[:, :, 1] == s["accumulated"][0]) and np.all(src[:, :, 4] == s["accumulated"][1])
    assert not src[:, :, [0, 2, 3]].any() and s["accumulated"][0] == s["body_force_x"]
    # the same state again: the same bits (a registration resets the controller, so mdot_old is mdot0 again)
    X.F.register(e, X.mdot0)
    e.evaluate_body_force()
    s2 = e.body_force_state()
    assert s2["n_steps"] == 1
    assert np.array_equal(s2["integral"], s["integral"]) and s2["body_force_x"] == s["body_force_x"] and s2["ubulk"] == s["ubulk"]
    # and as the second evaluation of a controller: the integral does not depend on the controller's history
    e.evaluate_body_force()
    assert np.array_equal(e.body_force_state()["integral"], s["integral"])
    close(ctx, e, faces)


# ---- 2. the controller's sequence ---------------------------------------------------------------------------------------------
def test_controller_sequence():
    X = fixture(True)
    ctx, e, faces = X.device()
    n = X.F.n_terms(e.n_upts)
    mdot_old, acc, rows, b_prev = X.mdot0, np.zeros(2), [], 0.0
    for step in range(4):
        u = e.download(hfx.DISU_UPTS0)
        hfx.run_steps(e, faces, 1, fused=3)
        s = e.body_force_state()
        r = restatement(X.F, u, X.mdot0, mdot_old, X.dt)
        b = 4 * n * EPS * r["mag"][1]
        fb = (2 * b + b_prev) / (X.F.area * X.dt)  # this step's mass flux twice, the previous one once
        print("step %d: mass_flux dev %.17g ref %.17g; force dev %.17g ref %.17g (bound %.3g)" %
              (step, s["mass_flux"], r["mass_flux"], s["body_force_x"], r["bf1"], fb))
        assert s["n_steps"] == step + 1
        assert abs(s["mass_flux"] - r["mass_flux"]) <= b + 4 * EPS * abs(r["mass_flux"])
        assert abs(s["ubulk"] - r["ubulk"]) <= (b + 4 * n * EPS * r["mag"][0] * abs(r["ubulk"])) / abs(r["integral"][0])
        assert abs(s["body_force_x"] - r["bf1"]) <= fb
        acc += (s["body_force_x"], s["body_force_x"] * s["ubulk"])
        assert np.abs(s["accumulated"] - acc).max() <= 8 * EPS * np.abs(acc).max()
        rows.append((s["mass_flux"], s["ubulk"], s["body_force_x"]))
        mdot_old, b_prev = s["mass_flux"], b  # (the device's own previous flux, so nothing accumulates in the comparison)
    assert abs(rows[0][2] - (2.0 * X.mdot0 - 2.0 * rows[0][0]) / (X.F.area * X.dt)) <= fb  # mdot_old = mdot0 at step one
    assert np.array_equal(e.body_force_history(), np.array(rows))
    assert np.array_equal(e.body_force_history(2), np.array(rows[2:]))
    # against the lockstep CPU run as well
    ref_rows = X.reference()[2]
    assert col_rel(e.body_force_history(), ref_rows) < 1e-9
    # a ring of two keeps the newest two
    X.F.register(e, X.mdot0, capacity=2)
    e.upload(hfx.DISU_UPTS0, X.u_init)
    hfx.run_steps(e, faces, 3, fused=3)
    h = e.body_force_history()
    assert h.shape == (2, 3) and e.body_force_state()["n_steps"] == 3
    assert col_rel(h, ref_rows[1:3]) < 1e-9 * np.abs(ref_rows).max() / np.abs(ref_rows[1:3]).max()
    close(ctx, e, faces)


# ---- 3. every loop ------------------------------------------------------------------------------------------------------------
def run_loop(e, faces, fused, n):
    if fused == 4:
        hfx.run_steps_blocks([e], faces, n, fused=4)
    else:
        hfx.run_steps(e, faces, n, fused=fused)


@pytest.mark.parametrize("deformed", [True, False])
@pytest.mark.parametrize("fused", [0, 2, 3, 4])
def test_every_loop_against_lockstep_reference(deformed, fused):
    X = fixture(deformed)
    states, srcs, rows = X.reference()
    ctx, e, faces = X.device()
    run_loop(e, faces, fused, 4)
    u4 = e.download(hfx.DISU_UPTS0)
    src4 = e.download(hfx.SRC_UPTS)
    err = rel(u4, states[3])
    print("fused %d, %s: state after four steps against the lockstep CPU run %.3g" % (fused, "deformed" if deformed else "affine", err))
    assert err < TOL
    assert rel(src4, srcs[3]) < 1e-9
    assert e.body_force_state()["n_steps"] == 4
    close(ctx, e, faces)


@pytest.mark.parametrize("loop", [0, 2, 3, 4, "mirror"])
def test_two_calls_of_two_steps_equal_one_of_four_bitwise(loop):
    """The controller's record (mdot_old, the accumulated force, the ring) and src_upts live on the device from call to call, so
    cutting the four steps into two calls changes nothing it is given."""
    X = fixture(True if loop != "mirror" else False)
    if loop == "mirror":
        got = []
        for calls in ([4], [2, 2]):
            c = X.mirror()
            for n in calls:
                c.run(n)
            got.append((download_state(c), c.body_force_history()))
            c.close()
    else:
        ctx, e, faces = X.device()
        got = []
        for calls in ([4], [2, 2]):
            X.F.register(e, X.mdot0)
            e.upload(hfx.DISU_UPTS0, X.u_init)
            for n in calls:
                run_loop(e, faces, loop, n)
            got.append((e.download(hfx.DISU_UPTS0), e.body_force_history(), e.download(hfx.SRC_UPTS)))
        close(ctx, e, faces)
    print("loop %s: two calls of two against one of four: state %.3g, history %.3g" %
          (loop, rel(got[1][0], got[0][0]), col_rel(got[1][1], got[0][1])))
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(a, b)


def test_mirror_run_steps_deferred():
    """the mirror's RunSteps on the affine box (its own inflow selection), deferred execution on: evaluate_body_force at the top
    of the first stage flushes exactly the previous stage, so every stage runs fused and none is replayed"""
    X = fixture(False)
    states, srcs, rows = X.reference()
    c = X.mirror()
    c.run(4)
    u = download_state(c)  # (the state alone: the stage still pending runs fused)
    nf, nr, why = hfx.deferred_stats(c.handles()[0])
    print("mirror, deferred: %.3g; %d stages fused, %d replayed %s" % (rel(u, states[3]), nf, nr, why))
    assert rel(u, states[3]) < TOL
    assert (nf, nr) == (20, 0), why
    s = c.body_force_state()
    assert s["n_steps"] == 4 and abs(s["body_force_x"] - rows[3][2]) < 1e-9 * np.abs(rows[:, 2]).max()
    assert col_rel(c.body_force_history(), rows) < 1e-9
    c.close()
    # two calls of two: the record pending between them is flushed by the first evaluation of the second call
    c = X.mirror()
    c.run(2)
    c.run(2)
    u2 = download_state(c)
    assert rel(u2, states[3]) < TOL
    assert hfx.deferred_stats(c.handles()[0])[:2] == (20, 0)
    c.close()
    # deferred off: the per-method calls
    c = X.mirror()
    c.set_deferred(False)
    c.run(4)
    assert rel(download_state(c), states[3]) < TOL
    c.close()


# ---- 4. it is the force that acts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [0, 3])
def test_unforced_run_differs(fused):
    X = fixture(True)
    states = X.reference()[0]
    ctx, e, faces = X.device(register=False)
    run_loop(e, faces, fused, 4)
    u = e.download(hfx.DISU_UPTS0)
    with pytest.raises(hfx.HfxError, match="never uploaded"):
        e.download(hfx.SRC_UPTS)  # no registration: no source term, no launch
    d = np.abs(u[:, :, 1] - states[3][:, :, 1]).max() / np.abs(states[3][:, :, 1]).max()
    print("x-momentum, unforced against forced: %.3g" % d)
    assert d > 1e-6
    close(ctx, e, faces)


# ---- 5. a source term of the caller's, the force on top ----------------------------------------------------------------------------
def test_source_term_on_top():
    X = fixture(False)
    ctx, e, faces = X.device(register=False)
    rng = np.random.default_rng(5)
    up = np.asfortranarray(1e-3 * rng.standard_normal(X.u_init.shape))
    e.upload(hfx.SRC_UPTS, up)
    X.F.register(e, X.mdot0)
    hfx.run_steps(e, faces, 2, fused=3)
    s = e.body_force_state()
    want = up.copy(order="F")
    want[:, :, 1] += s["accumulated"][0]
    want[:, :, 4] += s["accumulated"][1]
    src = e.download(hfx.SRC_UPTS)
    assert np.array_equal(src[:, :, [0, 2, 3]], up[:, :, [0, 2, 3]])
    err = rel(src, want)
    print("src_upts against upload + accumulated force: %.3g" % err)
    assert err < 1e-14 and abs(s["accumulated"][0]) > 1.0
    # registering again takes the contribution out and resets the controller
    X.F.register(e, X.mdot0)
    assert rel(e.download(hfx.SRC_UPTS), up) < 1e-14 * max(1.0, np.abs(want).max() / np.abs(up).max())
    e.clear_body_force()
    with pytest.raises(hfx.HfxError, match="no body force registered"):
        e.body_force_state()
    close(ctx, e, faces)


# ---- 6. tetrahedra: registered arrays of any class ----------------------------------------------------------------------------------
def tet_forcing(d):
    """NumPy-built arrays for a tetrahedron block (the mirror produces the surface cubature of hexahedra only): the face's flux
    points as cubature points -- opp_0's rows are the nodal basis there --, equal weights of the reference triangle's area 2, and
    tdA_fpts as the surface Jacobian.  Faces: local faces 0..3 of ten elements, so every local face and a partial workgroup occur"""
    sz = [int(v) for v in d["sizes"]]
    n_eles, n_upts, n_fpts = sz[:3]
    nfp = n_fpts // 4
    opp = [np.asfortranarray(d["opp_0"][l * nfp:(l + 1) * nfp, :]) for l in range(4)]
    wgt = [np.full(nfp, 2.0 / nfp) for l in range(4)]
    ele = [(3 * i) % n_eles for i in range(10)]
    inter = [i % 4 for i in range(10)]
    detjac = [np.array(d["tdA_fpts"])[l * nfp:(l + 1) * nfp, e].copy() for e, l in zip(ele, inter)]
    area = float(sum(wgt[l] @ dj for l, dj in zip(inter, detjac)))
    return Forcing(ele, inter, opp, wgt, detjac, area)


def test_tetrahedra_registered_arrays():
    d = load("tet_p2_n2_deformed")
    F = tet_forcing(d)
    u_init = np.asfortranarray(np.array(d["u_init"], dtype=np.float64))
    dt = float(np.ravel(d["dt"])[0])
    first = restatement(F, u_init, 0.0, 0.0, dt)
    mdot0 = 1.1 * first["mass_flux"] if abs(first["mass_flux"]) > 1e-3 * first["mag"][1] else first["mag"][1]
    ctx = hfx.Context(0)
    e, faces = build(ctx, d)
    F.register(e, mdot0)
    # the integral
    e.evaluate_body_force()
    s = e.body_force_state()
    r = restatement(F, u_init, mdot0, mdot0, dt)
    bound = 4 * F.n_terms(e.n_upts) * EPS * r["mag"]
    for m in (0, 1):
        print("tet integral(%d): |diff| %.3g bound %.3g" % (m, abs(s["integral"][m] - r["integral"][m]), bound[m]))
        assert abs(s["integral"][m] - r["integral"][m]) <= bound[m]
    assert abs(s["body_force_x"] - r["bf1"]) <= bound[1] / (F.area * dt)
    # two steps of the general fused stage against the lockstep CPU run
    o = O.load()
    oc = O.Case(d)
    ce, (cf, nf) = oc.c_eles(), oc.c_faces()
    src = np.zeros(u_init.shape, order="F")
    ce.src_upts = O.fptr(src)
    mdot_old = mdot0
    for _ in range(2):
        r = restatement(F, oc.arr["u0"], mdot0, mdot_old, dt)
        src[:, :, 1] += r["bf1"]
        src[:, :, 4] += r["bf4"]
        mdot_old = r["mass_flux"]
        assert o.orc_rk_step(C.byref(ce), cf, nf, C.byref(oc.params)) < 0
    F.register(e, mdot0)
    hfx.run_steps_blocks([e], faces, 2, fused=4)
    err = rel(e.download(hfx.DISU_UPTS0), oc.arr["u0"])
    print("tets, general fused stage, two steps: %.3g" % err)
    assert err < TOL
    assert rel(e.download(hfx.SRC_UPTS), src) < 1e-9
    close(ctx, e, faces)


# ---- 7. several ranks -----------------------------------------------------------------------------------------------------------------
class SumTransport(PU.ThreadTransport):
    """the thread transport of the partitioned tests plus the SUM reduction of the body force's integrals"""

    def __init__(self, world):
        super().__init__(world)
        self.sums = [None] * world

    def reduce_sum(self, rank):
        def fn(v):
            self.sums[rank] = list(v)
            self.barrier.wait()
            out = [sum(self.sums[r][i] for r in range(self.world)) for i in range(len(v))]  # rank order: the same bits everywhere
            self.barrier.wait()
            return out
        return fn


def test_two_ranks_threads():
    """The affine box cut in x, two ranks as threads on one card (host-staged exchange, as tests/test_gpu_partition.py does):
    rank 1 has no inflow faces, contributes zeros and receives the same force.  The integrals travel through the mirror's SUM
    hook and hfx_eles_body_force_integrals / _apply."""
    import torch
    X = fixture(False)
    one = X.mirror()
    one.run(2)
    u1 = download_state(one)
    s1 = one.body_force_state()
    one.close()
    assert rel(u1, X.reference()[0][1]) < TOL

    n_local, pgrid, world = [2, 3, 3], [2, 1, 1], 2
    cfg = dict(X.cfg, forcing_area=X.F.area, forcing_mdot0=X.mdot0)
    kw, _ = PU.case_kw(cfg)
    T = SumTransport(world)
    out, err = [None] * world, []

    def work(rank):
        try:
            torch.cuda.set_device(0)
            c = H.Case(list(n_local), rank=rank, pgrid=list(pgrid), **kw)
            assert len(c.inflow_faces()[0]) == (9 if rank == 0 else 0)
            c.to_device(0)
            upload_state(c, X.u_init[:, PU.global_index(n_local, pgrid, rank), :])
            T.register(rank, c, projected_flux=True)
            c.set_exchange(T.hook(rank))
            c.set_reduce_sum(T.reduce_sum(rank))
            T.barrier.wait()
            c.run_partitioned(2)
            out[rank] = (download_state(c), None, c.body_force_state(), c.body_force_history())
            T.barrier.wait()
            c.close()
        except BaseException as ex:  # noqa: BLE001
            err.append(ex)
            T.barrier.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if err:
        raise err[0]
    u = PU.assemble_arrays(out, 0, n_local, pgrid, u1.shape)
    print("two ranks against one: %.3g" % rel(u, u1))
    assert rel(u, u1) < TOL
    a, b = out[0][2], out[1][2]
    assert a["body_force_x"] == b["body_force_x"] and a["mass_flux"] == b["mass_flux"] and a["ubulk"] == b["ubulk"]
    assert np.array_equal(a["accumulated"], b["accumulated"]) and np.array_equal(out[0][3], out[1][3])
    assert a["n_steps"] == 2 and abs(a["body_force_x"] - s1["body_force_x"]) < 1e-9 * abs(X.reference()[2][0, 2])


def test_partitioned_loop_with_communicator():
    """hfx_run_steps_partitioned: the x wrap-around faces as partition faces of one rank that is its own neighbour, the library's
    communicator; the integrals take the all-reduce path (one rank: the identity) between the two halves of the evaluation"""
    X = fixture(False)
    states = X.reference()[0]
    c = X.mirror(self_partition=[1, 0, 0])
    c.set_comm(hfx.comm_unique_id())
    c.run_partitioned(2)
    u = download_state(c)
    print("self-partitioned, library communicator: %.3g" % rel(u, states[1]))
    assert rel(u, states[1]) < TOL
    assert c.body_force_state()["n_steps"] == 2
    c.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    X = fixture(False)
    F = X.F
    # a two-dimensional block
    d = load("quad_p3_vortex")
    ctx = hfx.Context(0)
    e, faces = build(ctx, d)
    with pytest.raises(hfx.HfxError, match="three-dimensional"):
        e.set_body_force([0], [0], [np.ones((4, e.n_upts))] * 4, [np.ones(4)] * 4, [np.ones(4)], 1.0, 1.0)
    with pytest.raises(hfx.HfxError, match="no body force registered"):
        e.evaluate_body_force()
    close(ctx, e, faces)
    # local time steps
    d = load("hex_p2_cfl_local")
    ctx = hfx.Context(0)
    e, faces = build(ctx, d)
    assert ctx.params.dt_type == 2
    with pytest.raises(hfx.HfxError, match="no body force registered"):
        e.body_force_state()  # a state query before the registration
    with pytest.raises(hfx.HfxError, match="no body force registered"):
        e.body_force_history()
    opp = [np.ones((4, e.n_upts)) / e.n_upts] * 6
    e.set_body_force([0, 1], [4, 4], opp, [np.ones(4)] * 6, [np.ones(4)] * 2, 1.0, 1.0)
    with pytest.raises(hfx.HfxError, match="local timestepping"):
        e.evaluate_body_force()
    e.set_h_ref(d["h_ref"])
    ctx.set_CFL(float(np.ravel(d["CFL"])[0]))
    for fused in (0, 3):  # (the loops' own calc_time_step comes first; the hook then refuses before its first launch)
        with pytest.raises(hfx.HfxError, match="local timestepping"):
            hfx.run_steps(e, faces, 1, fused=fused)
    assert e.body_force_state()["n_steps"] == 0
    with pytest.raises(hfx.HfxError, match="never uploaded"):
        e.download(hfx.SRC_UPTS)  # nothing was allocated, nothing launched
    # a face outside the block; the registration that stands is kept
    with pytest.raises(hfx.HfxError, match="names element"):
        e.set_body_force([0, e.n_eles], [4, 4], opp, [np.ones(4)] * 6, [np.ones(4)] * 2, 1.0, 1.0)
    with pytest.raises(hfx.HfxError, match="names element"):
        e.set_body_force([-1], [4], opp, [np.ones(4)] * 6, [np.ones(4)], 1.0, 1.0)
    with pytest.raises(hfx.HfxError, match="names local face"):
        e.set_body_force([0], [6], opp, [np.ones(4)] * 6, [np.ones(4)], 1.0, 1.0)
    with pytest.raises(hfx.HfxError, match="area"):
        e.set_body_force([0], [4], opp, [np.ones(4)] * 6, [np.ones(4)], 0.0, 1.0)
    assert e.body_force_state()["n_steps"] == 0
    close(ctx, e, faces)
    # zero faces are legal: the block only receives the force, (mdot0 + mdot_old) / (area dt) from a zero integral
    ctx, e, faces = X.device(register=False)
    e.set_body_force([], [], [None] * 6, [None] * 6, [], F.area, X.mdot0)
    e.evaluate_body_force()
    s = e.body_force_state()
    assert s["mass_flux"] == 0.0 and s["ubulk"] == 0.0 and s["body_force_x"] == 1.0 / F.area / X.dt * (X.mdot0 + X.mdot0)
    assert s["accumulated"][1] == 0.0
    # the NaN flag, the reference's message
    e.set_body_force([0], [4], F.opp, F.wgt, [F.detjac[0]], F.area, X.mdot0)
    u = np.array(X.u_init, order="F")
    u[0, 0, 1] = np.nan
    e.upload(hfx.DISU_UPTS0, u)
    e.evaluate_body_force()
    with pytest.raises(hfx.HfxError, match="NaN body force"):
        e.body_force_state()
    close(ctx, e, faces)
