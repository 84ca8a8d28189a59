"""Deferred execution with other entry points BETWEEN the recorded calls (include/hfx.h, option "deferred").

test_gpu_deferred.py drives whole stages and downloads; here every entry point a caller may meet between two recorded calls
is put into the reference's call sequence, at two positions, on every kind of fused stage:

  configurations   K1  split stage + boundary faces        hex_p2_bdy_walls
                   K1r the same on quads with a ramp        quad_p3_ramp
                   K3  general stage, two element blocks    mixed_p3_channel
                   K2  partitioned split stage (RCCL)       a self-partitioned hex box of the host mirror
                   K4  partitioned general stage (RCCL)     mixed_p3_channel, half of its same-class faces partition faces
  positions        P0  between stages 1 and 2: stage 1 is pending behind its AdvanceSolution
                   P1  in the middle of stage 2, after the inviscid phase (receive_solution, the partition faces' common flux)

Three stages run (step 0, stages 0-2), then the state is read.  Every case is held to
  * the genuine reference (the fixture's u_step0_stage2; K2: the undivided box on the per-method path),
  * the same script with "deferred" off (1e-12), arrays the interjection downloads included,
  * at P0, the (n_fused, n_replayed) the interjection must leave, and where it adds no replay and does not replace the state,
    the bits of the script without the interjection,
  * on K2 / K4, the exchange accounting of the communicator: the solution messages posted (less the one a partitioned fused
    stage leaves in flight) are what the same partition-face calls post with "deferred" off -- replay and flush decisions are
    a rank's own and must not put it out of step with its neighbours -- and nothing is left running after a synchronise.
"""
import ctypes as C
import os

import numpy as np
import pytest

import hfx
import mixed_util as MU
from test_gpu_deferred import tag
from test_gpu_methods_vs_golden import GOLDEN, RTOLS, build, relerr

pytestmark = pytest.mark.gpu

N_STAGES = 3
CONFIGS = ["K1", "K1r", "K3", "K2", "K4"]
PARTITIONED = ("K2", "K4")
INTERJECTIONS = ["synchronize", "flush", "set_params", "set_option", "set_CFL", "download_u", "download_grad", "upload",
                 "monitors", "eles", "bdy", "ramp", "comm", "deferred_off_on"]
CFL = 0.5
# K2: the box of test_gpu_partition.py's RCCL cases, periodic in y, its x and z sides partition faces to the rank itself
K2_CASE = dict(order=2, amp=0.05, riemann_solve_type=3, length=6.2831853071795862, T_c_ic=300.0, dt=1e-4)
K2_N = [3, 4, 3]


def applies(cfg, which):
    if which == "ramp":
        return cfg == "K1r"
    if which == "comm":
        return cfg in PARTITIONED
    if which == "bdy":
        return cfg != "K2"
    return True


class Rig:
    """one configuration's blocks in a fresh context; blocks / faces (interior + boundary) / mpi lists in call order"""

    def __init__(self, cfg, deferred):
        self.cfg = cfg
        self.ctx = hfx.Context(0)
        self.mpi, self.comm, self.bdy_args = [], None, {}
        if cfg in ("K1", "K1r"):
            d = dict(np.load(os.path.join(GOLDEN, ("hex_p2_bdy_walls" if cfg == "K1" else "quad_p3_ramp") + ".npz")))
            e, self.faces = build(self.ctx, d)
            tag(e, d)
            self.blocks = [e]
            self.params = hfx.params_from(d)
            sz = [int(v) for v in d["sizes"]]
            self.new_eles = lambda: hfx.Eles(self.ctx, sz[:5], d, ele_type=sz[6], order=sz[5])
            recs = hfx.bc_records(d["bc_flags"], d["bc_params"])
            ts = [t for t in range(3) if "bdy%d_L" % t in d]
            first = len(self.faces) - len(ts)
            for i, t in enumerate(ts):
                self.bdy_args[first + i] = (e, d["bdy%d_L" % t], d["bdy%d_id" % t], recs, float(np.ravel(d["bc_R_ref"])[0]),
                                            int(np.ravel(d["ramp_counter"])[0]))
            self.ramp = int(np.ravel(d["ramp_counter"])[0])
            self.ref = lambda k: [d["u_step0_stage%d" % k]]
            self.ref_tol = RTOLS
        elif cfg in ("K3", "K4"):
            d = dict(np.load(os.path.join(GOLDEN, "mixed_p3_channel.npz")))
            classes, per, faces, bdy = MU.split(d)
            self.params = hfx.params_from(per[classes[0]])
            self.ctx.set_params(self.params)
            E = {}
            for c in classes:
                sz = [int(v) for v in per[c]["sizes"]]
                E[c] = hfx.Eles(self.ctx, sz[:5], per[c], ele_type=sz[6], order=sz[5])
                E[c].upload(hfx.DISU_UPTS0, per[c]["u_init"])
                E[c].les_model, E[c].has_over_int, E[c].has_shock = None, False, False
            c0 = classes[0]
            sz0 = [int(v) for v in per[c0]["sizes"]]
            self.new_eles = lambda: hfx.Eles(self.ctx, sz0[:5], per[c0], ele_type=sz0[6], order=sz0[5])
            if cfg == "K4":
                from test_mixed_mesh import self_partition
                faces, self.mpi = self_partition(self.ctx, E, faces)
                self.comm = hfx.Comm(self.ctx.h, hfx.comm_unique_id(), 1, 0)
            self.faces = [hfx.IntInters(self.ctx, E[a], E[b], L, R) for a, b, L, R in faces]
            recs = hfx.bc_records(d["bc_flags"], d["bc_params"])
            for a, L, ids in bdy:
                self.bdy_args[len(self.faces)] = (E[a], L, ids, recs, float(np.ravel(d["bc_R_ref"])[0]), int(np.ravel(d["ramp_counter"])[0]))
                self.faces.append(hfx.BdyInters(self.ctx, *self.bdy_args[len(self.faces)]))
            self.blocks = [E[c] for c in classes]
            self.ref = lambda k: [d["c%d_u_step0_stage%d" % (c, k)] for c in classes]
            self.ref_tol = RTOLS
        else:  # K2 (and its undivided twin "K2u", the reference)
            import hfx_host as H
            case = H.Case(K2_N, self_partition=[1, 0, 1] if cfg == "K2" else None, **K2_CASE)
            reg = case.registration()
            L, Rlut, _ = case.mpi_faces()
            seg = case.mpi_segments()
            case.close()
            e, self.faces = build(self.ctx, reg)
            e.les_model, e.has_over_int, e.has_shock = None, False, False
            self.blocks = [e]
            self.params = hfx.params_from(reg)
            sz = [int(v) for v in reg["sizes"]]
            self.new_eles = lambda: hfx.Eles(self.ctx, sz[:5], reg, ele_type=sz[6], order=sz[5])
            if cfg == "K2":
                assert L.shape[1] > 0
                m = hfx.MpiInters(self.ctx, e, L, Rlut)
                m.set_neighbours(seg)
                self.mpi = [m]
                self.comm = hfx.Comm(self.ctx.h, hfx.comm_unique_id(), 1, 0)
                ref = undivided_k2()
                self.ref = lambda k: [ref[k]]
                self.ref_tol = 1e-11  # (test_gpu_partition.py: the self-partitioned rank against the undivided box)
        self.adv = int(self.params.adv_type)
        self.viscous = bool(self.params.viscous)
        self.ctx.set_CFL(CFL)
        self.deferred = deferred
        self.ctx.set_option("deferred", int(deferred))

    def stage(self, rk, part):
        """CalcResidual's calls (src/solver.cpp:59-221) with the partition-face calls; part "inv": up to the partition faces'
        common inviscid flux, "rest": the viscous phase, the divergence and AdvanceSolution (src/HiFiLES.cpp:201-217)"""
        B, M, comm = self.blocks, self.mpi, self.comm
        ints = [f for f in self.faces if isinstance(f, hfx.IntInters)]
        bdys = [f for f in self.faces if isinstance(f, hfx.BdyInters)]
        for e in B:
            assert e.les_model is None  # (no configuration here carries an LES closure)
        if part == "inv":
            for e in B: e.extrapolate_solution()
            for f in M: f.send_solution(comm)
            if self.viscous:
                for e in B: e.calculate_gradient()
            for e in B: e.evaluate_invFlux_over_int() if e.has_over_int else e.evaluate_invFlux()
            for f in ints: f.calculate_common_invFlux()
            for f in bdys: f.evaluate_boundaryConditions_invFlux()
            for f in M: f.receive_solution(comm)
            for f in M: f.calculate_common_invFlux()
            return
        if self.viscous:
            for e in B: e.correct_gradient()
            for f in M: f.send_corrected_gradient(comm)
            for e in B: e.evaluate_viscFlux()
        for e in B: e.extrapolate_totalFlux()
        for e in B: e.calculate_divergence()
        if self.viscous:
            for f in ints: f.calculate_common_viscFlux()
            for f in bdys: f.evaluate_boundaryConditions_viscFlux()
            for f in M: f.receive_corrected_gradient(comm)
            for f in M: f.calculate_common_viscFlux()
        for e in B: e.calculate_corrected_divergence()
        for e in B: e.AdvanceSolution(rk, self.adv)
        for e in B:
            if e.has_shock:
                e.shock_capture()

    def run_loop(self, n_steps):
        """the whole RK loop inside the library: hfx_run_steps_partitioned (K2) / _blocks (K4)"""
        if self.cfg == "K4":
            hfx.run_steps_partitioned_blocks(self.blocks, self.faces, self.mpi, self.comm, n_steps)
            return
        fa, ma = hfx._face_array(self.faces), hfx._face_array(self.mpi)
        hfx.check(hfx.lib().hfx_run_steps_partitioned(self.blocks[0].h, fa, C.c_int(len(self.faces)), ma, C.c_int(len(self.mpi)),
                                                      self.comm.h, C.c_int(n_steps)))

    def state(self):
        return [e.download(hfx.DISU_UPTS0) for e in self.blocks]

    def close(self):
        for f in self.faces + self.mpi:
            f.close()
        if self.comm:
            self.comm.close()
        for e in self.blocks:
            e.close()
        self.ctx.close()


def is_current(e, array_id):
    cur = C.c_int(-1)
    hfx.check(hfx.lib().hfx_eles_is_current(e.h, C.c_int(array_id), C.byref(cur)))
    return cur.value


def interject(r, which):
    """one entry point that leaves the physics alone; -> what it read"""
    got = {}
    if which == "synchronize":
        r.ctx.synchronize()
    elif which == "flush":
        r.ctx.flush()
    elif which == "set_params":
        r.ctx.set_params(r.params)
    elif which == "set_option":
        r.ctx.set_option("xcd_order", 1)  # (its default)
        r.ctx.set_fused_mode(3)
    elif which == "set_CFL":
        r.ctx.set_CFL(CFL)
    elif which == "download_u":
        got["u"] = r.state()
    elif which == "download_grad":
        # a pending stage -- whole (P0) or partial (P1) -- runs call by call for it: the gradient of the stage, never an older one
        got["grad"] = [e.download(hfx.GRAD_DISU_UPTS) for e in r.blocks]
    elif which == "upload":
        u = r.state()
        for e, x in zip(r.blocks, u):
            e.upload(hfx.DISU_UPTS0, x)
    elif which == "monitors":
        # (the residual first: asked for while a whole stage is pending, it makes that stage store div_tconf_upts)
        res = []
        for e in r.blocks:
            if is_current(e, hfx.DIV_TCONF_UPTS) == 0:
                # (P1 after a fused stage that did not store it: neither stored nor pending -- it must fail, not answer)
                with pytest.raises(hfx.HfxError, match="not stored"):
                    e.compute_res_upts(2, 0)
                res.append(None)
            else:
                res.append([e.compute_res_upts(nt, fld) for nt in (1, 2) for fld in range(e.n_fields)])
        got["res"] = res
        got["nan"] = [e.check_nan() for e in r.blocks]
    elif which == "eles":
        x = r.new_eles()
        x.close()
    elif which == "bdy":
        for i, args in r.bdy_args.items():
            r.faces[i].close()
            r.faces[i] = hfx.BdyInters(r.ctx, *args)
    elif which == "ramp":
        for f in r.faces:
            if isinstance(f, hfx.BdyInters):
                f.set_ramp_counter(r.ramp)
    elif which == "comm":
        c2 = hfx.Comm(r.ctx.h, hfx.comm_unique_id(), 1, 0)
        c2.close()
    elif which == "deferred_off_on":
        r.ctx.set_option("deferred", 0)
        r.ctx.set_option("deferred", int(r.deferred))
    else:
        raise AssertionError(which)
    return got


def run_script(cfg, which, pos, deferred):
    """stages 0..2 of step 0 with `which` at `pos` (None: no interjection); -> dict of what the run left"""
    r = Rig(cfg, deferred)
    got = {}
    for rk in range(N_STAGES):
        if rk == 2 and pos == "P0" and which:
            got = interject(r, which)
        r.stage(rk, "inv")
        if rk == 2 and pos == "P1" and which:
            got = interject(r, which)
        r.stage(rk, "rest")
    out = dict(u=r.state(), got=got, stats=r.ctx.deferred_stats()[:2], ref=r.ref(N_STAGES - 1), ref_tol=r.ref_tol,
               n_mpi=len(r.mpi))
    if r.comm:
        out["ex"] = r.comm.exchange_stats()
        r.ctx.synchronize()
        out["busy_after_sync"] = r.comm.exchange_stats()["stream_busy"]
    r.close()
    return out


_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def undivided_k2():
    """the reference of K2: the undivided box on the per-method path, the state after every stage"""
    def run():
        r = Rig("K2u", False)
        u = []
        for rk in range(N_STAGES):
            r.stage(rk, "inv")
            r.stage(rk, "rest")
            u.append(r.state()[0])
        r.close()
        return u
    return cached(("K2u",), run)


def expected_stats(cfg, which, pos):
    if pos == "P1":
        return (N_STAGES - 1, 2)  # the stage is cut in two partial records, each replayed
    if which == "download_grad":
        return (N_STAGES - 1, 1)  # the fused stages keep the gradient on chip
    if which == "monitors" and cfg in PARTITIONED:
        return (N_STAGES - 1, 1)  # the partitioned stages store div_tconf_upts at the last stage of a step only
    return (N_STAGES, 0)


def close_to(a, b, tol):
    return all(relerr(x, y) < tol for x, y in zip(a, b))


@pytest.mark.parametrize("pos", ["P0", "P1"])
@pytest.mark.parametrize("cfg,which", [(c, w) for c in CONFIGS for w in INTERJECTIONS if applies(c, w)])
def test_interjection(cfg, which, pos):
    on = run_script(cfg, which, pos, True)
    off = run_script(cfg, which, pos, False)
    # the genuine reference
    for u, ref in zip(on["u"], on["ref"]):
        assert relerr(u, ref) < on["ref_tol"]
    # the per-method path: the state and whatever the interjection read
    assert close_to(on["u"], off["u"], 1e-12)
    for k in ("u", "grad"):
        if k in on["got"]:
            assert close_to(on["got"][k], off["got"][k], 1e-12), k
    if "res" in on["got"]:
        assert on["got"]["nan"] == off["got"]["nan"] == [-1] * len(on["u"])
        for a, b in zip(on["got"]["res"], off["got"]["res"]):
            if a is not None:
                assert np.allclose(a, b, rtol=1e-10, atol=0.0)
    # what ran fused
    assert on["stats"] == expected_stats(cfg, which, pos), on["stats"]
    assert off["stats"] == (0, 0)
    if pos == "P0" and on["stats"] == (N_STAGES, 0) and which != "upload":
        base = cached((cfg, "base"), lambda: run_script(cfg, None, "P0", True))
        assert base["stats"] == (N_STAGES, 0)
        for a, b in zip(on["u"], base["u"]):
            assert np.array_equal(a, b)
    # the messages follow the calls
    if cfg in PARTITIONED:
        n = on["n_mpi"]
        assert off["ex"]["posted"][0] == N_STAGES * n and off["ex"]["in_flight"] == 0
        # an upload of the state drops the message a partitioned fused stage had posted for the state it replaces
        dropped = n if (which == "upload" and pos == "P0") else 0
        assert on["ex"]["posted"][0] - on["ex"]["in_flight"] == off["ex"]["posted"][0] + dropped, on["ex"]
        assert on["ex"]["posted"][1] == off["ex"]["posted"][1]
        # P0: stage 2 ran fused and left the next state's solution on its way; P1: it was replayed and consumed it
        assert on["ex"]["in_flight"] == (n if pos == "P0" else 0)
        assert on["busy_after_sync"] == 0 and off["busy_after_sync"] == 0


@pytest.mark.parametrize("cfg", PARTITIONED)
def test_whole_loop_between_deferred_stages(cfg):
    """deferred stages, then hfx_run_steps_partitioned(_blocks) for a step, then deferred stages again: the loop takes the
    solution message the last fused stage posted instead of posting it again, and leaves nothing in flight"""
    res = {}
    for deferred in (True, False):
        r = Rig(cfg, deferred)
        for rk in (0, 1):
            r.stage(rk, "inv")
            r.stage(rk, "rest")
        r.run_loop(1)
        for rk in (0, 1):
            r.stage(rk, "inv")
            r.stage(rk, "rest")
        res[deferred] = (r.state(), r.comm.exchange_stats(), r.ctx.deferred_stats()[:2], len(r.mpi))
        r.ctx.synchronize()
        assert r.comm.exchange_stats()["stream_busy"] == 0
        r.close()
    (u_on, ex_on, st_on, n), (u_off, ex_off, st_off, _) = res[True], res[False]
    nst = 5
    assert st_on == (4, 0) and st_off == (0, 0)
    assert ex_off["posted"][0] == n * (2 + nst + 1 + 2) and ex_off["in_flight"] == 0
    assert ex_on["posted"][0] - ex_on["in_flight"] == ex_off["posted"][0], ex_on
    assert close_to(u_on, u_off, 1e-12)


@pytest.mark.parametrize("cfg", PARTITIONED)
def test_gradient_download_after_each_stage(cfg):
    """a rank that reads the gradient after every stage replays every stage; it posts what its neighbours post"""
    res = {}
    for deferred in (True, False):
        r = Rig(cfg, deferred)
        g = []
        for rk in range(N_STAGES):
            r.stage(rk, "inv")
            r.stage(rk, "rest")
            g.append([e.download(hfx.GRAD_DISU_UPTS) for e in r.blocks])
        res[deferred] = (r.state(), g, r.comm.exchange_stats(), r.ctx.deferred_stats()[:2])
        r.close()
    (u_on, g_on, ex_on, st_on), (u_off, g_off, ex_off, _) = res[True], res[False]
    assert st_on == (0, N_STAGES)
    assert ex_on["posted"][0] - ex_on["in_flight"] == ex_off["posted"][0]
    assert ex_on["posted"][1] == ex_off["posted"][1]
    assert close_to(u_on, u_off, 1e-12)
    for a, b in zip(g_on, g_off):
        assert close_to(a, b, 1e-12)


def test_download_of_a_stale_array_fails_with_the_option_switched_off():
    """the contract of the stale marks does not depend on the option: switched off right after a fused stage, a download of an
    array that stage kept on chip fails; the state it did produce downloads; a per-method stage then refreshes the gradient"""
    r = Rig("K1", True)
    e = r.blocks[0]
    r.stage(0, "inv")
    r.stage(0, "rest")
    r.ctx.set_option("deferred", 0)  # (runs the pending stage, fused)
    assert r.ctx.deferred_stats()[:2] == (1, 0)
    assert is_current(e, hfx.GRAD_DISU_UPTS) == 0
    with pytest.raises(hfx.HfxError, match="not materialised"):
        e.download(hfx.GRAD_DISU_UPTS)
    with pytest.raises(hfx.HfxError, match="not stored"):
        e.compute_res_upts(2, 0)
    assert relerr(e.download(hfx.DISU_UPTS0), r.ref(0)[0]) < RTOLS
    r.stage(1, "inv")
    r.stage(1, "rest")
    assert is_current(e, hfx.GRAD_DISU_UPTS) == 1
    g = e.download(hfx.GRAD_DISU_UPTS)
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    assert relerr(e.download(hfx.DISU_UPTS0), r.ref(1)[0]) < RTOLS
    r.close()


def test_destroy_runs_the_pending_stage():
    """RunSteps leaves the last stage of a run pending behind its AdvanceSolution: destroying an unrelated block then runs it
    (and reports its failure) instead of dropping it for every block of the context"""
    r = Rig("K1", True)
    r.stage(0, "inv")
    r.stage(0, "rest")
    x = r.new_eles()  # (created before the stage is recorded: its creation does not run it)
    r.stage(1, "inv")
    r.stage(1, "rest")
    x.close()
    assert r.ctx.deferred_stats()[:2] == (2, 0)
    assert relerr(r.state()[0], r.ref(1)[0]) < RTOLS
    r.close()
