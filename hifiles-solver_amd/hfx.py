"""ctypes binding of libhfx.so (the C ABI declared in include/hfx.h).

Plumbing only: every call goes straight to the HIP library; there is no CPU
fallback.  If the shared library is missing the import fails loudly.
"""
import ctypes as C
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.path.join(os.environ.get("HFX_LIB_DIR", HERE), "libhfx.so")  # HFX_LIB_DIR: an A/B build (make variant)
HEADER = os.path.join(ROOT, "include", "hfx.h")

dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)

(DISU_UPTS0, DISU_UPTS1, DISU_FPTS, TDISF_UPTS, NORM_TDISF_FPTS, NORM_TCONF_FPTS, DIV_TCONF_UPTS,
 DELTA_DISU_FPTS, GRAD_DISU_UPTS, GRAD_DISU_FPTS, SRC_UPTS, DT_LOCAL, SENSOR, SGSF_UPTS, SGSF_FPTS,
 DISUF_UPTS, LU, LE) = range(18)


# hfx_average_field: the reference's average_fields names in the order of their codes
AVG_RHO, AVG_U, AVG_V, AVG_W, AVG_E = range(5)
AVERAGE_NAMES = ("rho_average", "u_average", "v_average", "w_average", "e_average")

# hfx_probe_field: the reference's probe field names (src/output.cpp:1482-1522) in the order of their codes
PROBE_RHO, PROBE_U, PROBE_V, PROBE_W, PROBE_E, PROBE_P = range(6)
PROBE_NAMES = ("rho", "u", "v", "w", "specific_total_energy", "pressure")


class Les(C.Structure):
    _fields_ = [("sgs_model", C.c_int), ("pad", C.c_int), ("C_s", C.c_double), ("filter_ratio", C.c_double),
                ("Kappa", C.c_double), ("prandtl_t", C.c_double)]
CONTRACT_AUTO, CONTRACT_DENSE, CONTRACT_SPARSE = 0, 1, 2


class Exact(C.Structure):
    """hfx_exact: run_input.test_case and what the exact solution of Couette flow takes"""
    _fields_ = [("test_case", C.c_int), ("pad", C.c_int)] + \
               [(n, C.c_double) for n in ("u_wall", "T_wall", "p_bound", "R_ref", "T_ref")]


class Params(C.Structure):
    _fields_ = [(n, C.c_double) for n in
                ("gamma", "prandtl", "rt_inf", "mu_inf", "c_sth", "fix_vis", "ldg_beta", "ldg_tau", "dt")] + \
               [(n, C.c_int) for n in
                ("viscous", "riemann_solve_type", "vis_riemann_solve_type", "adv_type", "dt_type", "n_rk")] + \
               [("RK_a", C.c_double * 16), ("RK_b", C.c_double * 16)]


class ElesDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n_eles", "n_upts", "n_fpts", "n_fields", "n_dims", "ele_type", "order")] + [
        ("opp_0", dp), ("opp_1", dp * 3), ("opp_2", dp * 3), ("opp_3", dp), ("opp_4", dp * 3),
        ("opp_5", dp * 3), ("opp_6", dp),
        ("detjac_upts", dp), ("JGinv_upts", dp), ("detjac_fpts", dp), ("JGinv_fpts", dp),
        ("tdA_fpts", dp), ("norm_fpts", dp)]


class Bc(C.Structure):
    """hfx_bc: one entry of run_input.bc_list after non-dimensionalisation."""
    _fields_ = [(n, C.c_int) for n in ("flag", "pressure_ramp", "use_wm", "pad")] + \
               [("rho", C.c_double), ("velocity", C.c_double * 3)] + \
               [(n, C.c_double) for n in ("p_static", "T_static", "p_total", "T_total", "nx", "ny", "nz",
                                          "p_ramp_coeff", "T_ramp_coeff", "p_total_old", "T_total_old")]


(BC_SUB_IN_SIMP, BC_SUB_OUT_SIMP, BC_SUB_IN_CHAR, BC_SUB_OUT_CHAR, BC_SUP_IN, BC_SUP_OUT, BC_SLIP_WALL, BC_CYCLIC,
 BC_ISOTHERM_WALL, BC_ADIABAT_WALL, BC_CHAR, BC_SLIP_WALL_DUAL) = range(12)


def bc_records(flags, params):
    """Bc array from the fixture form: flags (3,nbc) = flag, pressure_ramp, use_wm; params (15,nbc) = rho, velocity[3],
    p_static, T_static, p_total, T_total, nx, ny, nz, p_ramp_coeff, T_ramp_coeff, p_total_old, T_total_old."""
    fl = np.asarray(flags).reshape(3, -1, order="F")
    par = np.asarray(params).reshape(15, -1, order="F")
    out = (Bc * fl.shape[1])()
    for b in range(fl.shape[1]):
        r = out[b]
        r.flag, r.pressure_ramp, r.use_wm = int(fl[0, b]), int(fl[1, b]), int(fl[2, b])
        q = par[:, b]
        r.rho = q[0]
        for d in range(3):
            r.velocity[d] = q[1 + d]
        (r.p_static, r.T_static, r.p_total, r.T_total, r.nx, r.ny, r.nz,
         r.p_ramp_coeff, r.T_ramp_coeff, r.p_total_old, r.T_total_old) = [float(v) for v in q[4:15]]
    return out


def declared_symbols():
    """Names of every function include/hfx.h declares."""
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(hfx_[A-Za-z0-9_]+)\s*\(", txt)))


class HfxError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HfxError("libhfx.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`)")
        _lib = C.CDLL(LIB_PATH)
        _lib.hfx_last_error.restype = C.c_char_p
        _lib.hfx_ctx_stream.restype = C.c_void_p
        _lib.hfx_ctx_stream.argtypes = [C.c_void_p]
    return _lib


def check(rc):
    if rc != 0:
        raise HfxError(lib().hfx_last_error().decode())


def _f(a):
    a = np.asfortranarray(np.array(a, dtype=np.float64))
    return a


def deferred_stats(ctx_handle):
    nf, nr, why = C.c_long(0), C.c_long(0), C.c_char_p()
    check(lib().hfx_ctx_deferred_stats(ctx_handle, C.byref(nf), C.byref(nr), C.byref(why)))
    return nf.value, nr.value, (why.value or b"").decode()


def fused_launch_grids(eles_handle):
    """[(slot, grid, work)] of the persistent element kernels since the block's last split fused stage began, in launch order
    (hfx_fused_launch_grids: slot 1 flux / gradient, 3 update / residual, 4 over-integration, 5 shock capturing)"""
    n, slot, grid, work = C.c_int(0), (C.c_int * 16)(), (C.c_int * 16)(), (C.c_long * 16)()
    check(lib().hfx_fused_launch_grids(eles_handle, C.c_int(16), slot, grid, work, C.byref(n)))
    return [(slot[i], grid[i], work[i]) for i in range(min(n.value, 16))]


def body_force_state_of(call):
    """call(mass_flux*, ubulk*, body_force_x*, accumulated*, integral*, n_steps*) -> the record as a dict"""
    m, u, f, n = C.c_double(0), C.c_double(0), C.c_double(0), C.c_long(0)
    acc, integ = (C.c_double * 2)(), (C.c_double * 2)()
    call(C.byref(m), C.byref(u), C.byref(f), acc, integ, C.byref(n))
    return {"mass_flux": m.value, "ubulk": u.value, "body_force_x": f.value, "accumulated": np.array(list(acc)),
            "integral": np.array(list(integ)), "n_steps": n.value}


def body_force_history_of(call, max_rows):
    """call(max_rows, rows*, n_rows*) -> (n, 3) array of (mass_flux, ubulk, body_force(1)), oldest first"""
    rows = np.zeros((3, max(1, max_rows)), dtype=np.float64, order="F")
    n = C.c_int(0)
    call(C.c_int(max_rows), rows.ctypes.data_as(dp), C.byref(n))
    return rows[:, :n.value].T.copy()


class ForceRef(C.Structure):
    """hfx_force_ref: the reference state of the wall-force monitor"""
    _fields_ = [(n, C.c_double) for n in ("rho_c_ic", "u_c_ic", "v_c_ic", "w_c_ic", "p_c_ic", "area_ref")]


def wall_forces_of(call, n_dims, n_points):
    """call(inv_force*, vis_force*, cl*, cd*, cp*, cf*) -> dict; n_points None: no per-point values asked for"""
    fi, fv = (C.c_double * 3)(), (C.c_double * 3)()
    cl, cd = C.c_double(0), C.c_double(0)
    out = {}
    if n_points is None:
        call(fi, fv, C.byref(cl), C.byref(cd), None, None)
    else:
        cp, cf = np.zeros(max(1, n_points)), np.zeros(max(1, n_points))
        call(fi, fv, C.byref(cl), C.byref(cd), cp.ctypes.data_as(dp), cf.ctypes.data_as(dp))
        out = {"cp": cp[:n_points], "cf": cf[:n_points]}
    out.update(inv_force=np.array(fi[:n_dims]), vis_force=np.array(fv[:n_dims]), cl=cl.value, cd=cd.value)
    return out


def set_probes_of(eles_handle, n_upts, ele, opp_probe):
    el = np.ascontiguousarray(np.array(ele, dtype=np.int32).ravel())
    opp = _f(np.array(opp_probe, dtype=np.float64).reshape((n_upts, len(el)), order="F"))
    check(lib().hfx_eles_set_probes(eles_handle, C.c_int(len(el)), el.ctypes.data_as(ip), opp.ctypes.data_as(dp)))


def probe_count_of(eles_handle):
    ns, n = C.c_int(0), C.c_int(0)
    check(lib().hfx_eles_probe_count(eles_handle, C.byref(ns), C.byref(n)))
    return ns.value, n.value


def read_probes_of(eles_handle, n_fields):
    ns, n = probe_count_of(eles_handle)
    times, steps = np.zeros(max(1, ns)), np.zeros(max(1, ns), dtype=np.int32)
    values = np.zeros((n_fields, n, max(1, ns)), order="F")
    got = C.c_int(0)
    check(lib().hfx_eles_read_probes(eles_handle, C.c_int(ns), times.ctypes.data_as(dp), steps.ctypes.data_as(ip),
                                     values.ctypes.data_as(dp), C.byref(got)))
    return times[:got.value].copy(), steps[:got.value].copy(), values[:, :, :got.value].copy(order="F")


INTEGRAL_NAMES = ["kineticenergy", "enstropy", "pressuredilatation", "straincolonproduct", "devstraincolonproduct"]


def integral_count_of(eles_handle):
    n = C.c_int(0)
    check(lib().hfx_eles_integral_count(eles_handle, C.byref(n)))
    return n.value


def read_integral_history_of(eles_handle, n_quantities):
    ns = integral_count_of(eles_handle)
    times, steps = np.zeros(max(1, ns)), np.zeros(max(1, ns), dtype=np.int32)
    values = np.zeros((max(1, n_quantities), max(1, ns)), order="F")
    got = C.c_int(0)
    check(lib().hfx_eles_read_integral_history(eles_handle, C.c_int(ns), times.ctypes.data_as(dp), steps.ctypes.data_as(ip),
                                               values.ctypes.data_as(dp), C.byref(got)))
    return times[:got.value].copy(), steps[:got.value].copy(), values[:n_quantities, :got.value].copy(order="F")


def history_count_of(eles_handle):
    n = C.c_int(0)
    check(lib().hfx_eles_history_count(eles_handle, C.byref(n)))
    return n.value


def read_history_of(eles_handle, n_fields, n_forces):
    ns = history_count_of(eles_handle)
    times, steps = np.zeros(max(1, ns)), np.zeros(max(1, ns), dtype=np.int32)
    res = np.zeros((n_fields, max(1, ns)), order="F")
    forces = np.zeros((n_forces, max(1, ns)), order="F")
    got = C.c_int(0)
    check(lib().hfx_eles_read_history(eles_handle, C.c_int(ns), times.ctypes.data_as(dp), steps.ctypes.data_as(ip),
                                      res.ctypes.data_as(dp), forces.ctypes.data_as(dp), C.byref(got)))
    n = got.value
    return times[:n].copy(), steps[:n].copy(), res[:, :n].copy(order="F"), forces[:, :n].copy(order="F")


PLOT_NAMES = ["u", "v", "w", "energy", "mach", "pressure", "vorticity", "q_criterion", "scaled_q_criterion", "sensor"]


def plot_count_of(eles_handle):
    n = C.c_int(0)
    check(lib().hfx_eles_plot_count(eles_handle, C.byref(n)))
    return n.value


def plot_width_of(eles_handle):
    n = C.c_int(0)
    check(lib().hfx_eles_plot_width(eles_handle, C.byref(n)))
    return n.value


def read_plot_snapshots_of(eles_handle, n_ppts, n_eles):
    """(times (n), steps (n), values (n_ppts, n_eles, n_fields + n_average + n_diag, n)); empties the history"""
    ns, width = plot_count_of(eles_handle), plot_width_of(eles_handle)
    times, steps = np.zeros(max(1, ns)), np.zeros(max(1, ns), dtype=np.int32)
    values = np.zeros((n_ppts, n_eles, width, max(1, ns)), order="F")
    got = C.c_int(0)
    check(lib().hfx_eles_read_plot_snapshots(eles_handle, C.c_int(ns), times.ctypes.data_as(dp), steps.ctypes.data_as(ip),
                                             values.ctypes.data_as(dp), C.byref(got)))
    return times[:got.value].copy(), steps[:got.value].copy(), values[..., :got.value].copy(order="F")


def plot_monitor_samples(i_steps, n_steps, plot_freq):
    """how many of the steps i_steps + 1 .. i_steps + n_steps the plot monitor samples (no device needed)"""
    n = C.c_int(0)
    check(lib().hfx_plot_monitor_samples(C.c_int(i_steps), C.c_int(n_steps), C.c_int(plot_freq), C.byref(n)))
    return n.value


def plot_point_fields(names, u, grad, gamma, sensor=0.0):
    """the kernel's pointwise formulas on the host at one plot point (no device needed): u (n_dims + 2), grad (n_dims + 2, n_dims) or
    None; the fields `names` in their order"""
    codes = [PLOT_NAMES.index(n.lower()) if isinstance(n, str) else int(n) for n in names]
    a = (C.c_int * max(1, len(codes)))(*codes)
    u = np.ascontiguousarray(np.array(u, dtype=np.float64))
    g = None if grad is None else _f(grad)
    out = np.zeros(max(1, len(codes)))
    check(lib().hfx_plot_point_fields(C.c_int(len(u) - 2), u.ctypes.data_as(dp), None if g is None else g.ctypes.data_as(dp),
                                      C.c_double(gamma), C.c_double(sensor), C.c_int(len(codes)), a, out.ctypes.data_as(dp)))
    return out[:len(codes)]


def integral_monitor_samples(i_steps, n_steps, monitor_res_freq):
    """how many of the steps i_steps + 1 .. i_steps + n_steps the integral monitor samples (no device needed)"""
    n = C.c_int(0)
    check(lib().hfx_integral_monitor_samples(C.c_int(i_steps), C.c_int(n_steps), C.c_int(monitor_res_freq), C.byref(n)))
    return n.value


class Context:
    def __init__(self, device=0):
        self.h = C.c_void_p()
        check(lib().hfx_ctx_create(C.c_int(device), C.byref(self.h)))

    def set_params(self, p):
        self.params = p
        check(lib().hfx_ctx_set_params(self.h, C.byref(p)))

    def set_fused_mode(self, mode):
        check(lib().hfx_ctx_set_fused_mode(self.h, C.c_int(mode)))

    def set_contract_mode(self, mode):
        check(lib().hfx_ctx_set_contract_mode(self.h, C.c_int(mode)))

    def set_option(self, name, value):
        check(lib().hfx_ctx_set_option(self.h, name.encode(), C.c_int(int(value))))

    def set_CFL(self, CFL):
        check(lib().hfx_ctx_set_CFL(self.h, C.c_double(CFL)))

    def set_wall_model(self, wall_model, prandtl_t=0.9, Kappa=0.41):
        """run_input.wall_model (0 off, 1 Werner-Wengle, 2 Breuer-Rodi); before the boundary blocks are made"""
        check(lib().hfx_ctx_set_wall_model(self.h, C.c_int(wall_model), C.c_double(prandtl_t), C.c_double(Kappa)))

    def get_dt(self):
        v = C.c_double(0)
        check(lib().hfx_ctx_get_dt(self.h, C.byref(v)))
        return v.value

    def synchronize(self):
        check(lib().hfx_ctx_synchronize(self.h))

    def set_clock(self, time, i_steps=0):
        """hands FlowSol.time and i_steps to the library: its step loops then advance them and update the time averages"""
        check(lib().hfx_ctx_set_clock(self.h, C.c_double(time), C.c_int(i_steps)))

    def set_spinup_time(self, spinup_time):
        check(lib().hfx_ctx_set_spinup_time(self.h, C.c_double(spinup_time)))

    def get_clock(self):
        """(time, i_steps, spinup_time)"""
        t, n, s = C.c_double(0), C.c_int(0), C.c_double(0)
        check(lib().hfx_ctx_get_clock(self.h, C.byref(t), C.byref(n), C.byref(s)))
        return t.value, n.value, s.value

    def set_probes(self, fields, probe_freq=1, capacity=1):
        """fields: PROBE_* codes or the reference's names (rho, u, v, w, specific_total_energy, pressure); [] drops them"""
        codes = [PROBE_NAMES.index(f.lower()) if isinstance(f, str) else int(f) for f in fields]
        a = (C.c_int * max(1, len(codes)))(*codes)
        check(lib().hfx_ctx_set_probes(self.h, C.c_int(len(codes)), a, C.c_int(probe_freq), C.c_int(capacity)))
        self.n_probe_fields = len(codes)

    def set_integral_monitor(self, quantities, monitor_res_freq=100, capacity=1):
        """quantities: ids 0-4 or the reference's names (kineticenergy, enstropy, pressuredilatation, straincolonproduct,
        devstraincolonproduct), in the order of the input file; [] drops the monitor"""
        ids = [INTEGRAL_NAMES.index(q.lower()) if isinstance(q, str) else int(q) for q in quantities]
        a = (C.c_int * max(1, len(ids)))(*ids)
        check(lib().hfx_ctx_set_integral_monitor(self.h, C.c_int(len(ids)), a, C.c_int(monitor_res_freq), C.c_int(capacity)))
        self.n_integral_quantities = len(ids)

    def set_history_monitor(self, res_norm_type=2, with_forces=False, monitor_res_freq=100, capacity=1):
        """the residual (and, with_forces, wall-force) columns of history.plt; capacity 0 drops the monitor"""
        check(lib().hfx_ctx_set_history_monitor(self.h, C.c_int(res_norm_type), C.c_int(1 if with_forces else 0),
                                                C.c_int(monitor_res_freq), C.c_int(capacity)))

    def set_plot_monitor(self, fields, plot_freq=1, capacity=1):
        """fields: PLOT_* codes or the reference's names (u, v, w, energy, mach, pressure, vorticity, q_criterion,
        scaled_q_criterion, sensor), in the order of the input file; [] plots the conserved fields (and averages) alone;
        capacity 0 drops the monitor"""
        codes = [PLOT_NAMES.index(f.lower()) if isinstance(f, str) else int(f) for f in fields]
        a = (C.c_int * max(1, len(codes)))(*codes)
        check(lib().hfx_ctx_set_plot_monitor(self.h, C.c_int(len(codes)), a, C.c_int(plot_freq), C.c_int(capacity)))

    def set_exact_solution(self, test_case, u_wall=0.0, T_wall=0.0, p_bound=0.0, R_ref=0.0, T_ref=0.0):
        """test_case 1: isentropic vortex; 5: Couette flow, which takes the five parameters (hfx_exact)"""
        x = Exact(int(test_case), 0, u_wall, T_wall, p_bound, R_ref, T_ref)
        check(lib().hfx_ctx_set_exact_solution(self.h, C.byref(x)))

    def set_force_reference(self, rho_c_ic, u_c_ic, v_c_ic, w_c_ic, p_c_ic, area_ref):
        """the reference state the wall forces are made coefficients with (hfx_force_ref)"""
        r = ForceRef(rho_c_ic, u_c_ic, v_c_ic, w_c_ic, p_c_ic, area_ref)
        check(lib().hfx_ctx_set_force_reference(self.h, C.byref(r)))

    def flush(self):
        """deferred execution: run what has been recorded (no-op otherwise)"""
        check(lib().hfx_ctx_flush(self.h))

    def deferred_stats(self):
        """(stages run fused, records replayed call by call, why the last replay was one)"""
        return deferred_stats(self.h)

    @property
    def stream(self):
        return lib().hfx_ctx_stream(self.h)

    def close(self):
        if self.h:
            lib().hfx_ctx_destroy(self.h)
            self.h = C.c_void_p()


class Eles:
    """One element block; `data` maps the names of hfx_eles_desc to numpy arrays (hf_array / Fortran order)."""

    def __init__(self, ctx, sizes, data, ele_type=4, order=0):
        self.ctx = ctx
        self.n_eles, self.n_upts, self.n_fpts, self.n_fields, self.n_dims = [int(s) for s in sizes]
        d = ElesDesc()
        d.n_eles, d.n_upts, d.n_fpts, d.n_fields, d.n_dims = self.n_eles, self.n_upts, self.n_fpts, self.n_fields, self.n_dims
        d.ele_type, d.order = ele_type, order
        keep = []

        def ptr(name):
            if name not in data:
                return None
            a = _f(data[name])
            keep.append(a)
            return a.ctypes.data_as(dp)

        d.opp_0 = ptr("opp_0"); d.opp_3 = ptr("opp_3"); d.opp_6 = ptr("opp_6")
        for i in range(self.n_dims):
            d.opp_1[i] = ptr("opp_1_%d" % i); d.opp_2[i] = ptr("opp_2_%d" % i)
            d.opp_4[i] = ptr("opp_4_%d" % i); d.opp_5[i] = ptr("opp_5_%d" % i)
        for k in ("detjac_upts", "JGinv_upts", "detjac_fpts", "JGinv_fpts", "tdA_fpts", "norm_fpts"):
            setattr(d, k, ptr(k))
        self.h = C.c_void_p()
        check(lib().hfx_eles_create(ctx.h, C.byref(d), C.byref(self.h)))
        nu, nfp, ne, nf, nd = self.n_upts, self.n_fpts, self.n_eles, self.n_fields, self.n_dims
        self.shapes = {
            DISU_UPTS0: (nu, ne, nf), DISU_UPTS1: (nu, ne, nf), DISU_FPTS: (nfp, ne, nf),
            TDISF_UPTS: (nu, ne, nf, nd), NORM_TDISF_FPTS: (nfp, ne, nf), NORM_TCONF_FPTS: (nfp, ne, nf),
            DIV_TCONF_UPTS: (nu, ne, nf), DELTA_DISU_FPTS: (nfp, ne, nf), GRAD_DISU_UPTS: (nu, ne, nf, nd),
            GRAD_DISU_FPTS: (nfp, ne, nf, nd), SRC_UPTS: (nu, ne, nf), DT_LOCAL: (ne,), SENSOR: (ne,),
            SGSF_UPTS: (nu, ne, nf, nd), SGSF_FPTS: (nfp, ne, nf, nd),
            DISUF_UPTS: (nu, ne, nf), LU: (nu, ne, 3 if nd == 2 else 6), LE: (nu, ne, nd)}

    def upload(self, array_id, a):
        a = _f(a)
        assert a.shape == self.shapes[array_id], (a.shape, self.shapes[array_id])
        check(lib().hfx_eles_upload(self.h, C.c_int(array_id), a.ctypes.data_as(dp)))

    def download(self, array_id):
        a = np.zeros(self.shapes[array_id], dtype=np.float64, order="F")
        check(lib().hfx_eles_download(self.h, C.c_int(array_id), a.ctypes.data_as(dp)))
        return a

    def device_ptr(self, array_id):
        p = dp()
        check(lib().hfx_eles_device_ptr(self.h, C.c_int(array_id), C.byref(p)))
        return C.cast(p, C.c_void_p).value

    def _call(self, name, *args):
        check(getattr(lib(), name)(self.h, *args))

    def set_opp_p(self, opp_p):
        a = _f(opp_p)
        self.n_ppts = a.shape[0]
        check(lib().hfx_eles_set_opp_p(self.h, C.c_int(a.shape[0]), a.ctypes.data_as(dp)))

    def calc_disu_ppts(self):
        out = np.zeros((self.n_ppts, self.n_eles, self.n_fields), dtype=np.float64, order="F")
        check(lib().hfx_eles_calc_disu_ppts(self.h, out.ctypes.data_as(dp)))
        return out

    def set_average_fields(self, fields):
        """fields: AVG_* codes or the reference's names (rho_average ...), in the order of the input file; [] drops them"""
        codes = [AVERAGE_NAMES.index(f.lower()) if isinstance(f, str) else int(f) for f in fields]
        a = (C.c_int * max(1, len(codes)))(*codes)
        check(lib().hfx_eles_set_average_fields(self.h, C.c_int(len(codes)), a))
        self.n_average_fields = len(codes)

    def upload_average(self, a):
        a = _f(a)
        assert a.shape == (self.n_upts, self.n_eles, getattr(self, "n_average_fields", 0)), a.shape
        check(lib().hfx_eles_upload_average(self.h, a.ctypes.data_as(dp)))

    def download_average(self):
        a = np.zeros((self.n_upts, self.n_eles, getattr(self, "n_average_fields", 0)), dtype=np.float64, order="F")
        check(lib().hfx_eles_download_average(self.h, a.ctypes.data_as(dp)))
        return a

    def CalcTimeAverageQuantities(self, time, spinup_time):
        self._call("hfx_eles_CalcTimeAverageQuantities", C.c_double(time), C.c_double(spinup_time))

    def calc_time_average_ppts(self):
        out = np.zeros((self.n_ppts, self.n_eles, self.n_average_fields), dtype=np.float64, order="F")
        check(lib().hfx_eles_calc_time_average_ppts(self.h, out.ctypes.data_as(dp)))
        return out

    def set_probes(self, ele, opp_probe):
        """ele (n_probes): the element of each probe; opp_probe (n_upts, n_probes): its operator row as a column"""
        return set_probes_of(self.h, self.n_upts, ele, opp_probe)

    def sample_probes(self, time, step):
        self._call("hfx_eles_sample_probes", C.c_double(time), C.c_int(step))

    def probe_count(self):
        """(stored samples, registered probes)"""
        return probe_count_of(self.h)

    def read_probes(self):
        """(times (n_samples), steps (n_samples), values (n_fields, n_probes, n_samples)); empties the history"""
        return read_probes_of(self.h, getattr(self.ctx, "n_probe_fields", 0))

    def time_probes(self, reps=20):
        v = C.c_double(0)
        check(lib().hfx_time_probes(self.h, C.c_int(reps), C.byref(v)))
        return v.value

    def set_body_force(self, face_ele, face_inter, opp_inters_cubpts, weight_inters_cubpts, inter_detjac_inters_cubpts, area, mdot0,
                       history_capacity=64):
        """hfx_eles_set_body_force.  face_ele, face_inter: the inflow faces as (element, local face); opp_inters_cubpts[l]
        (n_cubpts, n_upts) and weight_inters_cubpts[l] (n_cubpts) per local face l (None for faces nobody names);
        inter_detjac_inters_cubpts: one array of n_cubpts values per listed face, in list order."""
        fe = np.ascontiguousarray(np.array(face_ele, dtype=np.int32).ravel())
        fl = np.ascontiguousarray(np.array(face_inter, dtype=np.int32).ravel())
        nl = len(opp_inters_cubpts)
        opp = [None if a is None else _f(a) for a in opp_inters_cubpts]
        wgt = [None if a is None else np.ascontiguousarray(np.array(a, dtype=np.float64).ravel()) for a in weight_inters_cubpts]
        ncub = (C.c_int * max(1, nl))(*[0 if a is None else a.shape[0] for a in opp])
        po = (dp * max(1, nl))(*[None if a is None else a.ctypes.data_as(dp) for a in opp])
        pw = (dp * max(1, nl))(*[None if a is None else a.ctypes.data_as(dp) for a in wgt])
        dj = np.ascontiguousarray(np.concatenate([np.array(a, dtype=np.float64).ravel() for a in inter_detjac_inters_cubpts])
                                  if len(fe) else np.zeros(1))
        check(lib().hfx_eles_set_body_force(self.h, C.c_int(len(fe)), fe.ctypes.data_as(ip), fl.ctypes.data_as(ip), C.c_int(nl), ncub,
                                            po, pw, dj.ctypes.data_as(dp), C.c_double(area), C.c_double(mdot0),
                                            C.c_int(history_capacity)))

    def clear_body_force(self): self._call("hfx_eles_clear_body_force")
    def evaluate_body_force(self): self._call("hfx_eles_evaluate_body_force")

    def body_force_integrals(self):
        v = (C.c_double * 2)()
        check(lib().hfx_eles_body_force_integrals(self.h, v))
        return [v[0], v[1]]

    def body_force_apply(self, integral):
        check(lib().hfx_eles_body_force_apply(self.h, (C.c_double * 2)(*[float(x) for x in integral])))

    def body_force_state(self):
        """dict(mass_flux, ubulk, body_force_x, accumulated (2), integral (2), n_steps); raises on the NaN flag"""
        return body_force_state_of(lambda *a: check(lib().hfx_eles_body_force_state(self.h, *a)))

    def body_force_history(self, max_rows=64):
        """(n, 3): mass_flux, ubulk, body_force(1) of the newest evaluations, oldest first"""
        return body_force_history_of(lambda *a: check(lib().hfx_eles_body_force_history(self.h, *a)), max_rows)

    def set_wall_faces(self, face_ele, face_inter, face_flag, opp_inters_cubpts, weight_inters_cubpts, inter_detjac_inters_cubpts,
                       norm_inters_cubpts):
        """hfx_eles_set_wall_faces.  face_ele, face_inter, face_flag: the wall faces as (element, local face, BC_* flag);
        opp_inters_cubpts[l] (n_cubpts, n_upts) and weight_inters_cubpts[l] (n_cubpts) per local face l (None for faces nobody
        names); per listed face, in list order, inter_detjac_inters_cubpts (n_cubpts) and norm_inters_cubpts (n_cubpts, n_dims)."""
        fe, fl, ff = [np.ascontiguousarray(np.array(a, dtype=np.int32).ravel()) for a in (face_ele, face_inter, face_flag)]
        nl = len(opp_inters_cubpts)
        opp = [None if a is None else _f(a) for a in opp_inters_cubpts]
        wgt = [None if a is None else np.ascontiguousarray(np.array(a, dtype=np.float64).ravel()) for a in weight_inters_cubpts]
        ncub = (C.c_int * max(1, nl))(*[0 if a is None else a.shape[0] for a in opp])
        po = (dp * max(1, nl))(*[None if a is None else a.ctypes.data_as(dp) for a in opp])
        pw = (dp * max(1, nl))(*[None if a is None else a.ctypes.data_as(dp) for a in wgt])
        cat = lambda parts: np.ascontiguousarray(np.concatenate(parts) if len(parts) else np.zeros(1))
        dj = cat([np.array(a, dtype=np.float64).ravel() for a in inter_detjac_inters_cubpts])
        nm = cat([_f(a).ravel(order="F") for a in norm_inters_cubpts])
        check(lib().hfx_eles_set_wall_faces(self.h, C.c_int(len(fe)), fe.ctypes.data_as(ip), fl.ctypes.data_as(ip), ff.ctypes.data_as(ip),
                                            C.c_int(nl), ncub, po, pw, dj.ctypes.data_as(dp), nm.ctypes.data_as(dp)))
        self.n_wall_points = int(sum(ncub[l] for l in fl))

    def clear_wall_faces(self): self._call("hfx_eles_clear_wall_faces")

    def compute_wall_forces(self, points=True):
        """eles::compute_wall_forces of this block: dict(inv_force (n_dims), vis_force (n_dims), cl, cd) and, with `points`,
        cp and cf (one value per listed face and cubature point, the caller's order)"""
        return wall_forces_of(lambda *a: check(lib().hfx_eles_compute_wall_forces(self.h, *a)), self.n_dims,
                              getattr(self, "n_wall_points", 0) if points else None)

    def wall_force_launch(self):
        """(workgroups, faces per pass) of the next compute_wall_forces"""
        g, n = C.c_int(0), C.c_int(0)
        check(lib().hfx_eles_wall_force_launch(self.h, C.byref(g), C.byref(n)))
        return g.value, n.value

    def time_wall_forces(self, reps=20):
        v = C.c_double(0)
        check(lib().hfx_time_wall_forces(self.h, C.c_int(reps), C.byref(v)))
        return v.value

    def extrapolate_solution(self): self._call("hfx_eles_extrapolate_solution")
    def calculate_gradient(self): self._call("hfx_eles_calculate_gradient")
    def evaluate_invFlux(self): self._call("hfx_eles_evaluate_invFlux")
    def correct_gradient(self): self._call("hfx_eles_correct_gradient")
    def evaluate_viscFlux(self): self._call("hfx_eles_evaluate_viscFlux")
    def extrapolate_totalFlux(self): self._call("hfx_eles_extrapolate_totalFlux")
    def calculate_divergence(self): self._call("hfx_eles_calculate_divergence")
    def calculate_corrected_divergence(self): self._call("hfx_eles_calculate_corrected_divergence")

    def AdvanceSolution(self, in_step, adv_type):
        self._call("hfx_eles_AdvanceSolution", C.c_int(in_step), C.c_int(adv_type))

    def set_shock_capture(self, inv_vandermonde, exp_filter, norm_basis_persson, high_modes, s0, shock_det_field):
        a, b = _f(inv_vandermonde), _f(exp_filter)
        n = np.ascontiguousarray(np.ravel(norm_basis_persson).astype(np.float64))
        h = np.ascontiguousarray(np.ravel(high_modes).astype(np.int32))
        check(lib().hfx_eles_set_shock_capture(self.h, a.ctypes.data_as(dp), b.ctypes.data_as(dp), n.ctypes.data_as(dp),
                                               h.ctypes.data_as(ip), C.c_double(s0), C.c_int(shock_det_field)))

    def shock_capture(self): self._call("hfx_eles_shock_capture")

    def set_les(self, sgs_model, C_s, filter_ratio, Kappa, prandtl_t, Jacobian_fpts, wall_distance=None, filter_upts=None):
        les = Les(sgs_model, 0, C_s, filter_ratio, Kappa, prandtl_t)
        J = _f(Jacobian_fpts)
        w = _f(wall_distance) if wall_distance is not None else None
        check(lib().hfx_eles_set_les(self.h, C.byref(les), w.ctypes.data_as(dp) if w is not None else None, J.ctypes.data_as(dp)))
        if filter_upts is not None:
            F = _f(filter_upts)
            assert F.shape == (self.n_upts, self.n_upts)
            check(lib().hfx_eles_set_les_filter(self.h, F.ctypes.data_as(dp)))

    def calc_sgs_terms(self): self._call("hfx_eles_calc_sgs_terms")

    def extrapolate_sgsFlux(self): self._call("hfx_eles_extrapolate_sgsFlux")

    def set_volume_cubpts(self, opp_volume_cubpts, weight_volume_cubpts, vol_detjac_vol_cubpts):
        a, d = _f(opp_volume_cubpts), _f(vol_detjac_vol_cubpts)
        w = np.ascontiguousarray(np.ravel(weight_volume_cubpts).astype(np.float64))
        check(lib().hfx_eles_set_volume_cubpts(self.h, C.c_int(a.shape[0]), a.ctypes.data_as(dp), w.ctypes.data_as(dp),
                                               d.ctypes.data_as(dp)))

    def CalcIntegralQuantities(self, ids):
        ids = np.ascontiguousarray(np.array(ids, dtype=np.int32))
        out = np.zeros(len(ids))
        check(lib().hfx_eles_CalcIntegralQuantities(self.h, C.c_int(len(ids)), ids.ctypes.data_as(ip), out.ctypes.data_as(dp)))
        return out

    def sample_integral_quantities(self, time, step):
        """one sample of the context's integral monitor into the block's device history (no synchronisation)"""
        self._call("hfx_eles_sample_integral_quantities", C.c_double(time), C.c_int(step))

    def integral_count(self):
        return integral_count_of(self.h)

    def read_integral_history(self):
        """(times (n_samples), steps (n_samples), values (n_quantities, n_samples)); empties the history"""
        return read_integral_history_of(self.h, getattr(self.ctx, "n_integral_quantities", 0))

    def integral_launch(self):
        """(workgroups, elements per pass) of the next sample"""
        g, n = C.c_int(0), C.c_int(0)
        check(lib().hfx_eles_integral_launch(self.h, C.byref(g), C.byref(n)))
        return g.value, n.value

    def general_plan(self):
        """the launch forms of the general fused stage on this block (hfx_general_plan), valid after a fused-4 call: dict of
        size_class, flux_waves, flux_batched, gather, les, update_waves, fold, flux_lds"""
        out = (C.c_int * 8)()
        check(lib().hfx_general_plan(self.h, out))
        return dict(zip(("size_class", "flux_waves", "flux_batched", "gather", "les", "update_waves", "fold", "flux_lds"), list(out)))

    def tensor_ops_plan(self):
        """over-integration and shock capturing on this block (hfx_eles_tensor_ops_plan): dict of over_int (1: factored), N, Nc,
        folded, shock (1: factored), shock_N, over_int_ran, shock_ran (the form of the last call: 1 sum-factorised, 0 dense, -1 none)"""
        out = (C.c_int * 8)()
        check(lib().hfx_eles_tensor_ops_plan(self.h, out))
        return dict(zip(("over_int", "N", "Nc", "folded", "shock", "shock_N", "over_int_ran", "shock_ran"), list(out)))

    def simplex2d_plan(self):
        """the form of the 2-D simplex fused stage on this block of triangles (hfx_simplex2d_plan), valid after a fused-4 call: dict of
        size_class, group, waves, gather, element_lds, update_lds"""
        out = (C.c_int * 8)()
        check(lib().hfx_simplex2d_plan(self.h, out))
        return dict(zip(("size_class", "group", "waves", "gather", "element_lds", "update_lds"), list(out)))

    def simplex2d_partition_plan(self):
        """what the partitioned loop runs on this block of triangles (hfx_simplex2d_partition_plan): dict of partition_groups,
        interior_groups, gather_remote"""
        out = (C.c_int * 4)()
        check(lib().hfx_simplex2d_partition_plan(self.h, out))
        return dict(zip(("partition_groups", "interior_groups", "gather_remote"), list(out)))

    def simplex2d_shock_plan(self):
        """shock capturing on this block of triangles in the 2-D simplex fused stage (hfx_simplex2d_shock_plan), valid after a fused-4
        call: dict of folded, update_lds (of the update kernel that runs), first_high_mode, launches_behind"""
        out = (C.c_int * 4)()
        check(lib().hfx_simplex2d_shock_plan(self.h, out))
        return dict(zip(("folded", "update_lds", "first_high_mode", "launches_behind"), list(out)))

    def simplex2d_over_int_plan(self):
        """over-integration on this block of triangles in the 2-D simplex fused stage (hfx_simplex2d_over_int_plan), valid after a
        fused-4 call: dict of folded, n_cubpts, chunk, chunks, element_lds, launches_in_front"""
        out = (C.c_int * 8)()
        check(lib().hfx_simplex2d_over_int_plan(self.h, out))
        return dict(zip(("folded", "n_cubpts", "chunk", "chunks", "element_lds", "launches_in_front"), list(out)))

    def simplex2d_les_plan(self):
        """an LES closure on this block of triangles in the 2-D simplex fused stage (hfx_simplex2d_les_plan), valid after a fused-4
        call: dict of les (the element kernel's LES form runs), sgs_model (-1: none), reads_leonard (Lu / Le), launches_in_front (of a
        step's first stage: those of calc_sgs_terms), element_lds"""
        out = (C.c_int * 8)()
        check(lib().hfx_simplex2d_les_plan(self.h, out))
        return dict(zip(("les", "sgs_model", "reads_leonard", "launches_in_front", "element_lds"), list(out)))

    def time_integral_quantities(self, reps=20):
        v = C.c_double(0)
        check(lib().hfx_time_integral_quantities(self.h, C.c_int(reps), C.byref(v)))
        return v.value

    def sample_plot(self, time, step):
        """one snapshot of the context's plot monitor into the block's device history (no synchronisation)"""
        self._call("hfx_eles_sample_plot", C.c_double(time), C.c_int(step))

    def plot_count(self):
        return plot_count_of(self.h)

    def read_plot_snapshots(self):
        """(times (n), steps (n), values (n_ppts, n_eles, n_fields + n_average + n_diag, n)); empties the history"""
        return read_plot_snapshots_of(self.h, self.n_ppts, self.n_eles)

    def calc_plot_fields(self):
        """one snapshot of the state as it stands, (n_ppts, n_eles, n_fields + n_average + n_diag); the history is untouched"""
        out = np.zeros((self.n_ppts, self.n_eles, plot_width_of(self.h)), dtype=np.float64, order="F")
        check(lib().hfx_eles_calc_plot_fields(self.h, out.ctypes.data_as(dp)))
        return out

    def plot_launch(self):
        """(workgroups, elements per pass, plot points of an element per pass of the lanes) of the next snapshot"""
        g, n, p = C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().hfx_eles_plot_launch(self.h, C.byref(g), C.byref(n), C.byref(p)))
        return g.value, n.value, p.value

    def time_plot_fields(self, reps=20):
        v = C.c_double(0)
        check(lib().hfx_time_plot_fields(self.h, C.c_int(reps), C.byref(v)))
        return v.value

    def sample_history(self, time, step):
        """one row of the context's history monitor into the block's device history (no synchronisation)"""
        self._call("hfx_eles_sample_history", C.c_double(time), C.c_int(step))

    def history_count(self):
        return history_count_of(self.h)

    def read_history(self):
        """(times (n_rows), steps (n_rows), residuals (n_fields, n_rows), forces (2 n_dims + 2, n_rows)): the block's raw values;
        empties the history"""
        return read_history_of(self.h, self.n_fields, 2 * self.n_dims + 2)

    def history_launch(self):
        """(workgroups, solution points per pass) of the residual kernel of the next sample"""
        g, n = C.c_int(0), C.c_int(0)
        check(lib().hfx_eles_history_launch(self.h, C.byref(g), C.byref(n)))
        return g.value, n.value

    def time_history(self, reps=20):
        v = C.c_double(0)
        check(lib().hfx_time_history(self.h, C.c_int(reps), C.byref(v)))
        return v.value

    def set_error_points(self, pos_volume_cubpts):
        """pos_volume_cubpts (n_cubpts, n_eles, n_dims): the positions of the cubature points of set_volume_cubpts"""
        a = _f(pos_volume_cubpts)
        assert a.ndim == 3 and a.shape[1:] == (self.n_eles, self.n_dims), a.shape
        check(lib().hfx_eles_set_error_points(self.h, a.ctypes.data_as(dp)))

    def compute_error(self, norm_type, time):
        """eles::compute_error of this block: (2, n_fields), row 0 the solution error, row 1 the gradient error, before the
        sum over blocks and ranks and the square root"""
        out = np.zeros((2, self.n_fields), dtype=np.float64, order="F")
        check(lib().hfx_eles_compute_error(self.h, C.c_int(norm_type), C.c_double(time), out.ctypes.data_as(dp)))
        return out

    def error_launch(self):
        """(workgroups, elements per pass) of the next compute_error"""
        g, n = C.c_int(0), C.c_int(0)
        check(lib().hfx_eles_error_launch(self.h, C.byref(g), C.byref(n)))
        return g.value, n.value

    def set_h_ref(self, h_ref):
        h = np.ascontiguousarray(np.ravel(h_ref).astype(np.float64))
        check(lib().hfx_eles_set_h_ref(self.h, h.ctypes.data_as(dp)))

    def calc_dt_local(self, CFL):
        v = C.c_double(0)
        check(lib().hfx_eles_calc_dt_local(self.h, C.c_double(CFL), C.byref(v)))
        return v.value

    def set_over_int(self, opp_over_int_cubpts, over_int_filter, JGinv_over_int_cubpts):
        a, b, c = _f(opp_over_int_cubpts), _f(over_int_filter), _f(JGinv_over_int_cubpts)
        assert a.shape == (b.shape[1], self.n_upts) and b.shape[0] == self.n_upts
        check(lib().hfx_eles_set_over_int(self.h, C.c_int(a.shape[0]), a.ctypes.data_as(dp), b.ctypes.data_as(dp),
                                          c.ctypes.data_as(dp)))

    def evaluate_invFlux_over_int(self): self._call("hfx_eles_evaluate_invFlux_over_int")

    def check_nan(self):
        v = C.c_long(0)
        check(lib().hfx_eles_check_nan(self.h, C.byref(v)))
        return v.value

    def compute_res_upts(self, norm_type, field):
        v = C.c_double(0)
        check(lib().hfx_eles_compute_res_upts(self.h, C.c_int(norm_type), C.c_int(field), C.byref(v)))
        return v.value

    def close(self):
        if self.h:
            lib().hfx_eles_destroy(self.h)
            self.h = C.c_void_p()


class IntInters:
    def __init__(self, ctx, left, right, L, R):
        L = np.asfortranarray(np.array(L, dtype=np.int32))
        R = np.asfortranarray(np.array(R, dtype=np.int32))
        self.n_fpts_per_inter, self.n_inters = L.shape
        self.h = C.c_void_p()
        check(lib().hfx_int_inters_create(ctx.h, left.h, right.h, C.c_int(self.n_inters), C.c_int(self.n_fpts_per_inter),
                                          L.ctypes.data_as(ip), R.ctypes.data_as(ip), C.byref(self.h)))

    def calculate_common_invFlux(self): check(lib().hfx_int_inters_calculate_common_invFlux(self.h))
    def calculate_common_viscFlux(self): check(lib().hfx_int_inters_calculate_common_viscFlux(self.h))

    def close(self):
        if self.h:
            lib().hfx_inters_destroy(self.h)
            self.h = C.c_void_p()


class BdyInters:
    """Boundary-face block (bdy_inters): left side only, ghost state from the group's record."""

    def __init__(self, ctx, left, L, boundary_id, bcs, R_ref, ramp_counter=0):
        L = np.asfortranarray(np.array(L, dtype=np.int32))
        ids = np.ascontiguousarray(np.array(boundary_id, dtype=np.int32).ravel())
        self.n_fpts_per_inter, self.n_inters = L.shape
        self.h = C.c_void_p()
        check(lib().hfx_bdy_inters_create(ctx.h, left.h, C.c_int(self.n_inters), C.c_int(self.n_fpts_per_inter),
                                          L.ctypes.data_as(ip), ids.ctypes.data_as(ip), bcs, C.c_int(len(bcs)),
                                          C.c_double(R_ref), C.byref(self.h)))
        if ramp_counter:
            check(lib().hfx_bdy_inters_set_ramp_counter(self.h, C.c_int(ramp_counter)))

    def set_ramp_counter(self, ramp_counter):
        check(lib().hfx_bdy_inters_set_ramp_counter(self.h, C.c_int(ramp_counter)))

    def set_wall_model_points(self, upt, dist):
        """the wall model's input point (a solution point of the face's own element) and its wall distance, per face"""
        upt = np.ascontiguousarray(np.array(upt, dtype=np.int32).ravel())
        dist = np.ascontiguousarray(np.array(dist, dtype=np.float64).ravel())
        if len(upt) != self.n_inters or len(dist) != self.n_inters:
            raise HfxError("set_wall_model_points: %d faces, %d points, %d distances" % (self.n_inters, len(upt), len(dist)))
        check(lib().hfx_bdy_inters_set_wall_model_points(self.h, upt.ctypes.data_as(ip), dist.ctypes.data_as(dp)))

    def wall_model_faces(self):
        n = C.c_int(0)
        check(lib().hfx_bdy_inters_wall_model_faces(self.h, C.byref(n)))
        return n.value

    def evaluate_boundaryConditions_invFlux(self, time=0.0):
        check(lib().hfx_bdy_inters_evaluate_boundaryConditions_invFlux(self.h, C.c_double(time)))

    def evaluate_boundaryConditions_viscFlux(self, time=0.0):
        check(lib().hfx_bdy_inters_evaluate_boundaryConditions_viscFlux(self.h, C.c_double(time)))

    def close(self):
        if self.h:
            lib().hfx_inters_destroy(self.h)
            self.h = C.c_void_p()


class MpiInters:
    """Partition-face block (mpi_inters): one-sided faces whose right state arrives in in_buffer_*."""

    def __init__(self, ctx, left, L, Rlut):
        L = np.asfortranarray(np.array(L, dtype=np.int32))
        Rlut = np.asfortranarray(np.array(Rlut, dtype=np.int32))
        self.n_fpts_per_inter, self.n_inters = L.shape
        self.h = C.c_void_p()
        check(lib().hfx_mpi_inters_create(ctx.h, left.h, C.c_int(self.n_inters), C.c_int(self.n_fpts_per_inter),
                                          L.ctypes.data_as(ip), Rlut.ctypes.data_as(ip), C.byref(self.h)))

    def pack_solution(self): check(lib().hfx_mpi_inters_pack_solution(self.h))
    def pack_corrected_gradient(self): check(lib().hfx_mpi_inters_pack_corrected_gradient(self.h))
    def calculate_common_invFlux(self): check(lib().hfx_mpi_inters_calculate_common_invFlux(self.h))
    def calculate_common_viscFlux(self): check(lib().hfx_mpi_inters_calculate_common_viscFlux(self.h))

    def buffer(self, which):
        """(device pointer, doubles) of 0 out_buffer_disu, 1 in_buffer_disu, 2 out_buffer_grad_disu, 3 in_buffer_grad_disu."""
        return mpi_buffer(self.h, which)

    def set_neighbours(self, segments):
        """segments: [(peer, send_first, recv_first, count)] (hfx_mpi_inters_set_neighbours)"""
        a = [np.ascontiguousarray([s[i] for s in segments], dtype=np.int32) for i in range(4)]
        check(lib().hfx_mpi_inters_set_neighbours(self.h, C.c_int(len(segments)), *[x.ctypes.data_as(ip) for x in a]))

    # mpi_inters::send_* / receive_* over libhfx's RCCL transport (comm: hfx.Comm)
    def send_solution(self, comm): check(lib().hfx_mpi_inters_send_solution(self.h, comm.h))
    def receive_solution(self, comm): check(lib().hfx_mpi_inters_receive_solution(self.h, comm.h))
    def send_corrected_gradient(self, comm): check(lib().hfx_mpi_inters_send_corrected_gradient(self.h, comm.h))
    def receive_corrected_gradient(self, comm): check(lib().hfx_mpi_inters_receive_corrected_gradient(self.h, comm.h))
    def send_sgsf_fpts(self, comm): check(lib().hfx_mpi_inters_send_sgsf_fpts(self.h, comm.h))
    def receive_sgsf_fpts(self, comm): check(lib().hfx_mpi_inters_receive_sgsf_fpts(self.h, comm.h))

    def close(self):
        if self.h:
            lib().hfx_inters_destroy(self.h)
            self.h = C.c_void_p()


def CalcResidual_blocks(eles, faces):
    """hfx_CalcResidual_blocks: several element blocks (a mixed mesh), face blocks between any two of them"""
    ea = (C.c_void_p * len(eles))(*[e.h for e in eles])
    fa = (C.c_void_p * max(1, len(faces)))(*[f.h for f in faces])
    check(lib().hfx_CalcResidual_blocks(ea, C.c_int(len(eles)), fa, C.c_int(len(faces))))


def run_steps_blocks(eles, faces, n_steps, fused=0):
    ea = (C.c_void_p * len(eles))(*[e.h for e in eles])
    fa = (C.c_void_p * max(1, len(faces)))(*[f.h for f in faces])
    check(lib().hfx_run_steps_blocks(ea, C.c_int(len(eles)), fa, C.c_int(len(faces)), C.c_int(n_steps), C.c_int(int(fused))))


def simplex2d_stage_plan(eles):
    """hfx_simplex2d_stage_plan: what one stage of the 2-D simplex fused stage launches over these blocks (the list of the fused-4 call
    that prepared them): dict of blocks, interior_face_blocks, cross_face_blocks, delta_launches, launches"""
    ea = (C.c_void_p * len(eles))(*[e.h for e in eles])
    out = (C.c_int * 8)()
    check(lib().hfx_simplex2d_stage_plan(ea, C.c_int(len(eles)), out))
    return dict(zip(("blocks", "interior_face_blocks", "cross_face_blocks", "delta_launches", "launches"), list(out)))


def time_general_kernels(eles, faces, reps=10):
    """hfx_time_general_kernels: (ms[8], the comma-separated kernel names) of the fused-4 stage on these blocks"""
    ea = (C.c_void_p * len(eles))(*[e.h for e in eles])
    fa = (C.c_void_p * max(1, len(faces)))(*[f.h for f in faces])
    ms, names = (C.c_double * 8)(), (C.c_char * 256)()
    check(lib().hfx_time_general_kernels(ea, C.c_int(len(eles)), fa, C.c_int(len(faces)), C.c_int(reps), ms, names))
    return list(ms), names.value.decode()


def general_kernel_bytes(eles):
    """hfx_general_kernel_bytes: algorithmic HBM bytes per launch, in the order of time_general_kernels"""
    ea = (C.c_void_p * len(eles))(*[e.h for e in eles])
    by = (C.c_double * 8)()
    check(lib().hfx_general_kernel_bytes(ea, C.c_int(len(eles)), by))
    return list(by)


def flush_for_samples(eles, integrals=False, history=False, plot=False):
    """hfx_flush_for_samples: deferred execution, before the first reader of a step -- the pending record runs so that what the
    named samples of these blocks read is in memory"""
    ea = (C.c_void_p * len(eles))(*[e.h for e in eles])
    check(lib().hfx_flush_for_samples(ea, C.c_int(len(eles)), C.c_int((1 if integrals else 0) | (2 if history else 0) | (4 if plot else 0))))


def run_steps_partitioned_blocks(eles, int_faces, mpi_faces, comm, n_steps):
    """hfx_run_steps_partitioned_blocks: the general fused stage on partitioned element blocks"""
    ea = (C.c_void_p * len(eles))(*[e.h for e in eles])
    fa = (C.c_void_p * max(1, len(int_faces)))(*[f.h for f in int_faces])
    ma = (C.c_void_p * max(1, len(mpi_faces)))(*[f.h for f in mpi_faces])
    check(lib().hfx_run_steps_partitioned_blocks(ea, C.c_int(len(eles)), fa, C.c_int(len(int_faces)), ma, C.c_int(len(mpi_faces)), comm.h,
                                                 C.c_int(n_steps)))


def comm_unique_id():
    """128 bytes for hfx_comm_create (ncclGetUniqueId): made on rank 0, distributed by the launcher."""
    b = C.create_string_buffer(128)
    check(lib().hfx_comm_get_unique_id(b))
    return b.raw


class Comm:
    """libhfx's RCCL communicator of one rank (hfx_comm_create is collective over the ranks)."""

    def __init__(self, ctx_handle, unique_id, nranks, rank):
        self.h = C.c_void_p()
        self._uid = C.create_string_buffer(bytes(unique_id), 128)
        check(lib().hfx_comm_create(ctx_handle, self._uid, C.c_int(nranks), C.c_int(rank), C.byref(self.h)))

    def allreduce(self, values, op):
        """op: "min" | "max" | "sum"; returns the reduced list"""
        a = (C.c_double * len(values))(*values)
        check(lib().hfx_comm_allreduce(self.h, a, C.c_int(len(values)), C.c_int({"min": 0, "max": 1, "sum": 2}[op])))
        return list(a)

    def exchange_stats(self):
        """-> {posted: [3], waited: [3], in_flight, stream_busy} (hfx_comm_exchange_stats): messages of kind 0 (solution),
        1 (gradient / projected flux), 2 (SGS flux) counted per partition-face block"""
        posted, waited = (C.c_long * 3)(), (C.c_long * 3)()
        in_flight, busy = C.c_int(0), C.c_int(0)
        check(lib().hfx_comm_exchange_stats(self.h, posted, waited, C.byref(in_flight), C.byref(busy)))
        return {"posted": list(posted), "waited": list(waited), "in_flight": in_flight.value, "stream_busy": busy.value}

    def close(self):
        if self.h:
            lib().hfx_comm_destroy(self.h)
            self.h = C.c_void_p()


def mpi_buffer(handle, which):
    p = dp()
    n = C.c_size_t(0)
    check(lib().hfx_mpi_inters_buffer(handle, C.c_int(which), C.byref(p), C.byref(n)))
    return C.cast(p, C.c_void_p).value, n.value


def stage_partitioned(eles_h, int_faces, mpi_faces, phase, in_step, first):
    """hfx_stage_partitioned on raw handles (lists of c_void_p)."""
    fi = (C.c_void_p * max(1, len(int_faces)))(*int_faces)
    fm = (C.c_void_p * max(1, len(mpi_faces)))(*mpi_faces)
    check(lib().hfx_stage_partitioned(eles_h, fi, C.c_int(len(int_faces)), fm, C.c_int(len(mpi_faces)),
                                      C.c_int(phase), C.c_int(in_step), C.c_int(first)))


def _face_array(faces):
    arr = (C.c_void_p * max(1, len(faces)))()
    for i, f in enumerate(faces):
        arr[i] = f.h
    return arr


def CalcResidual(eles, faces):
    check(lib().hfx_CalcResidual(eles.h, _face_array(faces), C.c_int(len(faces))))


def run_steps(eles, faces, n_steps, fused=False):
    check(lib().hfx_run_steps(eles.h, _face_array(faces), C.c_int(len(faces)), C.c_int(n_steps), C.c_int(int(fused))))


def _jacobi_normalized(x, alpha, beta, n):
    """the orthonormal Jacobi polynomial P_n^(alpha, beta) at x by its three-term recurrence (eval_jacobi, src/funcs.cpp:1245)"""
    import math
    x = np.asarray(x, dtype=np.float64)
    g = lambda m: float(math.factorial(m - 1))  # (Gamma at a positive integer: eval_gamma)
    p0 = math.sqrt(2.0 ** (-alpha - beta - 1) * g(alpha + beta + 2) / (g(alpha + 1) * g(beta + 1))) * np.ones_like(x)
    if n == 0:
        return p0
    p1 = 0.5 * p0 * math.sqrt((alpha + beta + 3.0) / ((alpha + 1.0) * (beta + 1.0))) * (x * (alpha + beta + 2) + (alpha - beta))

    def a(m):
        return 2.0 / (2 * m + alpha + beta) * math.sqrt(m * (m + alpha + beta) * (m + alpha) * (m + beta) / ((2 * m + alpha + beta - 1.0) * (2 * m + alpha + beta + 1.0)))

    for m in range(2, n + 1):
        b = -(alpha * alpha - beta * beta) / ((2 * (m - 1) + alpha + beta) * (2 * (m - 1) + alpha + beta + 2.0))
        p0, p1 = p1, ((x - b) * p1 - a(m - 1) * p0) / a(m)
    return p1


def tri_shock_operators(loc_upts, order, expf_fac, expf_order, expf_cutoff):
    """What a block of triangles registers for shock capturing (Eles.set_shock_capture), built as eles_tris does (set_vandermonde,
    set_exp_filter, shock_det_persson; src/eles_tris.cpp:432-524) from the solution points loc_upts (2, n_upts) of the reference
    triangle: the orthonormal Dubiner basis (eval_dubiner_basis_2d, src/funcs.cpp:1318), modes by total degree k = 0..order and
    within k by j = 0..k (i = k - j); sigma = 1 for k / order <= expf_cutoff / order, else exp(-expf_fac ((eta - eta_c) / (1 - eta_c))
    ^ expf_order).  -> (inv_vandermonde, exp_filter, norm_basis_persson (ones), high_modes (1 for the modes of degree `order`)).
    Host set-up only: nothing on the stepping path calls it."""
    r, s = np.asarray(loc_upts, dtype=np.float64).reshape(2, -1)
    nu = (order + 1) * (order + 2) // 2
    assert r.size == nu, (r.size, nu)
    a = np.where(s == 1.0, -1.0, 2.0 * (1.0 + r) / np.where(s == 1.0, 1.0, 1.0 - s) - 1.0)  # rs_to_ab
    V = np.zeros((nu, nu))
    sigma = np.zeros(nu)
    high = np.zeros(nu, dtype=np.int32)
    eta_c = float(expf_cutoff) / float(order)
    mode = 0
    for k in range(order + 1):
        for j in range(k + 1):
            i = k - j
            V[:, mode] = np.sqrt(2.0) * _jacobi_normalized(a, 0, 0, i) * _jacobi_normalized(s, 2 * i + 1, 0, j) * (1.0 - s) ** i
            eta = float(k) / float(order)
            sigma[mode] = 1.0 if eta <= eta_c else np.exp(-expf_fac * ((eta - eta_c) / (1.0 - eta_c)) ** expf_order)
            high[mode] = int(k == order)
            mode += 1
    Vinv = np.linalg.inv(V)
    return np.asfortranarray(Vinv), np.asfortranarray(V @ (sigma[:, None] * Vinv)), np.ones(nu), high


def params_from(data):
    """hfx Params from a dict holding the scalar names of the fixtures / host setup."""
    s = lambda k, dflt=0.0: float(np.ravel(data[k])[0]) if k in data else dflt
    p = Params()
    for k in ("gamma", "prandtl", "rt_inf", "mu_inf", "c_sth", "fix_vis", "ldg_beta", "ldg_tau", "dt"):
        setattr(p, k, s(k))
    for k in ("viscous", "riemann_solve_type", "vis_riemann_solve_type", "adv_type", "dt_type"):
        setattr(p, k, int(s(k)))
    ra, rb = np.ravel(data["RK_a"]), np.ravel(data["RK_b"])
    p.n_rk = len(ra)
    for i in range(len(ra)):
        p.RK_a[i] = float(ra[i])
        p.RK_b[i] = float(rb[i])
    return p
