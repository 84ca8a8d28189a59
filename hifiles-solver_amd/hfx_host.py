"""ctypes binding of libhfx_host.so (include/hfx_host.h): the host-side mirror of the reference's
eles / int_inters / solver interface.  Setup is host code; every per-stage call ends in libhfx."""
import ctypes as C
import os

import numpy as np

import hfx

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.environ.get("HFX_LIB_DIR", HERE), "libhfx_host.so")  # HFX_LIB_DIR: an A/B build (make variant)

dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)


class CaseDesc(C.Structure):
    _fields_ = [("dims", C.c_int), ("n", C.c_int * 3), ("order", C.c_int), ("length", C.c_double), ("amp", C.c_double),
                ("xv", dp), ("loc_1d_upts", dp),
                ("viscous", C.c_int), ("riemann_solve_type", C.c_int), ("adv_type", C.c_int), ("ic_form", C.c_int),
                ("upts_type", C.c_int), ("vcjh_scheme", C.c_int), ("eta", C.c_double), ("fix_vis", C.c_int),
                ("dt", C.c_double), ("ldg_beta", C.c_double), ("ldg_tau", C.c_double)] + \
               [(k, C.c_double) for k in ("gamma", "prandtl", "S_gas", "T_gas", "R_gas", "mu_gas",
                                          "Mach_free_stream", "rho_free_stream", "L_free_stream", "T_free_stream",
                                          "rho_c_ic", "Mach_c_ic", "T_c_ic", "u_c_ic", "v_c_ic", "w_c_ic", "p_c_ic")] + \
               [("rank", C.c_int), ("nproc", C.c_int), ("pgrid", C.c_int * 3),
                ("n_bcs", C.c_int), ("bcs", C.c_void_p), ("side_bc", C.c_int * 6),
                ("dt_type", C.c_int), ("CFL", C.c_double),
                ("over_int", C.c_int), ("over_int_order", C.c_int), ("shock_cap", C.c_int), ("shock_det_field", C.c_int),
                ("s0", C.c_double), ("expf_fac", C.c_double), ("expf_order", C.c_int), ("expf_cutoff", C.c_int),
                ("LES", C.c_int), ("SGS_model", C.c_int), ("C_s", C.c_double), ("filter_ratio", C.c_double),
                ("prandtl_t", C.c_double), ("p_res", C.c_int), ("self_partition", C.c_int * 3), ("filter_type", C.c_int),
                ("body_forcing", C.c_int), ("forcing_area", C.c_double), ("forcing_mdot0", C.c_double),
                ("nx_c_ic", C.c_double), ("ny_c_ic", C.c_double), ("nz_c_ic", C.c_double),
                ("calc_force", C.c_int), ("area_ref", C.c_double), ("monitor_cp_freq", C.c_int), ("wall_model", C.c_int)]


class BcDesc(C.Structure):
    """hfxh_bc_desc: one boundary group, dimensional inputs as in the reference's input file."""
    _fields_ = [("flag", C.c_int), ("pressure_ramp", C.c_int)] + \
               [(k, C.c_double) for k in ("rho", "u", "v", "w", "p_static", "T_static", "p_total", "T_total", "nx", "ny", "nz",
                                          "mach", "p_ramp_coeff", "T_ramp_coeff", "p_total_old", "T_total_old")] + \
               [("use_wm", C.c_int)]


BC_TYPES = {"sub_in_simp": 0, "sub_out_simp": 1, "sub_in_char": 2, "sub_out_char": 3, "sup_in": 4, "sup_out": 5,
            "slip_wall": 6, "cyclic": 7, "isotherm_wall": 8, "adiabat_wall": 9, "char": 10, "slip_wall_dual": 11}
SIDES3 = ("z-", "y-", "x+", "y+", "x-", "z+")  # element-local face numbers of a hex
SIDES2 = ("y-", "x+", "y+", "x-")

EXCHANGE_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int)
REDUCE_MIN_CB = C.CFUNCTYPE(C.c_double, C.c_void_p, C.c_double)
REDUCE_SUM_CB = C.CFUNCTYPE(None, C.c_void_p, dp, C.c_int)


# the shipped Taylor-Green case (/root/reference/testcases/navier-stokes/Taylor_Green_vortex/input_TGV_SD_hex)
TGV = dict(dims=3, order=4, length=6.2831853071795862, amp=0.0, viscous=1, riemann_solve_type=3, adv_type=3, ic_form=7,
           upts_type=0, vcjh_scheme=1, eta=0.0, fix_vis=1, dt=0.00001440389, ldg_beta=0.5, ldg_tau=0.0,
           gamma=1.4, prandtl=0.72, S_gas=120.0, T_gas=291.15, R_gas=286.9, mu_gas=1.827e-05,
           Mach_free_stream=0.1, rho_free_stream=0.0008421095852102401, L_free_stream=1.0, T_free_stream=300.0,
           rho_c_ic=0.0008421095852102401, Mach_c_ic=0.1, T_c_ic=300.0)

_lib = None


def lib():
    global _lib
    if _lib is None:
        hfx.lib()  # dependency, loaded first so that the rpath-less case also resolves
        if not os.path.exists(LIB_PATH):
            raise hfx.HfxError("libhfx_host.so is not built")
        _lib = C.CDLL(LIB_PATH)
        _lib.hfxh_last_error.restype = C.c_char_p
    return _lib


def check(rc):
    if rc != 0:
        raise hfx.HfxError(lib().hfxh_last_error().decode())


def norm_residual(res_norm_type, sums, n_upts):
    """the finish of output::CalcNormResidual (no device needed): the max / sums over blocks and ranks -> norm_residual; raises the
    reference's errors for an unknown norm type and a NaN norm"""
    s = np.ascontiguousarray(np.ravel(sums).astype(np.float64))
    out = np.zeros(max(1, len(s)))
    check(lib().hfxh_norm_residual(C.c_int(res_norm_type), C.c_int(len(s)), s.ctypes.data_as(dp), C.c_long(int(n_upts)),
                                   out.ctypes.data_as(dp)))
    return out[:len(s)]


def _locate(fn, handle, n_dims, positions):
    pos = np.asfortranarray(np.array(positions, dtype=np.float64).reshape((n_dims, -1), order="F"))
    n = pos.shape[1]
    p2c, loc = np.zeros(max(1, n), dtype=np.int32), np.zeros((n_dims, max(1, n)), order="F")
    check(fn(handle, C.c_int(n), pos.ctypes.data_as(dp), p2c.ctypes.data_as(ip), loc.ctypes.data_as(dp)))
    return p2c[:n].copy(), loc[:, :n].copy(order="F")


def _calc_pos(fn, handle, n_dims, ele, loc):
    el = np.ascontiguousarray(np.array(ele, dtype=np.int32).ravel())
    l = np.asfortranarray(np.array(loc, dtype=np.float64).reshape((n_dims, len(el)), order="F"))
    pos = np.zeros((n_dims, max(1, len(el))), order="F")
    check(fn(handle, C.c_int(len(el)), el.ctypes.data_as(ip), l.ctypes.data_as(dp), pos.ctypes.data_as(dp)))
    return pos[:, :len(el)].copy(order="F")


def _pos_to_loc(fn, handle, n_dims, ele, position):
    pos = np.ascontiguousarray(np.array(position, dtype=np.float64).ravel())
    loc = np.zeros(n_dims)
    check(fn(handle, C.c_int(int(ele)), pos.ctypes.data_as(dp), loc.ctypes.data_as(dp)))
    return loc


def _opp_probe(fn, handle, n_dims, n_upts, loc):
    l = np.asfortranarray(np.array(loc, dtype=np.float64).reshape((n_dims, -1), order="F"))
    out = np.zeros((n_upts, max(1, l.shape[1])), order="F")
    check(fn(handle, C.c_int(l.shape[1]), l.ctypes.data_as(dp), out.ctypes.data_as(dp)))
    return out[:, :l.shape[1]].copy(order="F")


class Case:
    def __init__(self, n, xv=None, loc_1d_upts=None, rank=0, pgrid=None, bcs=None, sides=None, self_partition=None, **kw):
        """n: cells per direction of THIS rank's block; pgrid: ranks per direction (None: one rank).
        bcs: list of boundary groups, each a dict with `type` (the reference's bc type name) and the type's
        dimensional parameters (rho,u,v,w,p_static,T_static,p_total,T_total,nx,ny,nz,mach,pressure_ramp,...);
        sides: {"x-": index into bcs, ...}; sides that are not listed are periodic."""
        d = CaseDesc()
        cfg = dict(TGV)
        cfg.update(kw)
        self._bcs = None
        if bcs:
            self._bcs = (BcDesc * len(bcs))()
            for i, b in enumerate(bcs):
                r = self._bcs[i]
                r.nx, r.T_total, r.T_total_old = 1.0, -1.0, -1.0
                for k, v in b.items():
                    if k == "type":
                        r.flag = BC_TYPES[v]
                    else:
                        setattr(r, k, v)
            d.n_bcs = len(bcs)
            d.bcs = C.cast(self._bcs, C.c_void_p)
            names = SIDES3 if cfg.get("dims", 3) == 3 else SIDES2
            for f in range(6):
                d.side_bc[f] = (sides or {}).get(names[f], -1) if f < len(names) else -1
        self.rank, self.pgrid = rank, (list(pgrid) if pgrid is not None else None)
        if pgrid is not None:
            d.rank, d.nproc = rank, int(np.prod(pgrid))
            for i in range(3):
                d.pgrid[i] = pgrid[i] if i < len(pgrid) else 1
        self.nproc = max(1, d.nproc)
        self.cfg = cfg
        for i, v in enumerate(self_partition or ()):
            d.self_partition[i] = int(v)
        for k, v in cfg.items():
            setattr(d, k, v)
        if isinstance(n, int):
            n = [n] * 3
        for i in range(3):
            d.n[i] = n[i] if i < len(n) else 1
        self._xv = None
        if xv is not None:
            self._xv = np.asfortranarray(np.array(xv, dtype=np.float64))
            d.xv = self._xv.ctypes.data_as(dp)
        self._x1 = None
        if loc_1d_upts is not None:
            self._x1 = np.ascontiguousarray(np.array(loc_1d_upts, dtype=np.float64))
            d.loc_1d_upts = self._x1.ctypes.data_as(dp)
        self.h = C.c_void_p()
        check(lib().hfxh_case_create(C.byref(d), C.byref(self.h)))
        sz = (C.c_int * 8)()
        check(lib().hfxh_case_sizes(self.h, sz))
        self.sizes = list(sz)
        self.n_eles, self.n_upts, self.n_fpts, self.n_fields, self.n_dims, self.order, self.ele_type, self.n_stages = self.sizes
        self.on_device = False

    def array(self, name):
        """Copy of a host array, Fortran-ordered with the reference's dims (trailing 1s dropped)."""
        p = dp()
        dims = (C.c_int * 4)()
        check(lib().hfxh_case_get_array(self.h, name.encode(), C.byref(p), dims))
        dims = list(dims)
        while len(dims) > 1 and dims[-1] == 1:
            dims.pop()
        n = int(np.prod(dims))
        a = np.ctypeslib.as_array(p, shape=(n,)).copy()
        return a.reshape(dims, order="F")

    def faces(self):
        L, R = ip(), ip()
        nf, ni = C.c_int(), C.c_int()
        check(lib().hfxh_case_get_faces(self.h, C.byref(L), C.byref(R), C.byref(nf), C.byref(ni)))
        n = nf.value * ni.value
        l = np.ctypeslib.as_array(L, shape=(n,)).copy().reshape((nf.value, ni.value), order="F")
        r = np.ctypeslib.as_array(R, shape=(n,)).copy().reshape((nf.value, ni.value), order="F")
        return l, r

    def bdy_faces(self):
        """(L, boundary_id) of the boundary-face block."""
        L, ids = ip(), ip()
        nf, ni = C.c_int(), C.c_int()
        check(lib().hfxh_case_get_bdy_faces(self.h, C.byref(L), C.byref(ids), C.byref(nf), C.byref(ni)))
        if ni.value == 0:
            return np.zeros((nf.value, 0), dtype=np.int32, order="F"), np.zeros(0, dtype=np.int32)
        n = nf.value * ni.value
        l = np.ctypeslib.as_array(L, shape=(n,)).copy().reshape((nf.value, ni.value), order="F")
        return l, np.ctypeslib.as_array(ids, shape=(ni.value,)).copy()

    def bc_list(self):
        """(flags (3,nbc), params (15,nbc), R_ref, ramp_counter): run_input.bc_list after non-dimensionalisation,
        in the fixtures' array form."""
        p = C.POINTER(hfx.Bc)()
        n, rc = C.c_int(), C.c_int()
        R = C.c_double()
        check(lib().hfxh_case_get_bcs(self.h, C.byref(p), C.byref(n), C.byref(R), C.byref(rc)))
        fl = np.zeros((3, n.value), dtype=np.int32, order="F")
        par = np.zeros((15, n.value), order="F")
        for b in range(n.value):
            r = p[b]
            fl[:, b] = (r.flag, r.pressure_ramp, r.use_wm)
            par[:, b] = [r.rho, r.velocity[0], r.velocity[1], r.velocity[2], r.p_static, r.T_static, r.p_total, r.T_total,
                         r.nx, r.ny, r.nz, r.p_ramp_coeff, r.T_ramp_coeff, r.p_total_old, r.T_total_old]
        return fl, par, R.value, rc.value

    def wall_model_points(self):
        """(wall_model, upt (n_inters), dist (n_inters), number of wall-model faces): the model's input point of every boundary
        face and its wall distance (0 on faces without a model), in the order of bdy_faces()"""
        wm, ni, nw = C.c_int(), C.c_int(), C.c_int()
        u, d = ip(), dp()
        check(lib().hfxh_case_get_wall_model_points(self.h, C.byref(wm), C.byref(u), C.byref(d), C.byref(ni), C.byref(nw)))
        if ni.value == 0:
            return wm.value, np.zeros(0, dtype=np.int32), np.zeros(0), 0
        return (wm.value, np.ctypeslib.as_array(u, shape=(ni.value,)).copy(), np.ctypeslib.as_array(d, shape=(ni.value,)).copy(),
                nw.value)

    def mpi_faces(self):
        """(L, Rlut, Nout_proc) of the partition-face block."""
        L, R, nout = ip(), ip(), ip()
        nf, ni = C.c_int(), C.c_int()
        check(lib().hfxh_case_get_mpi_faces(self.h, C.byref(L), C.byref(R), C.byref(nf), C.byref(ni), C.byref(nout)))
        n = nf.value * ni.value
        if n == 0:
            z = np.zeros((nf.value, 0), dtype=np.int32, order="F")
            return z, z.copy(), np.zeros(self.nproc, dtype=np.int32)
        l = np.ctypeslib.as_array(L, shape=(n,)).copy().reshape((nf.value, ni.value), order="F")
        r = np.ctypeslib.as_array(R, shape=(n,)).copy().reshape((nf.value, ni.value), order="F")
        return l, r, np.ctypeslib.as_array(nout, shape=(self.nproc,)).copy()

    def mpi_segments(self):
        """[(peer, send_first, recv_first, count)] of the partition-face block."""
        a = [ip(), ip(), ip(), ip()]
        n = C.c_int()
        check(lib().hfxh_case_get_mpi_segments(self.h, *[C.byref(x) for x in a], C.byref(n)))
        return [tuple(int(x[s]) for x in a) for s in range(n.value)]

    def set_reduce_min(self, fn):
        """fn(v) -> min over the ranks: calc_time_step's MPI_Allreduce(MIN) when the transport is the caller's"""
        self._rcb = REDUCE_MIN_CB(lambda user, v: float(fn(v)))
        check(lib().hfxh_case_set_reduce_min(self.h, self._rcb, None))

    def set_comm(self, unique_id):
        """collective: libhfx's own RCCL transport; unique_id = bytes from hfx.comm_unique_id() on rank 0"""
        if unique_id is None:  # back to the exchange / reduce hooks
            check(lib().hfxh_case_set_comm(self.h, None))
            return
        assert len(unique_id) == 128
        self._uid = C.create_string_buffer(bytes(unique_id), 128)
        check(lib().hfxh_case_set_comm(self.h, self._uid))

    def time_partitioned(self, reps):
        ms = (C.c_double * 8)()
        check(lib().hfxh_case_time_partitioned(self.h, C.c_int(reps), ms))
        return dict(zip(("phase1_interior_ldg", "phase2_gradient_flux", "phase3_interior_common_flux", "phase4_update",
                         "exchange_solution", "exchange_flux", "stage", "flux_kernel"), list(ms)[:8]))

    def comm_info(self):
        """what RCCL reports for the case's communicator: {nranks, rank, device, pci_bus_id}"""
        n, r, d = C.c_int(0), C.c_int(0), C.c_int(0)
        bus = C.create_string_buffer(32)
        check(lib().hfxh_case_comm_info(self.h, C.byref(n), C.byref(r), C.byref(d), bus))
        return {"nranks": n.value, "rank": r.value, "device": d.value, "pci_bus_id": bus.value.decode()}

    def set_exchange(self, fn):
        """fn(kind, phase): kind 0 solution / 1 corrected gradient, phase 0 start / 1 wait."""
        self._cb = EXCHANGE_CB(lambda user, kind, phase: fn(kind, phase))
        check(lib().hfxh_case_set_exchange(self.h, self._cb, None))

    def mpi_handle(self):
        f = C.c_void_p()
        check(lib().hfxh_case_mpi_handle(self.h, C.byref(f)))
        return f

    def set_deferred(self, on):
        """deferred execution of the mirrored method calls (default on): whole stages run as fused stages"""
        check(lib().hfxh_case_set_deferred(self.h, C.c_int(1 if on else 0)))

    def run_partitioned(self, n_steps):
        check(lib().hfxh_case_run_partitioned(self.h, C.c_int(n_steps)))

    def params(self):
        p = hfx.Params()
        check(lib().hfxh_case_params(self.h, C.byref(p)))
        return p

    def registration(self):
        """dict with the fixture key names (operators, metrics, faces, params) for the oracle / raw C ABI."""
        d = {"sizes": np.array(self.sizes, dtype=np.int32)}
        names = ["opp_0", "opp_3", "detjac_upts", "JGinv_upts", "detjac_fpts", "JGinv_fpts", "tdA_fpts", "norm_fpts"]
        p = self.params()
        if p.viscous:
            names.append("opp_6")
        for i in range(self.n_dims):
            names += ["opp_1_%d" % i, "opp_2_%d" % i] + (["opp_4_%d" % i, "opp_5_%d" % i] if p.viscous else [])
        for k in names:
            d[k] = self.array(k)
        L, R = self.faces()
        t = 2 if self.n_dims == 3 else 0
        d["int%d_L" % t], d["int%d_R" % t] = L, R
        bL, bid = self.bdy_faces()
        if bid.size:
            d["bdy%d_L" % t], d["bdy%d_id" % t] = bL, bid
            d["bc_flags"], d["bc_params"], R_ref, rc = self.bc_list()
            d["bc_R_ref"], d["ramp_counter"] = np.array([R_ref]), np.array([rc], dtype=np.int32)
        for k in ("gamma", "prandtl", "rt_inf", "mu_inf", "c_sth", "fix_vis", "ldg_beta", "ldg_tau", "dt",
                  "viscous", "riemann_solve_type", "vis_riemann_solve_type", "adv_type", "dt_type"):
            d[k] = np.array([getattr(p, k)], dtype=np.float64)
        d["RK_a"] = np.array(list(p.RK_a)[:p.n_rk])
        d["RK_b"] = np.array(list(p.RK_b)[:p.n_rk])
        d["u_init"] = self.array("disu_upts0")
        if self.cfg.get("LES", 0):
            # the closure's keys in the fixtures' form (oracle_py.Case, hfx.Eles.set_les); Kappa and prandtl_t: the
            # reference's defaults (src/input.cpp:176-180) unless given
            d["LES"] = np.array([1.0])
            d["SGS_model"] = np.array([float(self.cfg.get("SGS_model", 0))])
            d["C_s"] = np.array([float(self.cfg.get("C_s", 0.0))])
            d["filter_ratio"] = np.array([float(self.cfg.get("filter_ratio", 1.0))])
            d["Kappa"] = np.array([0.41])
            d["prandtl_t"] = np.array([float(self.cfg.get("prandtl_t", 0.0)) or 0.9])
            d["Jacobian_fpts"] = self.array("Jacobian_fpts")
            if int(self.cfg.get("SGS_model", 0)) >= 2:
                d["filter_upts"] = self.array("filter_upts")
        if self.cfg.get("over_int", 0):
            # over-integration in the fixtures' form (oracle_py.Case, hfx.Eles.set_over_int)
            d["over_int"] = np.array([1.0])
            for k in ("opp_over_int_cubpts", "over_int_filter", "JGinv_over_int_cubpts"):
                d[k] = self.array(k)
        if self.cfg.get("shock_cap", 0):
            # shock capturing likewise (oracle_py.Case, hfx.Eles.set_shock_capture)
            d["shock_cap"] = np.array([float(self.cfg["shock_cap"])])
            for k in ("inv_vandermonde", "exp_filter", "norm_basis_persson"):
                d[k] = self.array(k)
            d["persson_high_modes"] = self.array("persson_high_modes").astype(np.int32)
            d["s0"] = np.array([float(self.cfg.get("s0", 0.0))])
            d["shock_det_field"] = np.array([int(self.cfg.get("shock_det_field", 0))], dtype=np.int32)
        return d

    def to_device(self, device=0):
        check(lib().hfxh_case_to_device(self.h, C.c_int(device)))
        self.on_device = True

    def handles(self):
        ctx, e, f = C.c_void_p(), C.c_void_p(), C.POINTER(C.c_void_p)()
        nb = C.c_int()
        check(lib().hfxh_case_handles(self.h, C.byref(ctx), C.byref(e), C.byref(f), C.byref(nb)))
        return ctx, e, f, nb.value

    def CalcResidual(self):
        check(lib().hfxh_case_CalcResidual(self.h))

    def run(self, n_steps):
        check(lib().hfxh_case_run(self.h, C.c_int(n_steps)))

    def run_steps_lib(self, n_steps, fused=False):
        """hfx_run_steps on this case's device blocks (the whole RK loop inside libhfx)."""
        ctx, e, f, nb = self.handles()
        hfx.check(hfx.lib().hfx_run_steps(e, f, C.c_int(nb), C.c_int(n_steps), C.c_int(int(fused))))

    def synchronize(self):
        ctx, e, f, nb = self.handles()
        hfx.check(hfx.lib().hfx_ctx_synchronize(ctx))

    def stream(self):
        ctx, e, f, nb = self.handles()
        return hfx.lib().hfx_ctx_stream(ctx)

    def write_restart(self, directory, file_num):
        check(lib().hfxh_case_write_restart(self.h, str(directory).encode(), C.c_int(file_num)))

    def read_restart(self, directory, file_num, n_files=1):
        check(lib().hfxh_case_read_restart(self.h, str(directory).encode(), C.c_int(file_num), C.c_int(n_files)))

    def calc_time_step(self):
        v = C.c_double(0)
        check(lib().hfxh_case_calc_time_step(self.h, C.byref(v)))
        return v.value

    def calc_disu_ppts(self):
        """eles::calc_disu_ppts for every element: (n_ppts, n_eles, n_fields)"""
        ptr = dp()
        dims = (C.c_int * 3)()
        check(lib().hfxh_case_calc_disu_ppts(self.h, C.byref(ptr), dims))
        n = dims[0] * dims[1] * dims[2]
        return np.ctypeslib.as_array(ptr, shape=(n,)).reshape(tuple(dims), order="F").copy()

    def set_diagnostic_fields(self, names):
        """run_input.diagnostic_fields: names out of u, v, w, energy, mach, pressure, vorticity, q_criterion, scaled_q_criterion,
        sensor (any letter case)"""
        a = (C.c_char_p * max(1, len(names)))(*[n.encode() for n in names])
        check(lib().hfxh_case_set_diagnostic_fields(self.h, C.c_int(len(names)), a))

    def set_plot(self, plot_freq, capacity):
        """run_input.plot_freq and the snapshots the device history of the plot monitor holds (0: no monitor)"""
        check(lib().hfxh_case_set_plot(self.h, C.c_int(plot_freq), C.c_int(capacity)))

    def sample_plot(self):
        check(lib().hfxh_case_sample_plot(self.h))

    def plot_count(self):
        n = C.c_int(0)
        check(lib().hfxh_case_plot_count(self.h, C.byref(n)))
        return n.value

    def read_plot_rows(self):
        """(times (n), steps (n), rows (n, n_points, n_cols)): per snapshot the rows as write_tec prints them; empties the history"""
        ncol, npts = C.c_int(0), C.c_long(0)
        check(lib().hfxh_case_get_plot(self.h, None, None, C.byref(ncol), C.byref(npts)))
        ns = self.plot_count()
        times, steps = np.zeros(max(1, ns)), np.zeros(max(1, ns), dtype=np.int32)
        rows = np.zeros((max(1, ns), npts.value, ncol.value))
        got = C.c_int(0)
        check(lib().hfxh_case_read_plot_rows(self.h, C.c_int(ns), times.ctypes.data_as(dp), steps.ctypes.data_as(ip),
                                             rows.ctypes.data_as(dp), C.byref(got)))
        return times[:got.value].copy(), steps[:got.value].copy(), rows[:got.value].copy()

    def sync_host(self):
        check(lib().hfxh_case_sync_host(self.h))

    def set_average_fields(self, names):
        """run_input.average_fields: names out of rho_average, u_average, v_average, w_average, e_average (any letter case)"""
        a = (C.c_char_p * max(1, len(names)))(*[n.encode() for n in names])
        check(lib().hfxh_case_set_average_fields(self.h, C.c_int(len(names)), a))

    def average_fields(self):
        """the stored (lower-cased) names; their number is run_input.n_average_fields"""
        n = C.c_int(0)
        names = (C.c_char_p * 16)()
        check(lib().hfxh_case_get_average_fields(self.h, C.byref(n), names))
        return [names[i].decode() for i in range(n.value)]

    def _average_array(self, fn):
        ptr = dp()
        dims = (C.c_int * 3)()
        check(fn(self.h, C.byref(ptr), dims))
        n = dims[0] * dims[1] * dims[2]
        return np.ctypeslib.as_array(ptr, shape=(n,)).reshape(tuple(dims), order="F").copy()

    def averages(self):
        """disu_average_upts from the device: (n_upts, n_eles, n_average_fields)"""
        return self._average_array(lib().hfxh_case_get_averages)

    def calc_time_average_ppts(self):
        """eles::calc_time_average_ppts for every element: (n_ppts, n_eles, n_average_fields)"""
        return self._average_array(lib().hfxh_case_calc_time_average_ppts)

    def clock(self):
        """(time, i_steps, spinup_time) of the mirrored main loop"""
        t, n, s = C.c_double(0), C.c_int(0), C.c_double(0)
        check(lib().hfxh_case_get_clock(self.h, C.byref(t), C.byref(n), C.byref(s)))
        return t.value, n.value, s.value

    # ---- point probes
    def locate(self, positions):
        """calc_p2c + pos_to_loc of positions (n_dims, n): (p2c (n), -1 where no element holds the point; loc (n_dims, n))"""
        return _locate(lib().hfxh_case_locate, self.h, self.n_dims, positions)

    def calc_pos(self, ele, loc):
        """physical positions (n_dims, n) of the reference locations loc (n_dims, n) in the elements ele (n)"""
        return _calc_pos(lib().hfxh_case_calc_pos, self.h, self.n_dims, ele, loc)

    def pos_to_loc(self, ele, position):
        return _pos_to_loc(lib().hfxh_case_pos_to_loc, self.h, self.n_dims, ele, position)

    def opp_probe(self, loc):
        """eles::set_opp_probe at every column of loc (n_dims, n): (n_upts, n)"""
        return _opp_probe(lib().hfxh_case_opp_probe, self.h, self.n_dims, self.n_upts, loc)

    def set_probes(self, positions, fields, probe_freq=1, capacity=1):
        """positions (n_dims, n) physical; fields: the reference's names (rho, u, v, w, specific_total_energy, pressure)"""
        pos = np.asfortranarray(np.array(positions, dtype=np.float64).reshape((self.n_dims, -1), order="F"))
        a = (C.c_char_p * max(1, len(fields)))(*[f.encode() for f in fields])
        check(lib().hfxh_case_set_probes(self.h, C.c_int(pos.shape[1]), pos.ctypes.data_as(dp), C.c_int(len(fields)), a,
                                         C.c_int(probe_freq), C.c_int(capacity)))
        self.n_probe_fields = len(fields)

    def probes(self):
        """the located probes: dict(p2c, p2t, loc_probe (n_dims, n_located), global_index)"""
        n, p2c, p2t, loc, gi = C.c_int(0), ip(), ip(), dp(), ip()
        check(lib().hfxh_case_get_probes(self.h, C.byref(n), C.byref(p2c), C.byref(p2t), C.byref(loc), C.byref(gi)))
        k = n.value
        if k == 0:
            z = np.zeros(0, dtype=np.int32)
            return {"p2c": z, "p2t": z.copy(), "loc_probe": np.zeros((self.n_dims, 0)), "global_index": z.copy()}
        iarr = lambda p: np.ctypeslib.as_array(p, shape=(k,)).copy()
        return {"p2c": iarr(p2c), "p2t": iarr(p2t), "global_index": iarr(gi),
                "loc_probe": np.ctypeslib.as_array(loc, shape=(k * self.n_dims,)).copy().reshape((self.n_dims, k), order="F")}

    def sample_probes(self):
        check(lib().hfxh_case_sample_probes(self.h))

    def probe_count(self):
        ns, n = C.c_int(0), C.c_int(0)
        check(lib().hfxh_case_probe_count(self.h, C.byref(ns), C.byref(n)))
        return ns.value, n.value

    def read_probes(self, dimensional=False):
        """(times, steps, values (n_fields, n_located, n_samples)); dimensional: the reference factors of a viscous case"""
        ns, n = self.probe_count()
        times, steps = np.zeros(max(1, ns)), np.zeros(max(1, ns), dtype=np.int32)
        values = np.zeros((getattr(self, "n_probe_fields", 0), n, max(1, ns)), order="F")
        got = C.c_int(0)
        check(lib().hfxh_case_read_probes(self.h, C.c_int(1 if dimensional else 0), C.c_int(ns), times.ctypes.data_as(dp),
                                          steps.ctypes.data_as(ip), values.ctypes.data_as(dp), C.byref(got)))
        return times[:got.value].copy(), steps[:got.value].copy(), values[:, :, :got.value].copy(order="F")

    def ref_values(self):
        """dict(rho_ref, uvw_ref, p_ref, time_ref, viscous)"""
        v = (C.c_double * 5)()
        check(lib().hfxh_case_ref_values(self.h, v))
        return dict(zip(("rho_ref", "uvw_ref", "p_ref", "time_ref", "viscous"), list(v)))

    def forcing(self):
        """(body_forcing, forcing_area, forcing_mdot0) as the case holds them"""
        on, a, m = C.c_int(0), C.c_double(0), C.c_double(0)
        check(lib().hfxh_case_get_forcing(self.h, C.byref(on), C.byref(a), C.byref(m)))
        return on.value, a.value, m.value

    def set_forcing(self, area, mdot0):
        """new inflow area and target mass flux; on the device this registers again and resets the controller"""
        check(lib().hfxh_case_set_forcing(self.h, C.c_double(area), C.c_double(mdot0)))

    def set_reduce_sum(self, fn):
        """fn(list of n doubles) -> their sums over the ranks: the body force's MPI_Allreduce(SUM) when the transport is the caller's"""
        def cb(user, v, n):
            out = fn([v[i] for i in range(n)])
            for i in range(n):
                v[i] = float(out[i])
        self._scb = REDUCE_SUM_CB(cb)
        check(lib().hfxh_case_set_reduce_sum(self.h, self._scb, None))

    # ---- exact-solution error norms and integral diagnostics
    def set_test_case(self, test_case, error_norm_type=2):
        """run_input.test_case (0 none, 1 isentropic vortex, 5 Couette flow) and error_norm_type (1 L1, 2 L2)"""
        check(lib().hfxh_case_set_test_case(self.h, C.c_int(test_case), C.c_int(error_norm_type)))

    def test_case(self):
        """dict(test_case, error_norm_type, u_wall, T_wall): the walls as found among the boundary groups (test case 5)"""
        tc, nt, u, t = C.c_int(0), C.c_int(0), C.c_double(0), C.c_double(0)
        check(lib().hfxh_case_get_test_case(self.h, C.byref(tc), C.byref(nt), C.byref(u), C.byref(t)))
        return dict(test_case=tc.value, error_norm_type=nt.value, u_wall=u.value, T_wall=t.value)

    def set_integral_quantities(self, names):
        """run_input.integral_quantities: names out of kineticenergy, enstropy, pressuredilatation, straincolonproduct,
        devstraincolonproduct (any letter case)"""
        a = (C.c_char_p * max(1, len(names)))(*[n.encode() for n in names])
        check(lib().hfxh_case_set_integral_quantities(self.h, C.c_int(len(names)), a))
        self.n_integral_quantities = len(names)

    def set_monitor_res_freq(self, monitor_res_freq=100, capacity=0):
        """run_input.monitor_res_freq (0 means 1000) and the samples the integral monitor's device history holds (0: no monitor)"""
        check(lib().hfxh_case_set_monitor_res_freq(self.h, C.c_int(monitor_res_freq), C.c_int(capacity)))

    def monitor_res_freq(self):
        """(monitor_res_freq, capacity)"""
        f, n = C.c_int(0), C.c_int(0)
        check(lib().hfxh_case_get_monitor_res_freq(self.h, C.byref(f), C.byref(n)))
        return f.value, n.value

    def set_history(self, res_norm_type=2, capacity=0):
        """run_input.res_norm_type (0 infinity, 1 L1, 2 L2) and the rows the history monitor's device history holds (0: no monitor)"""
        check(lib().hfxh_case_set_history(self.h, C.c_int(res_norm_type), C.c_int(capacity)))

    def history(self):
        """(res_norm_type, capacity, columns of a row)"""
        t, n, k = C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().hfxh_case_get_history(self.h, C.byref(t), C.byref(n), C.byref(k)))
        return t.value, n.value, k.value

    def CalcNormResidual(self):
        """output::CalcNormResidual now, over blocks and ranks: norm_residual (n_fields)"""
        out = np.zeros(self.n_fields)
        check(lib().hfxh_case_CalcNormResidual(self.h, out.ctypes.data_as(dp)))
        return out

    def sample_history(self):
        check(lib().hfxh_case_sample_history(self.h))

    def history_count(self):
        n = C.c_int(0)
        check(lib().hfxh_case_history_count(self.h, C.byref(n)))
        return n.value

    def read_history(self):
        """(steps (n_rows), rows (n_cols, n_rows)): the rows of history.plt without the computing time; empties the histories"""
        ns, nc = self.history_count(), self.history()[2]
        steps, rows = np.zeros(max(1, ns), dtype=np.int32), np.zeros((nc, max(1, ns)), order="F")
        got, cols = C.c_int(0), C.c_int(0)
        check(lib().hfxh_case_read_history(self.h, C.c_int(ns), steps.ctypes.data_as(ip), rows.ctypes.data_as(dp), C.byref(cols),
                                           C.byref(got)))
        return steps[:got.value].copy(), rows[:, :got.value].copy(order="F")

    def sample_integral_quantities(self):
        check(lib().hfxh_case_sample_integral_quantities(self.h))

    def integral_count(self):
        n = C.c_int(0)
        check(lib().hfxh_case_integral_count(self.h, C.byref(n)))
        return n.value

    def read_integral_history(self):
        """(times, steps, values (n_integral_quantities, n_samples)): the rows of history.plt over blocks and ranks; empties the
        histories"""
        ns, nq = self.integral_count(), getattr(self, "n_integral_quantities", 0)
        times, steps = np.zeros(max(1, ns)), np.zeros(max(1, ns), dtype=np.int32)
        values = np.zeros((max(1, nq), max(1, ns)), order="F")
        got = C.c_int(0)
        check(lib().hfxh_case_read_integral_history(self.h, C.c_int(ns), times.ctypes.data_as(dp), steps.ctypes.data_as(ip),
                                                    values.ctypes.data_as(dp), C.byref(got)))
        return times[:got.value].copy(), steps[:got.value].copy(), values[:nq, :got.value].copy(order="F")

    def compute_error(self):
        """output::compute_error at the mirror's clock: (2, n_fields), over blocks and ranks, after the square root (norm 2)"""
        out = np.zeros((2, self.n_fields), dtype=np.float64, order="F")
        check(lib().hfxh_case_compute_error(self.h, out.ctypes.data_as(dp)))
        return out

    def CalcIntegralQuantities(self):
        out = np.zeros(max(1, getattr(self, "n_integral_quantities", 0)))
        check(lib().hfxh_case_CalcIntegralQuantities(self.h, out.ctypes.data_as(dp)))
        return out[:getattr(self, "n_integral_quantities", 0)]

    def inflow_faces(self):
        """(elements, local faces) the reference's inflow rule selects"""
        e, l, n = ip(), ip(), C.c_int(0)
        check(lib().hfxh_case_get_inflow_faces(self.h, C.byref(e), C.byref(l), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
        return (np.ctypeslib.as_array(e, shape=(n.value,)).copy(), np.ctypeslib.as_array(l, shape=(n.value,)).copy())

    def body_force_state(self):
        """the controller's record: dict(mass_flux, ubulk, body_force_x, accumulated (2), integral (2), n_steps)"""
        return hfx.body_force_state_of(lambda *a: check(lib().hfxh_case_body_force_state(self.h, *a)))

    def body_force_history(self, max_rows=4096):
        """rows (n, 3) of (mass_flux, ubulk, body_force(1)), oldest first: the columns of the reference's massflux.dat"""
        return hfx.body_force_history_of(lambda *a: check(lib().hfxh_case_body_force_history(self.h, *a)), max_rows)

    # ---- wall forces (calc_force=1, area_ref=..., monitor_cp_freq=... among the case's keys)
    def CalcForces(self):
        """output::CalcForces at the mirror's clock, over blocks and ranks: dict(inv_force (n_dims), vis_force (n_dims), cl, cd)"""
        fi, fv = (C.c_double * 3)(), (C.c_double * 3)()
        cl, cd = C.c_double(0), C.c_double(0)
        check(lib().hfxh_case_CalcForces(self.h, fi, fv, C.byref(cl), C.byref(cd)))
        return dict(inv_force=np.array(fi[:self.n_dims]), vis_force=np.array(fv[:self.n_dims]), cl=cl.value, cd=cd.value)

    def wall_points(self):
        """the rows of cp_*.dat: dict(ele, inter, flag, n_points (n_faces each), pos (n_dims, points), cp, cf (points; None
        before the first CalcForces)); faces in the reference's order, inside a face the cubature index descending"""
        n, e, l, fl, npts = C.c_int(0), ip(), ip(), ip(), ip()
        pos, cp, cf = dp(), dp(), dp()
        check(lib().hfxh_case_get_wall_points(self.h, C.byref(n), C.byref(e), C.byref(l), C.byref(fl), C.byref(npts), C.byref(pos),
                                              C.byref(cp), C.byref(cf)))
        k = n.value
        iarr = lambda p: np.ctypeslib.as_array(p, shape=(k,)).copy() if k else np.zeros(0, dtype=np.int32)
        out = dict(ele=iarr(e), inter=iarr(l), flag=iarr(fl), n_points=iarr(npts))
        tot = int(out["n_points"].sum())
        darr = lambda p, m: np.ctypeslib.as_array(p, shape=(m,)).copy() if (m and p) else None
        P = darr(pos, tot * self.n_dims)
        out["pos"] = np.zeros((self.n_dims, 0)) if P is None else P.reshape((self.n_dims, tot), order="F")
        out["cp"], out["cf"] = darr(cp, tot), darr(cf, tot)
        return out

    def calc_force(self):
        """dict(calc_force, area_ref (non-dimensional), monitor_cp_freq, rho_c_ic, u_c_ic, v_c_ic, w_c_ic, p_c_ic)"""
        on, a, m, r = C.c_int(0), C.c_double(0), C.c_int(0), (C.c_double * 5)()
        check(lib().hfxh_case_get_calc_force(self.h, C.byref(on), C.byref(a), C.byref(m), r))
        return dict(calc_force=on.value, area_ref=a.value, monitor_cp_freq=m.value, rho_c_ic=r[0], u_c_ic=r[1], v_c_ic=r[2],
                    w_c_ic=r[3], p_c_ic=r[4])

    def close(self):
        if self.h:
            lib().hfxh_case_destroy(self.h)
            self.h = C.c_void_p()


class Simplex:
    """eles_tets (ele_type 2) / eles_pris (3) of the host mirror as producers of operators and metrics for the given
    elements: shape (3, n_spts, n_eles), n_spts 4 / 6 (straight-sided) or 10 / 15 (quadratic)."""

    class Keys(C.Structure):
        _fields_ = [("vcjh_scheme", C.c_int), ("c", C.c_double), ("SGS_model", C.c_int), ("filter_type", C.c_int),
                    ("filter_ratio", C.c_double), ("shock_cap", C.c_int), ("expf_fac", C.c_double), ("expf_order", C.c_int),
                    ("expf_cutoff", C.c_int)]

    def __init__(self, ele_type, order, shape, viscous=1, loc_1d_upts=None, vcjh_scheme=1, c=0.0, SGS_model=-1, filter_type=0,
                 filter_ratio=1.0, shock_cap=0, expf_fac=36.0, expf_order=4, expf_cutoff=0):
        """vcjh_scheme: vcjh_scheme_tet / vcjh_scheme_tri (0: c given, 1 DG, 2 SD-like, 3 Huynh-like, 4 c+); SGS_model >= 0: a
        run with an LES closure (Jacobian_fpts, and filter_upts on tetrahedra for the closures that filter the solution);
        shock_cap 1: the shock-capturing operators (inv_vandermonde, exp_filter, norm_basis_persson, persson_high_modes)"""
        shp = np.asfortranarray(np.array(shape, dtype=np.float64))
        assert shp.shape[0] == 3 and shp.shape[1] in ((4, 10) if ele_type == 2 else (6, 15))
        x1 = None if loc_1d_upts is None else np.ascontiguousarray(np.array(loc_1d_upts, dtype=np.float64))
        self.h = C.c_void_p()
        k = Simplex.Keys(vcjh_scheme, c, SGS_model, filter_type, filter_ratio, shock_cap, expf_fac, expf_order, expf_cutoff)
        self.n_dims, self.n_eles = 3, shp.shape[2]
        check(lib().hfxh_simplex_create_keys(C.c_int(ele_type), C.c_int(order), C.c_int(viscous), C.c_int(shp.shape[2]),
                                             C.c_int(shp.shape[1]), shp.ctypes.data_as(dp), None if x1 is None else x1.ctypes.data_as(dp),
                                             C.byref(k), C.byref(self.h)))

    def array(self, name):
        p = dp()
        dims = (C.c_int * 4)()
        check(lib().hfxh_simplex_get_array(self.h, name.encode(), C.byref(p), dims))
        dims = list(dims)
        while len(dims) > 1 and dims[-1] == 1:
            dims.pop()
        n = int(np.prod(dims))
        return np.ctypeslib.as_array(p, shape=(n,)).copy().reshape(dims, order="F")

    def locate(self, positions):
        return _locate(lib().hfxh_simplex_locate, self.h, 3, positions)

    def calc_pos(self, ele, loc):
        return _calc_pos(lib().hfxh_simplex_calc_pos, self.h, 3, ele, loc)

    def pos_to_loc(self, ele, position):
        return _pos_to_loc(lib().hfxh_simplex_pos_to_loc, self.h, 3, ele, position)

    def opp_probe(self, loc):
        return _opp_probe(lib().hfxh_simplex_opp_probe, self.h, 3, self.array("loc_upts").shape[1], loc)

    def close(self):
        if self.h:
            lib().hfxh_simplex_destroy(self.h)
            self.h = C.c_void_p()
