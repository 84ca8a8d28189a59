"""The integral quantities of history.plt restated in numpy -- TEST INFRASTRUCTURE.

eles::CalcIntegralQuantities (src/eles.cpp:5485-5627): the state and the gradient interpolated to the volume cubature points, the
pointwise diagnostic (src/eles.cpp:5540-5620), times weight x detjac, summed.  The reference's two-dimensional forms are kept:
diag = (S00 + S11) / 3.0 in 2-D as in 3-D (src/eles.cpp:5594).

The sampling rule of the main loop (src/HiFiLES.cpp:247-266): after step i_steps when i_steps == 1 or i_steps %
monitor_res_freq == 0; monitor_res_freq defaults to 100 and 0 means 1000 (src/input.cpp:101,534-535).
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IH_DIR = os.path.join(GOLDEN, "integral_history")
NAMES = ["kineticenergy", "enstropy", "pressuredilatation", "straincolonproduct", "devstraincolonproduct"]
INTEGRALS = ["hex_p2_integrals", "quad_p3_integrals", "tet_p2_integrals", "pri_p2_integrals"]
IH = ["ih_hex_p2_rk45", "ih_hex_p2_euler", "ih_quad_p3_rk45", "ih_hex_p2_walls", "ih_tet_p2_rk45"]


def load(name):
    path = os.path.join(IH_DIR if name.startswith("ih_") else GOLDEN, name + ".npz")
    return dict(np.load(path))


def scalar(d, k):
    return float(np.ravel(d[k])[0])


def sample_step(i_steps, monitor_res_freq):
    return i_steps == 1 or i_steps % monitor_res_freq == 0


def sample_steps(i_steps, n_steps, monitor_res_freq):
    """the steps of a call of n_steps steps from i_steps after which the reference samples"""
    return [s for s in range(i_steps + 1, i_steps + n_steps + 1) if sample_step(s, monitor_res_freq)]


def quantities(ids, opp, weight, detjac, u, grad, gamma):
    """ids: 0-4; opp (n_cubpts, n_upts); weight (n_cubpts); detjac (n_cubpts, n_eles); u (n_upts, n_eles, n_fields);
    grad (n_upts, n_eles, n_fields, n_dims), or None with kinetic energy alone"""
    opp, u = np.asarray(opp, dtype=np.float64), np.asarray(u, dtype=np.float64)
    nf = u.shape[2]
    nd = nf - 2
    uc = np.einsum("jk,kif->jif", opp, u)
    irho = 1.0 / uc[..., 0]
    tke = sum(0.5 * uc[..., n] * uc[..., n] for n in range(1, nd + 1))
    if grad is not None:
        gc = np.einsum("jk,kifd->jifd", opp, np.asarray(grad, dtype=np.float64))
        # dv[i][j] = d u_i / d x_j
        dv = [[irho * (gc[..., i + 1, j] - uc[..., i + 1] * irho * gc[..., 0, j]) for j in range(nd)] for i in range(nd)]
    w = np.ravel(weight)[:, None] * np.asarray(detjac, dtype=np.float64)
    out = []
    for q in np.ravel(ids):
        q = int(q)
        assert q == 0 or grad is not None
        if q == 0:
            diag = irho * tke
        elif q == 1:
            diag = (dv[1][0] - dv[0][1]) ** 2
            if nd == 3:
                diag = diag + (dv[2][1] - dv[1][2]) ** 2 + (dv[0][2] - dv[2][0]) ** 2
            diag = diag * (0.5 / irho)
        elif q == 2:
            pressure = (gamma - 1.0) * (uc[..., nd + 1] - irho * tke)
            diag = pressure * sum(dv[a][a] for a in range(nd))
        elif q in (3, 4):
            S = [[dv[a][a] if a == b else (dv[a][b] + dv[b][a]) / 2.0 for b in range(nd)] for a in range(nd)]
            trace3 = sum(S[a][a] for a in range(nd)) / 3.0  # (/ 3.0 in two dimensions too)
            if q == 4:
                for a in range(nd):
                    S[a][a] = S[a][a] - trace3
            diag = sum(S[a][b] * S[a][b] for a in range(nd) for b in range(nd))
        else:
            raise ValueError("integral diagnostic quantity not recognized")
        out.append(float(np.sum(diag * w)))
    return np.array(out)


def fixture_quantities(d, u, grad, ids=None):
    return quantities(np.ravel(d["integral_quantity_ids"]) if ids is None else ids, d["opp_volume_cubpts"], d["weight_volume_cubpts"],
                      d["vol_detjac_vol_cubpts"], u, grad, scalar(d, "gamma"))


class OracleRun:
    """the oracle (tests/oracle_py.py) stepping a fixture's case: after step() u is the new state and grad what the last RK stage's
    correct_gradient left -- the gradient of that stage's input state"""

    def __init__(self, d):
        import ctypes as C
        import oracle_py as O
        self.C, self.O, self.o = C, O, O.load()
        self.case = O.Case(d)
        self.e, (self.f, self.nb) = self.case.c_eles(), self.case.c_faces()
        self.b, self.nbd = self.case.c_bdy() if self.case.bdy else (None, 0)

    def step(self):
        C, p = self.C, self.case.params
        if self.nbd:
            bad = self.o.orc_rk_step_bdy(C.byref(self.e), self.f, self.nb, self.b, self.nbd, C.byref(p))
        else:
            bad = self.o.orc_rk_step(C.byref(self.e), self.f, self.nb, C.byref(p))
        assert bad == -1, bad

    @property
    def u(self):
        return self.case.arr["u0"]

    @property
    def grad(self):
        return self.case.arr["grad_disu_upts"]

    def own_gradient(self):
        """the corrected gradient of the state as it stands (a residual on a copy; this run is left as it was)"""
        C = self.C
        saved = {k: v.copy(order="F") for k, v in self.case.arr.items()}
        if self.nbd:
            bad = self.o.orc_CalcResidual_bdy(C.byref(self.e), self.f, self.nb, self.b, self.nbd, C.byref(self.case.params))
        else:
            bad = self.o.orc_CalcResidual(C.byref(self.e), self.f, self.nb, C.byref(self.case.params))
        assert bad == -1, bad
        g = self.case.arr["grad_disu_upts"].copy(order="F")
        for k, v in saved.items():
            self.case.arr[k][...] = v
        return g
