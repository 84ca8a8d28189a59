"""What the error-norm tests share (tests/test_gpu_error_norm.py, tests/test_error_norm_host.py): the yardstick, a numpy
restatement in np.longdouble of eles::compute_error / get_pointwise_error (src/eles.cpp:5076-5277) and of the two exact
solutions eval_isentropic_vortex (src/funcs.cpp:1724-1739) and eval_couette_flow (src/funcs.cpp:1830-1922), applied to exactly
the arrays the device gets; and the bar.

The bar is derived, not measured: for field m the norms are compared after the square root (norm 2) or as sums (norm 1), and
    |got - want| <= 1e-12 (||exact_m|| + ||interpolated_m||)      in the same norm,
for the solution row and for the gradient row alike.  Both sides round `interpolated - exact` at a few ulp of the operands
times at most n_upts terms, about 1e-14 of that scale; 1e-12 leaves two orders of margin.  A bar relative to `want` would be
wrong where the error is a small difference of large values.
"""
import numpy as np

LD = np.longdouble
BAR = 1e-12
PI = LD(np.pi)  # the reference's double constant


def exact_vortex(pos, time, gamma, n_dims):
    """pos (..., n_dims) -> the conservative state (..., n_dims + 2); eps = 5, the centre moves with (t, t), vz = 0"""
    pos = np.asarray(pos, dtype=LD)
    g, eps = LD(gamma), LD(5.0)
    x, y = pos[..., 0] - LD(time), pos[..., 1] - LD(time)
    f = 1 - (x * x + y * y)
    rho = (1 - eps * eps * (g - 1) / (8 * g * PI * PI) * np.exp(f)) ** (1 / (g - 1))
    vx = 1 - eps * y / (2 * PI) * np.exp(f / 2)
    vy = 1 + eps * x / (2 * PI) * np.exp(f / 2)
    p = rho ** g
    out = np.zeros(pos.shape[:-1] + (n_dims + 2,), dtype=LD)
    out[..., 0] = rho
    out[..., 1] = rho * vx
    out[..., 2] = rho * vy
    out[..., n_dims + 1] = p / (g - 1) + LD(0.5) * rho * (vx * vx + vy * vy)
    return out


def exact_couette(pos, gamma, prandtl, u_wall, T_wall, p_bound, R_ref, T_ref, n_dims):
    """pos (..., n_dims) -> state (..., n_fields), gradient (..., n_fields, n_dims).  Channel height 1.  The reference fills
    d(rho)/dy, d(rho u)/dy and dE/dy and leaves every other exact gradient zero (src/funcs.cpp:1898-1921)."""
    pos = np.asarray(pos, dtype=LD)
    g, R, uw, Tw, ps, pr = [LD(v) for v in (gamma, R_ref, u_wall, T_wall, p_bound, prandtl)]
    y = pos[..., 1]
    cp = (g * R) / (g - 1)
    vx = uw * y
    ka = 1 / LD(T_ref)
    kb = LD(0.5) * (pr / cp) * (uw * uw) * ka
    Ts = Tw + y * ka + kb * y * (1 - y)
    rho = ps / (R * Ts)
    mx = rho * vx
    nf = n_dims + 2
    sol = np.zeros(pos.shape[:-1] + (nf,), dtype=LD)
    sol[..., 0] = rho
    sol[..., 1] = mx
    sol[..., nf - 1] = ps / (g - 1) + LD(0.5) * rho * (vx * vx)
    grad = np.zeros(pos.shape[:-1] + (nf, n_dims), dtype=LD)
    rho_dy = -(ps / R) * (ka - kb * y + kb * (1 - y)) / (Ts * Ts)
    grad[..., 0, 1] = rho_dy
    grad[..., 1, 1] = rho_dy * vx + rho * uw
    grad[..., nf - 1, 1] = LD(0.5) * rho_dy * (vx * vx) + mx * uw
    return sol, grad


def yardstick(opp, weight, detjac, pos, u, grad_u, test_case, norm_type, time, gamma, viscous=0, couette=None, prandtl=0.0):
    """eles::compute_error for one block, in np.longdouble.
    opp (n_cubpts, n_upts), weight (n_cubpts), detjac (n_cubpts, n_eles), pos (n_cubpts, n_eles, n_dims), u (n_upts, n_eles,
    n_fields), grad_u (n_upts, n_eles, n_fields, n_dims) or None; couette: dict(u_wall, T_wall, p_bound, R_ref, T_ref).
    -> error (2, n_fields): the sums BEFORE the square root; scale (2, n_fields): ||exact|| + ||interpolated|| in the norm
    asked for (after the square root for norm 2), the scale of the bar."""
    opp, weight, detjac = [np.asarray(a, dtype=LD) for a in (opp, weight, detjac)]
    u = np.asarray(u, dtype=LD)
    n_dims, nf = pos.shape[2], u.shape[2]
    wd = weight[:, None] * detjac                       # (n_cubpts, n_eles)
    sol = np.einsum("jk,kim->jim", opp, u)              # (n_cubpts, n_eles, n_fields)
    with_grad = test_case == 5 and viscous
    if test_case == 1:
        ex = exact_vortex(pos, time, gamma, n_dims)
        exg = None
    elif test_case == 5:
        ex, exg = exact_couette(pos, gamma, prandtl, n_dims=n_dims, **couette)
    else:
        raise ValueError(test_case)
    fn = (lambda a: np.abs(a)) if norm_type == 1 else (lambda a: a * a)
    fin = (lambda s: s) if norm_type == 1 else np.sqrt
    error = np.zeros((2, nf), dtype=LD)
    scale = np.zeros((2, nf), dtype=LD)
    error[0] = np.einsum("jim,ji->m", fn(sol - ex), wd)
    scale[0] = fin(np.einsum("jim,ji->m", fn(ex), wd)) + fin(np.einsum("jim,ji->m", fn(sol), wd))
    if with_grad:
        g = np.einsum("jk,kimn->jimn", opp, np.asarray(grad_u, dtype=LD))
        error[1] = np.einsum("jimn,ji->m", fn(g - exg), wd)
        scale[1] = fin(np.einsum("jimn,ji->m", fn(exg), wd)) + fin(np.einsum("jimn,ji->m", fn(g), wd))
    return error, scale


def assert_at_the_bar(got, want, scale, norm_type, what=""):
    """got, want (2, n_fields): the sums before the square root; printed before they are asserted"""
    fin = (lambda s: s) if norm_type == 1 else np.sqrt
    g, w = fin(np.asarray(got, dtype=LD)), fin(np.asarray(want, dtype=LD))
    miss = np.abs(g - w)
    bar = LD(BAR) * scale
    print("%s norm %d: |got - want| / scale = %s" % (what, norm_type, np.array2string(
        np.asarray(miss / np.where(scale > 0, scale, 1), dtype=np.float64), precision=2)))
    assert np.all(miss <= bar), (what, norm_type, np.asarray(miss, dtype=np.float64), np.asarray(bar, dtype=np.float64))


def gauss_tensor_rule(n, n_dims):
    """the tensor Gauss rule with n points per direction, first direction fastest: loc (n_dims, n^n_dims), weight (n^n_dims)"""
    x, w = np.polynomial.legendre.leggauss(n)
    if n_dims == 2:
        loc = np.array([[x[i], x[j]] for j in range(n) for i in range(n)]).T
        wt = np.array([w[i] * w[j] for j in range(n) for i in range(n)])
    else:
        loc = np.array([[x[i], x[j], x[k]] for k in range(n) for j in range(n) for i in range(n)]).T
        wt = np.array([w[i] * w[j] * w[k] for k in range(n) for j in range(n) for i in range(n)])
    return loc, wt
