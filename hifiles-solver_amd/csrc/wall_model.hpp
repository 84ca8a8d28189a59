// wall_model.hpp -- the wall stress of a wall-modelled no-slip face (reference calc_wall_stress,
// /root/reference/src/wall_model_funcs.cpp:13-119).
//
// Plain C++: the same text is the device function of the boundary kernel (kernels_bdy.hpp; its exact and its FAST
// instantiation alike) and, compiled by a host compiler without any HIP header, a host function a stand-alone program can
// call.  The arithmetic is the reference's, operation by operation, including what its quotients give when the relative
// wall-parallel speed is zero (0/0, a NaN flux).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define HFX_WM_FN __host__ __device__ inline
#else
#define HFX_WM_FN inline
#endif

namespace hfx
{

// the scalars of run_input that calc_wall_stress reads
struct WallModelPhys
{
  double gamma, prandtl, rt_inf, mu_inf, c_sth, fix_vis;
};

// The Newton loop of model 2 runs `do ... while (|dutau| > 1e-6)` in the reference, which never ends where the iteration
// cycles; a kernel that spins is a hang of the whole device.  Here it carries a cap: on reaching it utau becomes NaN (the
// flux of that point is NaN, which the NaN check of the step loop reports).  Below the cap nothing differs.
constexpr int WALL_MODEL_NEWTON_CAP = 64;

// model 1: Werner-Wengle, 2: Breuer-Rodi / compressible wall function.  u_wm: state at the face's input point, u_w: the wall
// state (sol_spec 2), dist: distance of the input point from the wall, n: unit normal.  fn: the normal flux (0, tau_w,
// -q_w + v_w . tau_w).  n_newton (optional): the Newton iterations model 2 took.
template <int ND>
HFX_WM_FN void wall_stress(const int model, const WallModelPhys &P, const double prandtl_t, const double Kappa,
                           const double (&u_wm)[ND + 2], const double (&u_w)[ND + 2], const double dist, const double (&n)[ND],
                           double (&fn)[ND + 2], int *n_newton = nullptr)
{
  using std::sqrt; using std::pow; using std::log; using std::asin; using std::fabs;
  const double rho_wm = u_wm[0], rho_w = u_w[0];
  double v_wm_n = 0;
  for (int i = 0; i < ND; i++) v_wm_n += u_wm[i + 1] / rho_wm * n[i];

  double vw[ND], v_wm_rel[ND], tw[ND];
  double v_wm_rel_mag = 0;
  for (int i = 0; i < ND; i++)
  {
    const double v_par = u_wm[i + 1] / rho_wm - n[i] * v_wm_n; // wall-parallel input velocity
    vw[i] = u_w[i + 1] / rho_w;
    v_wm_rel[i] = v_par - vw[i];
    v_wm_rel_mag += v_wm_rel[i] * v_wm_rel[i];
  }
  v_wm_rel_mag = sqrt(v_wm_rel_mag);

  double ke_wm = 0., ke_w = 0.;
  for (int i = 0; i < ND; i++)
  {
    const double v = u_wm[i + 1] / rho_wm;
    ke_wm += 0.5 * (v * v); // 0.5 * pow(v, 2)
    ke_w += 0.5 * (vw[i] * vw[i]);
  }
  const double inte_wm = u_wm[ND + 1] / rho_wm - ke_wm;
  const double inte_w = u_w[ND + 1] / rho_w - ke_w;

  auto sutherland = [&](double inte) {
    const double rt_ratio = (P.gamma - 1.0) * inte / P.rt_inf;
    double mu = P.mu_inf * pow(rt_ratio, 1.5) * (1 + P.c_sth) / (rt_ratio + P.c_sth);
    mu = mu + P.fix_vis * (P.mu_inf - mu);
    return mu;
  };

  double tw_mag, qw;
  if (model == 1)
  {
    const double mu_wm = sutherland(inte_wm);
    const double Rey_c = 11.81 * 11.81;
    const double Rey = rho_wm * v_wm_rel_mag * dist / mu_wm;
    double uplus;
    if (Rey < Rey_c)
      uplus = sqrt(Rey);
    else
      uplus = pow(8.3, 0.875) * pow(Rey, 0.125);
    const double utau = v_wm_rel_mag / uplus;
    tw_mag = rho_wm * utau * utau;
    if (Rey < Rey_c)
      qw = (inte_w - inte_wm) * P.gamma * tw_mag / (P.prandtl * v_wm_rel_mag);
    else
      qw = (inte_w - inte_wm) * P.gamma * tw_mag / (prandtl_t * (v_wm_rel_mag + utau * 11.81 * (P.prandtl / prandtl_t - 1.0)));
  }
  else
  {
    const double B = sqrt(2 * P.gamma * inte_w / prandtl_t), C = 5.2;
    const double ueq = B * asin(v_wm_rel_mag / B);
    const double mu_w = sutherland(inte_w);
    double utau = 1., dutau;
    int it = 0;
    do
    {
      dutau = -(utau * (log(rho_w * dist * utau / mu_w) / Kappa + C) - ueq) / (1 / Kappa * (log(rho_w * dist * utau / mu_w) + 1.) + C);
      utau += dutau;
      it++;
    } while (fabs(dutau) > 1.e-6 && it < WALL_MODEL_NEWTON_CAP);
    if (fabs(dutau) > 1.e-6) utau = NAN; // the cap was reached (a NaN iterate leaves the loop by itself, as in the reference)
    if (n_newton) *n_newton = it;
    tw_mag = rho_w * utau * utau;
    qw = 0.;
  }
  for (int i = 0; i < ND; i++) tw[i] = tw_mag * v_wm_rel[i] / v_wm_rel_mag;

  double vw_tw = 0.;
  for (int i = 0; i < ND; i++) vw_tw += vw[i] * tw[i];
  fn[0] = 0;
  for (int i = 0; i < ND; i++) fn[i + 1] = tw[i];
  fn[ND + 1] = -qw + vw_tw;
}

} // namespace hfx
