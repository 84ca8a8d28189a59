// plot_point.hpp -- the pointwise formulas of eles::calc_diagnostic_fields_ppts (src/eles.cpp:3858-4006) at one plot point, in the
// reference's arithmetic and order.  plot_fields_kernel (plot_fields.hip) calls them with the interpolated state and the velocity
// gradient in registers.  Plain C++ behind one macro, so that a host compiler takes the header as it is.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HFX_PP_FN __host__ __device__ inline
#else
#define HFX_PP_FN inline
#endif

namespace hfx
{

constexpr int PF_MAX_DIAG = 16; // diagnostic fields per monitor (the reference knows ten names; a name may be listed twice)

// run_input.diagnostic_fields by code (hfx_plot_field of include/hfx.h, in the order of src/eles.cpp:3885-3983)
enum PlotField : int
{
  PF_U = 0, PF_V, PF_W, PF_ENERGY, PF_MACH, PF_PRESSURE, PF_VORTICITY, PF_Q_CRITERION, PF_SCALED_Q_CRITERION, PF_SENSOR, PF_N_FIELDS
};

HFX_PP_FN bool pf_reads_gradient(int code) { return code == PF_VORTICITY || code == PF_Q_CRITERION || code == PF_SCALED_Q_CRITERION; }

// column j of the velocity gradient, dv[i][j] = d u_i / d x_j = irho (d(rho u_i) - u_i d(rho)), with u_i from the interpolated state u
// and g the interpolated derivative of the CONSERVED fields with respect to x_j (src/eles.cpp:3917-3945)
template <int ND>
HFX_PP_FN void pf_velocity_gradient(const double *u, const double *g, int j, double (&dv)[ND][ND])
{
  const double irho = 1. / u[0];
  for (int i = 0; i < ND; i++)
  {
    const double vel = u[i + 1] * irho;
    dv[i][j] = irho * (g[i + 1] - vel * g[0]);
  }
}

// diagnostic field `code` at a point with the state u (ND + 2 conserved fields), the velocity gradient dv (read by vorticity and the
// two Q criteria only) and the element's sensor value.  Q in two dimensions is refused before any launch: it gives 0 here
template <int ND>
HFX_PP_FN double pf_diagnostic(int code, const double *u, const double (&dv)[ND][ND], double gamma, double sensor)
{
  double v_sq = 0.;
  for (int m = 0; m < ND; m++) v_sq += u[m + 1] * u[m + 1];
  v_sq /= u[0] * u[0];
  const double pressure = (gamma - 1.0) * (u[ND + 1] - 0.5 * u[0] * v_sq);
  const double irho = 1. / u[0];
  switch (code)
  {
  case PF_U: return u[1] * irho;
  case PF_V: return u[2] * irho;
  case PF_W: return ND == 2 ? 0. : u[ND] * irho;
  case PF_ENERGY: return u[ND + 1];
  case PF_MACH: return sqrt(v_sq / (gamma * pressure / u[0]));
  case PF_PRESSURE: return pressure;
  case PF_SENSOR: return sensor;
  default: break;
  }
  const double dudy = dv[0][1], dvdx = dv[1][0];
  if (ND == 2) return code == PF_VORTICITY ? fabs(dvdx - dudy) : 0.;
  const double dudx = dv[0][0], dudz = dv[0][ND - 1], dvdy = dv[1][1], dvdz = dv[1][ND - 1];
  const double dwdx = dv[ND - 1][0], dwdy = dv[ND - 1][1], dwdz = dv[ND - 1][ND - 1];
  double wx = dwdy - dvdz, wy = dudz - dwdx, wz = dvdx - dudy;
  if (code == PF_VORTICITY) return sqrt(wx * wx + wy * wy + wz * wz);
  wx *= 0.5;
  wy *= 0.5;
  wz *= 0.5;
  const double Sxx = dudx, Syy = dvdy, Szz = dwdz;
  const double Sxy = 0.5 * (dudy + dvdx), Sxz = 0.5 * (dudz + dwdx), Syz = 0.5 * (dvdz + dwdy);
  const double SS = Sxx * Sxx + Syy * Syy + Szz * Szz + 2 * Sxy * Sxy + 2 * Sxz * Sxz + 2 * Syz * Syz;
  const double OO = 2 * wx * wx + 2 * wy * wy + 2 * wz * wz;
  if (code == PF_Q_CRITERION) return 0.5 * (OO - SS);
  const double eps = 1.e-24;
  return 0.5 * (OO - SS) / (SS + eps); // normalized
}

} // namespace hfx
