// integral_point.hpp -- the pointwise formulas of eles::CalcIntegralQuantities (src/eles.cpp:5540-5620) at one cubature point, in the
// reference's arithmetic and order.  Both kernels that integrate them call these two functions: integral_quantities_kernel
// (kernels_point.hpp; state and gradient read from scratch arrays) and integral_history_kernel (integrals.hip; both in registers).
#pragma once
#include <hip/hip_runtime.h>

namespace hfx
{

constexpr int IQ_MAX = 8; // quantities per call / per monitor

// column j of the velocity gradient, dv[i][j] = d u_i / d x_j, from the state u (NF fields), irho = 1 / u[0] and g, the derivative of
// the conserved fields with respect to x_j (density and momenta are read; the energy's is not)
template <int ND>
__device__ inline void iq_velocity_gradient(const double *u, double irho, const double *g, int j, double (&dv)[ND][ND])
{
#pragma unroll
  for (int i = 0; i < ND; i++) dv[i][j] = irho * (g[i + 1] - u[i + 1] * irho * g[0]);
}

// 0.5 |rho v|^2: irho * tke is the kinetic energy per volume
template <int ND>
__device__ inline double iq_tke(const double *u)
{
  double tke = 0.0;
#pragma unroll
  for (int n = 1; n < ND + 1; n++) tke += 0.5 * u[n] * u[n];
  return tke;
}

// diagnostic `id` (0 kineticenergy, 1 enstropy, 2 pressuredilatation, 3 straincolonproduct, 4 devstraincolonproduct), the reference's
// two-dimensional forms included: diag = (S00 + S11) / 3.0 in 2-D as well (src/eles.cpp:5594)
template <int ND>
__device__ inline double iq_diagnostic(int id, const double *u, double irho, double tke, const double (&dv)[ND][ND], double gamma)
{
  double diagnostic = 0.0;
  if (id == 0)
    diagnostic = irho * tke;
  else if (id == 1)
  {
    const double wz = dv[1][0] - dv[0][1];
    diagnostic = wz * wz;
    if (ND == 3)
    {
      const double wx = dv[ND - 1][1] - dv[1][ND - 1], wy = dv[0][ND - 1] - dv[ND - 1][0];
      diagnostic += wx * wx + wy * wy;
    }
    diagnostic *= 0.5 / irho;
  }
  else if (id == 2)
  {
    const double pressure = (gamma - 1.0) * (u[ND + 1] - irho * tke);
    double dil = dv[0][0] + dv[1][1];
    if (ND == 3) dil = dil + dv[ND - 1][ND - 1];
    diagnostic = pressure * dil;
  }
  else
  {
    double S[ND][ND];
#pragma unroll
    for (int a = 0; a < ND; a++)
#pragma unroll
      for (int b = 0; b < ND; b++) S[a][b] = (a == b) ? dv[a][a] : (dv[a][b] + dv[b][a]) / 2.0;
    double diag = (S[0][0] + S[1][1]) / 3.0;
    if (ND == 3) diag += S[ND - 1][ND - 1] / 3.0;
    if (id == 4)
#pragma unroll
      for (int a = 0; a < ND; a++) S[a][a] -= diag;
#pragma unroll
    for (int a = 0; a < ND; a++)
#pragma unroll
      for (int b = 0; b < ND; b++) diagnostic += S[a][b] * S[a][b];
  }
  return diagnostic;
}

} // namespace hfx
