// face_physics.hpp -- the physics of ONE flux point of a face, once: the reference's inters::calculate_common_*, ldg_solution and
// ldg_flux (src/inters.cpp:561-650) and the gathers and stores around them.  Every common-flux kernel -- per-method
// (kernels_point.hpp), partition faces (kernels_mpi.hpp), boundary faces (kernels_bdy.hpp), the fused stages' pairwise kernels
// (face_kernels.hpp) -- computes its indices, gathers, and calls in here.  No kernels and no argument structs: the kernels decide
// the order of loads and stores, these functions only compute.  Two copies of the common-solution line stay outside on purpose:
// phase A0 of split_flux_tensor_kernel and the staging loop of general_flux_kernel, element kernels with hand-placed loads.
#pragma once
#include "physics.hpp"

namespace hfx
{

// ---- gathers: v(s) of the point i of a plane-strided array (point, element | field [, dim]) ...
// ((p + i)[s * plane], the point's address first: with p[i + s * plane] the kernels held up to eight more registers)
template <int S>
__device__ __forceinline__ void gather_plane(const double *p, long i, long plane, double (&v)[S])
{
#pragma unroll
  for (int s = 0; s < S; s++) v[s] = (p + i)[s * plane];
}

// ... and of an exchanged record (fpt, field [, dim], inter): slot j of face i, nfpi flux points per face (src/mpi_inters.cpp:225-229)
template <int S>
__device__ __forceinline__ void gather_record(const double *buf, int j, int nfpi, long i, double (&v)[S])
{
#pragma unroll
  for (int s = 0; s < S; s++) v[s] = buf[j + (long)nfpi * (s + S * i)];
}

// both sides of a pair together, left and right alternating (the order in which the loads are requested) ...
template <int S>
__device__ __forceinline__ void gather_pair(const double *pl, long il, long plane_l, const double *pr, long ir, long plane_r, double (&vl)[S],
                                            double (&vr)[S])
{
#pragma unroll
  for (int s = 0; s < S; s++)
  {
    vl[s] = (pl + il)[s * plane_l];
    vr[s] = (pr + ir)[s * plane_r];
  }
}

// ... and those of a partition face, whose right side is the exchanged record
template <int S>
__device__ __forceinline__ void gather_pair_record(const double *pl, long il, long plane, const double *buf, int j, int nfpi, long i,
                                                   double (&vl)[S], double (&vr)[S])
{
#pragma unroll
  for (int s = 0; s < S; s++)
  {
    vl[s] = pl[il + s * plane];
    vr[s] = buf[j + (long)nfpi * (s + S * i)];
  }
}

// ---- LDG.  What follows computes ONE field of the point: the kernels loop over the fields and place their stores.
// beta of a pair from the sign decision stored with its LEFT point (bit 1 of the meta byte / partner word: ldg_switch on the left
// normal came out negative when the tables were built)
__device__ __forceinline__ double ldg_beta(int meta, const Phys &P) { return (meta & 2) ? -P.ldg_beta : P.ldg_beta; }

// common solution u_c = (u_L + u_R)/2 - beta (u_L - u_R) (src/inters.cpp:637) as the corrections u_c - u_L and u_c - u_R;
// one-sided faces (partition faces) take the left one only
__device__ __forceinline__ void ldg_common_solution(double beta, double ul, double ur, double &dl, double &dr)
{
  const double uc = 0.5 * (ul + ur) - beta * (ul - ur);
  dl = uc - ul;
  dr = uc - ur;
}

__device__ __forceinline__ double ldg_common_solution(double beta, double ul, double ur)
{
  double dl, dr;
  ldg_common_solution(beta, ul, ur, dl, dr);
  return dl;
}

// the weights of the left and right viscous flux in the common one (src/inters.cpp:641-647)
__device__ __forceinline__ void ldg_weights(double beta, double &wl, double &wr)
{
  wl = 0.5 + beta;
  wr = 0.5 - beta;
}

// the penalty on the jump of the solution, taken off the common viscous flux
__device__ __forceinline__ double ldg_penalty(const Phys &P, double ul, double ur) { return P.ldg_tau * (ur - ul); }

// Common viscous flux (field k) from the two FULL fluxes f(k,m) = f[k + NF*m], in the reference's order: the fluxes are combined
// first and the combination is projected on the left normal.  The per-method kernels (common_viscflux_kernel,
// mpi_common_viscflux_kernel), which are held against the reference's own arrays.
template <int ND>
__device__ __forceinline__ double ldg_flux_reference(const Phys &P, double beta, double ul, double ur, const double (&fl)[(ND + 2) * ND],
                                                     const double (&fr)[(ND + 2) * ND], const double (&n)[ND], int k)
{
  constexpr int NF = ND + 2;
  double wl, wr;
  ldg_weights(beta, wl, wr);
  double fn = 0.0;
#pragma unroll
  for (int l = 0; l < ND; l++)
  {
    const double fc = wl * fl[k + NF * l] + wr * fr[k + NF * l];
    fn += fc * n[l];
  }
  fn -= ldg_penalty(P, ul, ur);
  return fn;
}

// The same in the split stage's association: each side's weighted flux is projected on its own, (w f) . n with w of ldg_weights,
// and ldg_flux_projections sums the two.  face_flux_kernel, which holds one side's gradient and flux in registers at a time; the
// result differs from the reference's order in the last bit, and both stay as they are.
template <int ND>
__device__ __forceinline__ double ldg_weighted_projection(double w, const double (&f)[(ND + 2) * ND], const double (&n)[ND], int k)
{
  constexpr int NF = ND + 2;
  double s = 0.0;
#pragma unroll
  for (int l = 0; l < ND; l++) s += (w * f[k + NF * l]) * n[l];
  return s;
}

__device__ __forceinline__ double ldg_flux_projections(const Phys &P, double ul, double ur, double pl, double pr)
{
  double fv = pl + pr;
  fv -= ldg_penalty(P, ul, ur);
  return fv;
}

// Common viscous flux from the two PROJECTED fluxes, each on its own side's normal: (1/2+b) F_L.n + (1/2-b) F_R.n - tau (u_R - u_L)
// with n the left normal = -(right normal).  face_flux2_kernel, gface_flux_multi_kernel, mpi_common_flux2_kernel.
__device__ __forceinline__ double ldg_flux_projected(const Phys &P, double beta, double ul, double ur, double fnl, double fnr)
{
  double wl, wr;
  ldg_weights(beta, wl, wr);
  double fv = wl * fnl - wr * fnr;
  fv -= ldg_penalty(P, ul, ur);
  return fv;
}

// One-sided LDG: with |ldg_beta| = 1/2 one of the two weights of every pair is exactly 0.0 and the common viscous flux is the Fn of
// ONE side (which one: the pair's sign bit).  The flux kernels that know their points' partners do not write an Fn whose weight is
// zero (split3_kernels.hpp, fn_needed), so the pairwise kernels must not read it: `both` -- uniform, from the run's ldg_beta --
// says whether both sides enter; if not, the one load per field goes to the side with the non-zero weight and the other side is 0.0
// (w * Fn - 0.0 * 0.0: the result of the full formula for finite data).
__device__ __forceinline__ bool ldg_both_sides(const Phys &P) { return (0.5 + P.ldg_beta) != 0.0 && (0.5 - P.ldg_beta) != 0.0; }

template <int S>
__device__ __forceinline__ void gather_pair_needed(const Phys &P, double beta, const double *pl, long il, long plane_l, const double *pr, long ir,
                                                   long plane_r, double (&vl)[S], double (&vr)[S])
{
  if (ldg_both_sides(P))
  {
    gather_pair(pl, il, plane_l, pr, ir, plane_r, vl, vr);
    return;
  }
  double wl, wr;
  ldg_weights(beta, wl, wr);
  const bool left = wl != 0.0;
  const double *p = left ? pl + il : pr + ir;
  const long plane = left ? plane_l : plane_r;
#pragma unroll
  for (int s = 0; s < S; s++)
  {
    const double x = p[s * plane];
    vl[s] = left ? x : 0.0;
    vr[s] = left ? 0.0 : x;
  }
}

// ---- the fused paths' Riemann solver (reciprocal-multiply physics) where the solver is not a template argument of the kernel
template <int ND>
__device__ __forceinline__ void riemann_flux_fast(const Phys &P, const double (&ul)[ND + 2], const double (&ur)[ND + 2], const double (&n)[ND],
                                                  double (&fn)[ND + 2])
{
  if (P.riemann == 0)
    riemann_flux_t<ND, 0, true>(P, ul, ur, n, fn);
  else if (P.riemann == 2)
    riemann_flux_t<ND, 2, true>(P, ul, ur, n, fn);
  else
    riemann_flux_t<ND, 3, true>(P, ul, ur, n, fn);
}

// ---- stores of one field of the common flux: norm_tconf_l = f tdA_l, norm_tconf_r = -f tdA_r (src/int_inters.cpp:217-220,329-332).
// ACC: added to what is there (the per-method viscous sweep); (fn, fv): the inviscid and the viscous common flux in one store
template <bool ACC = false>
__device__ __forceinline__ void store_flux_left(double &tcl, double tl, double f)
{
  if (ACC)
    tcl += f * tl;
  else
    tcl = f * tl;
}

__device__ __forceinline__ void store_flux_left(double &tcl, double tl, double fn, double fv) { tcl = fn * tl + fv * tl; }

template <bool ACC = false>
__device__ __forceinline__ void store_flux_both(double &tcl, double tl, double &tcr, double tr, double f)
{
  store_flux_left<ACC>(tcl, tl, f);
  if (ACC)
    tcr += -f * tr;
  else
    tcr = -f * tr;
}

// (`viscous` false: fn alone -- a uniform choice inside the one store per side, where a kernel serves both kinds of run)
__device__ __forceinline__ void store_flux_both(double &tcl, double tl, double &tcr, double tr, double fn, double fv, bool viscous = true)
{
  tcl = viscous ? fn * tl + fv * tl : fn * tl;
  tcr = viscous ? -fn * tr + -fv * tr : -fn * tr;
}

} // namespace hfx
