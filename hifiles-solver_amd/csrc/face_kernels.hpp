// face_kernels.hpp -- the pairwise kernels of the fused stages: a thread per interior flux-point pair, the point physics of
// face_physics.hpp.  The split stage's are instantiated in fused_hex.hip, the general stage's in general.hip (each kernel in one
// translation unit).
//
//   face_delta_kernel        LDG common solution -> delta_disu_fpts of both sides (a viscous block whose flux kernel does not gather
//                            the partner's values itself)
//   face_flux_kernel         split variant 2: Riemann + LDG viscous flux from the gradients -> norm_tconf_fpts of both sides
//   face_flux2_kernel        split variant 3: Riemann + LDG combination of the projected fluxes Fn, one launch per face block
//   gface_flux_multi_kernel  general stage: the same point, all face blocks of a stage in one launch
#pragma once
#include <type_traits>
#include "hfx_internal.hpp"
#include "face_physics.hpp"

namespace hfx
{

// one side of an interior-face block: the arrays of its element block at the flux points (unused ones: NULL)
struct FaceSide
{
  long plane; // n_fpts * n_eles
  const double *disu, *grad, *tdA;
  const double *fn; // the side's viscous flux projected on its own normal (split variant 3, general stage)
  // LES: the SGS flux at the flux points (NULL: off) -- physical (per-method path: extrapolate_sgsFlux has taken it back), or, with
  // jac / detjac, still in REFERENCE space (n_fpts,n_eles,n_fields,n_dims): the kernel takes it to physical space with |J|^-1 J
  // (second half of eles::extrapolate_sgsFlux, src/eles.cpp:2862-2893)
  const double *sgsf, *jac, *detjac;
  double *delta, *tconf;
};

// the pairs of one interior-face block (int_inters): every pairwise kernel's argument; a block of one element block with
// itself has l == r
struct FacePairArgs
{
  long npairs; // n_fpts_per_inter * n_inters
  const int *L, *R;
  const unsigned char *meta; // of the LEFT block, bit1 of the left point: beta sign flipped (fused stages; the per-method kernels apply ldg_switch)
  const double *norm;        // left block norm_fpts (fpt,ele,dim)
  FaceSide l, r;
};

// f(RS) with the Riemann solver of a pairwise common-flux kernel as a constant
template <class F>
static void with_riemann_solver(int riemann, F f)
{
  if (riemann == 0)
    f(std::integral_constant<int, 0>{});
  else if (riemann == 2)
    f(std::integral_constant<int, 2>{});
  else
    f(std::integral_constant<int, 3>{});
}

template <int ND>
__global__ __launch_bounds__(256) void face_delta_kernel(const FacePairArgs a, const Phys P)
{
  constexpr int NF = ND + 2;
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= a.npairs) return;
  const long il = a.L[q], ir = a.R[q];
  const double beta = ldg_beta(a.meta[il], P);
  // every load before the first store (the compiler must assume that delta and disu overlap: a load behind a store waits)
  double ul[NF], ur[NF];
  gather_pair(a.l.disu, il, a.l.plane, a.r.disu, ir, a.r.plane, ul, ur);
#pragma unroll
  for (int k = 0; k < NF; k++) ldg_common_solution(beta, ul[k], ur[k], a.l.delta[il + k * a.l.plane], a.r.delta[ir + k * a.r.plane]);
}

template <int ND, int RS>
__global__ __launch_bounds__(256) void face_flux_kernel(const FacePairArgs a, const Phys P)
{
  constexpr int NF = ND + 2, NG = NF * ND;
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= a.npairs) return;
  const long il = a.L[q], ir = a.R[q];
  double ul[NF], ur[NF], n[ND], fn[NF];
  gather_pair(a.l.disu, il, a.l.plane, a.r.disu, ir, a.r.plane, ul, ur);
  gather_plane(a.norm, il, a.l.plane, n);
  const double tl = a.l.tdA[il], tr = a.r.tdA[ir];
  riemann_flux_t<ND, RS, true>(P, ul, ur, n, fn);
  if (P.viscous)
  {
    double wl, wr, pl[NF];
    ldg_weights(ldg_beta(a.meta[il], P), wl, wr);
    // (one side's gradient and flux in registers at a time)
    {
      double gq[NG], fq[NG];
      gather_plane(a.l.grad, il, a.l.plane, gq);
      calc_visf<ND, true>(P, ul, gq, fq);
      if (a.l.sgsf) add_sgs_flux<ND>(a.l.sgsf, a.l.jac, a.l.detjac, il, a.l.plane, fq); // src/int_inters.cpp:302-318
#pragma unroll
      for (int k = 0; k < NF; k++) pl[k] = ldg_weighted_projection<ND>(wl, fq, n, k);
    }
    {
      double gq[NG], fq[NG];
      gather_plane(a.r.grad, ir, a.r.plane, gq);
      calc_visf<ND, true>(P, ur, gq, fq);
      if (a.r.sgsf) add_sgs_flux<ND>(a.r.sgsf, a.r.jac, a.r.detjac, ir, a.r.plane, fq);
#pragma unroll
      for (int k = 0; k < NF; k++)
      {
        const double fv = ldg_flux_projections(P, ul[k], ur[k], pl[k], ldg_weighted_projection<ND>(wr, fq, n, k));
        store_flux_both(a.l.tconf[il + k * a.l.plane], tl, a.r.tconf[ir + k * a.r.plane], tr, fn[k], fv);
      }
    }
  }
  else
  {
#pragma unroll
    for (int k = 0; k < NF; k++) store_flux_both(a.l.tconf[il + k * a.l.plane], tl, a.r.tconf[ir + k * a.r.plane], tr, fn[k]);
  }
}

// face_flux2_kernel alone takes the block's arrays ONCE: the pairs of a split stage connect one element block with itself, and with
// the two-sided struct the kernel held both copies of every pointer and plane in scalar registers (38 against 32)
struct FaceBlockArgs
{
  long npairs;
  const int *L, *R;
  const unsigned char *meta;
  const double *norm;
  FaceSide s;
  FaceBlockArgs(const FacePairArgs &a) : npairs(a.npairs), L(a.L), R(a.R), meta(a.meta), norm(a.norm), s(a.l) {}
  __device__ FacePairArgs pair() const { return FacePairArgs{npairs, L, R, meta, norm, s, s}; }
};

// Riemann + LDG common flux of the pairs from u and Fn of both sides -> norm_tconf of both sides: one branch on P.viscous, a store
// loop in either arm.  gface_flux_multi_kernel below is the same point with the choice inside its one store per side and field
// (two sets of stores behind a branch cost that kernel a wave at RoeM); both are written out, every formula a call into
// face_physics.hpp -- behind a shared point function either shape was allocated up to six more registers.
// (Args = FacePairArgs: the two-sided form, for a block whose sides are DIFFERENT element blocks -- the 2-D stage's cross blocks)
__device__ __forceinline__ FacePairArgs face_pair_args(const FaceBlockArgs &b) { return b.pair(); }
__device__ __forceinline__ const FacePairArgs &face_pair_args(const FacePairArgs &a) { return a; }

template <int ND, int RS, class Args = FaceBlockArgs>
__global__ __launch_bounds__(256) void face_flux2_kernel(const Args b, const Phys P)
{
  constexpr int NF = ND + 2;
  const FacePairArgs a = face_pair_args(b);
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= a.npairs) return;
  const long il = a.L[q], ir = a.R[q];
  double ul[NF], ur[NF], n[ND], fn[NF];
  gather_pair(a.l.disu, il, a.l.plane, a.r.disu, ir, a.r.plane, ul, ur);
  gather_plane(a.norm, il, a.l.plane, n);
  const double tl = a.l.tdA[il], tr = a.r.tdA[ir];
  // (every load before the first store: tconf may overlap the inputs as far as the compiler knows)
  double fl[NF], fr[NF];
  const unsigned char mt = a.meta[il]; // with the other loads, not behind the Riemann solver
  const double beta = ldg_beta(mt, P);
  // (one-sided LDG: only the side whose weight is not zero -- the affine flux kernel did not write the other; quads: both, as the
  // 2-D flux kernels write both -- the one register more of the selected load costs this kernel's 2-D form a resident wave)
  if (P.viscous)
  {
    if constexpr (ND == 3)
      gather_pair_needed(P, beta, a.l.fn, il, a.l.plane, a.r.fn, ir, a.r.plane, fl, fr);
    else
      gather_pair(a.l.fn, il, a.l.plane, a.r.fn, ir, a.r.plane, fl, fr);
  }
  riemann_flux_t<ND, RS, true>(P, ul, ur, n, fn);
  if (P.viscous)
  {
#pragma unroll
    for (int k = 0; k < NF; k++)
    {
      const double fv = ldg_flux_projected(P, beta, ul[k], ur[k], fl[k], fr[k]);
      store_flux_both(a.l.tconf[il + k * a.l.plane], tl, a.r.tconf[ir + k * a.r.plane], tr, fn[k], fv);
    }
  }
  else
  {
#pragma unroll
    for (int k = 0; k < NF; k++) store_flux_both(a.l.tconf[il + k * a.l.plane], tl, a.r.tconf[ir + k * a.r.plane], tr, fn[k]);
  }
}

// ALL interior-face blocks of a stage in ONE launch.  A mixed mesh has one block per (left class, right
// class, face type) -- the channel four --, each a few tens of microseconds of work: launched one after the other every one
// pays its own ramp-up and tail (4 x 45 us for 208 MB, i.e. 1.2 TB/s).  Workgroups are dealt to the blocks in whole numbers
// (wg_start), so the block of a workgroup is uniform and its arguments come through scalar loads.
constexpr int GFACE_MAX_BLOCKS = 8;
struct GFaceMulti
{
  int nb;
  unsigned wg_start[GFACE_MAX_BLOCKS + 1];
  struct Block
  {
    FacePairArgs a;
    Phys P; // with the block's arguments: one stride for everything a workgroup reads
  } blk[GFACE_MAX_BLOCKS];
};

template <int RS>
__global__ __launch_bounds__(256) void gface_flux_multi_kernel(const GFaceMulti m)
{
  int b = 0;
  while (b + 1 < m.nb && blockIdx.x >= m.wg_start[b + 1]) b++;
  const FacePairArgs &a = m.blk[b].a;
  const long q = (long)(blockIdx.x - m.wg_start[b]) * 256 + threadIdx.x;
  if (q >= a.npairs) return;
  constexpr int ND = 3, NF = ND + 2;
  const Phys &P = m.blk[b].P;
  const long il = a.L[q], ir = a.R[q];
  double ul[NF], ur[NF], n[ND], fn[NF];
  gather_pair(a.l.disu, il, a.l.plane, a.r.disu, ir, a.r.plane, ul, ur);
  gather_plane(a.norm, il, a.l.plane, n);
  const double tl = a.l.tdA[il], tr = a.r.tdA[ir];
  double fl[NF], fr[NF];
  const unsigned char mt = a.meta[il];
  const bool viscous = P.viscous;
  const double beta = ldg_beta(mt, P);
  if (viscous) gather_pair_needed(P, beta, a.l.fn, il, a.l.plane, a.r.fn, ir, a.r.plane, fl, fr);
  riemann_flux_t<ND, RS, true>(P, ul, ur, n, fn);
#pragma unroll
  for (int k = 0; k < NF; k++)
  {
    double fv = 0.0;
    if (viscous) fv = ldg_flux_projected(P, beta, ul[k], ur[k], fl[k], fr[k]);
    store_flux_both(a.l.tconf[il + k * a.l.plane], tl, a.r.tconf[ir + k * a.r.plane], tr, fn[k], fv, viscous);
  }
}

} // namespace hfx
