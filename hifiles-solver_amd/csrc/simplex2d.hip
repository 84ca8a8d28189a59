// simplex2d.hip -- the fused RK stage for TWO-DIMENSIONAL SIMPLEX blocks: triangles (eles_tris of the reference).
//
// Reference side: the same 17 calls of CalcResidual + AdvanceSolution as everywhere (src/solver.cpp:50-223); on triangles the seven
// operators (built by src/eles_tris.cpp) are dense and SMALL -- P1..P5: 3, 6, 10, 15, 21 solution and 6, 9, 12, 15, 18 flux points.
// The stage is cut where the general stage (general.hip) is cut and is at most four launches per stage:
//
//   face_delta_kernel<2>       thread per interior flux-point pair: LDG common solution -> delta_disu_fpts (only where the element
//                              kernel does not gather the partner values itself)
//   simplex2d_element_kernel   corrected gradient at the solution points (opp_4, opp_5), its extrapolation (opp_6), both point physics
//                              blocks, the discontinuous divergence (opp_2) and normal flux (opp_1); leaves div_tdisf, norm_tdisf and
//                              each side's viscous flux projected on its own normal (Fn, 4 doubles per flux point); where the block
//                              registered over-integration, the de-aliased inviscid flux too (OVERINT, below); where it registered
//                              an LES closure, the SGS flux too, and Fn carries F_sgs . n (LES, below)
//   face_flux2_kernel<2>       thread per pair: Riemann + LDG common flux from u and Fn of both sides -> norm_tconf; the boundary kernels
//   simplex2d_update_kernel    opp_3 (norm_tconf - norm_tdisf), RK update, opp_0 of the new state
//
// Form: VECTOR, not matrix cores.  The general stage's batches of 16 elements on v_mfma_f64_16x16x4_f64 pad every operator to 16
// rows: at P1 (3 and 6 rows) and P2 (6 and 9) most of a tile would be padding.  Here one lane owns one (element, operator row):
// item q of a group is element q / n, row q % n -- the order of the arrays in memory, so every global load and store of a phase
// is one contiguous run per field.  A group's state lies in LDS as [row][element][field] (all fields of a point in one 32- or
// 64-byte read, the same address for the lanes of one element: a broadcast), the operators as the dense column-major matrices the
// block registered (consecutive rows in consecutive lanes: conflict free).  A workgroup stages the operators once and walks groups
// grid-stride.  Ordinary stores, no atomics but the NaN flag's: bit-reproducible from run to run.
//
// Option blocks_2d: the same stage over SEVERAL two-dimensional blocks (a mixed quadrilateral / triangle mesh, several triangle
// blocks) and over a block of quadrilaterals -- the dense kernels' plain forms on a second size table (QUAD2D_SIZES, P1..P4).  Each
// block has its own tables and its own element and update launch; an interior-face block between two element blocks (a cross block)
// takes each side's arrays from its own block (face_flux2_kernel's two-sided form), and its LDG corrections are face_delta_kernel's:
// a partner word addresses the block's own flux points only (simplex2d_prepare_blocks, simplex2d_build).
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "simplex2d.hpp"
#include "face_kernels.hpp" // the pairwise kernels (face_delta_kernel<2>, face_flux2_kernel<2, RS> are instantiated here too)

namespace hfx
{

struct Simplex2dData
{
  DevBuf<double> element_ops, update_ops; // the operators one behind the other, in the kernels' order (zeros where inviscid)
  // shock capturing registered in the triangle's own form (shock_form_refusal): update_ops + inv_vandermonde + exp_filter for the
  // update kernel's SHOCK instantiation, and the registration (hfx_eles::shock_serial) the tables were made from
  DevBuf<double> update_shock_ops;
  bool shock = false;
  unsigned shock_serial = 0;
  // over-integration (hfx_eles_set_over_int): opp_over_int_cubpts and over_int_filter one behind the other for the element kernel's
  // OVERINT instantiation, and the registration (hfx_eles::over_int_serial) they were made from
  DevBuf<double> overint_ops;
  bool over_int = false;
  unsigned over_int_serial = 0;
  int n_cub = 0;
  // an LES closure with an SGS flux (sgs_model 0, 1, 2, 4; les_jacobian_residual): its squared length scale (n_upts, n_eles;
  // les_len2_upload) for the element kernel's LES instantiation, and the registration (hfx_eles::les_serial) it was made from
  DevBuf<double> les_len2;
  bool les = false;
  unsigned les_serial = 0;
  DevBuf<unsigned char> meta;             // (n_fpts, n_eles): bit1 beta sign flipped (LEFT point of a pair), bit2 boundary point
  DevBuf<int> nbr;                        // (n_fpts, n_eles) partner word of every flux point (S2dArgs::nbr)
  DevBuf<double> disu_alt;                // second disu_fpts buffer (the update kernel writes the new state's flux-point solution)
  DevBuf<double> fn_fpts;                 // (n_fpts, n_eles, n_fields) viscous flux projected on the point's own normal
  bool any_bdy = false, any_int = false; // any_int: pairs INSIDE the block (the partner words address them)
  // points on cross blocks (an interior-face block between this block and another one of the call): their partner word is -1 and
  // face_delta_kernel<2> writes their corrections
  long n_cross_pts = 0;
  std::vector<const hfx_eles *> built_blocks; // the element blocks of the call the tables were made for
  // partitioned blocks: the groups (of the size class's G consecutive elements) with and without a partition flux point, ascending
  DevBuf<int> partition_groups, interior_groups;
  int n_partition_groups = 0, n_interior_groups = 0;
  bool any_mpi = false;
  // the ONE partition-face block whose receive record the partner words of partition points address (their remote bit); NULL:
  // partition points carry the word -1 and mpi_delta_kernel<2> writes their corrections
  const hfx_inters *remote_face = nullptr;
  std::vector<const hfx_inters *> built_with; // the face blocks the tables were made from
  bool built = false;
};

void Simplex2dDelete::operator()(Simplex2dData *p) const { delete p; }

void simplex2d_invalidate(hfx_eles *e)
{
  if (e && e->simplex2d) e->simplex2d->built = false;
}

struct S2dArgs
{
  int n_eles, n_groups;
  const double *ops;
  const double *u0, *delta, *disu;
  // the LDG correction of an interior flux point is formed in the element kernel from the partner's flux-point solution:
  // (partner offset << 4) | remote << 2 | beta sign flipped << 1 | this point is the right side; -1: a boundary point (its
  // correction is in `delta`).  NULL: `delta` holds all of them.  remote: a partition point whose partner lies in the receive
  // record `in_disu` of the block's partition faces -- the offset is that of the partner's slot in its face's record (Rlut), the
  // stride from field to field `nfpi` instead of the plane, and the point is the LEFT side with its own switch bit
  const int *nbr;
  const double *in_disu;
  int nfpi;
  // the groups this launch walks: groups[0 .. n_list); NULL: all n_groups, in order
  const int *groups;
  int n_list;
  const double *detjac_upts, *JGinv_upts, *detjac_fpts, *JGinv_fpts, *norm_fpts;
  const unsigned char *meta;
  double *div, *ntd, *fn, *grad_fpts; // grad_fpts: boundary points only (NULL: no boundary faces / inviscid)
  Phys P;
  // update kernel
  double *u0w, *u1;
  const double *tconf, *src, *dt_local;
  double *disu_next;
  unsigned long long *nan_flag;
  int adv_type, in_step, dt_local_on, write_div, need_u1;
  double dt, rk_a, rk_b;
  // update kernel with the shock filter folded in (SHOCK): the sensor's field (0 or n_dims + 1), the threshold and sensor(n_eles)
  int sens_field;
  double s0;
  double *sensor;
  // element kernel with over-integration (S2dOverInt::folded): opp_over_int_cubpts (n_cub x NU) and over_int_filter (NU x n_cub) one
  // behind the other, dense column-major; JGinv_over_int_cubpts (l, n, m, ele).  S2dOverInt::unfolded: tdisf_upts as
  // hfx_eles_evaluate_invFlux_over_int left it (the transformed inviscid flux at the solution points)
  const double *oi_ops, *JG_oi, *tdisf_in;
  int n_cub;
  // element kernel with an LES closure (LES): the closure (Lu / Le of the step's calc_sgs_terms are read through it), its squared
  // length scale les_len2 (n_upts, n_eles) and tdA_fpts, which takes the projected transformed SGS flux back to physical space
  LesParams les;
  const double *les_len2, *tdA_fpts;
};

// how the element kernel takes the inviscid flux at the solution points of a block that registered over-integration
enum class S2dOverInt { none, folded, unfolded };

constexpr int S2D_NF = 4, S2D_ND = 2, S2D_T = 64 * SIMPLEX2D_WAVES;

// g_phys(d) = sum_l (inv_detjac * g_ref(l)) * JGinv(l,d)   (BLAS=NO branch of src/eles.cpp:1975-1979)
__device__ __forceinline__ void s2d_to_physical(const double inv_detjac, const double (&JG)[4], const double (&tg)[2], double (&cg)[2])
{
#pragma unroll
  for (int d = 0; d < 2; d++) cg[d] = 0.0;
#pragma unroll
  for (int l = 0; l < 2; l++)
  {
    const double temp = inv_detjac * tg[l];
#pragma unroll
    for (int d = 0; d < 2; d++) cg[d] += temp * JG[l + 2 * d];
  }
}

__device__ __forceinline__ void s2d_stage_ops(double *dst, const double *src, int n, int tid)
{
  for (int q = tid; q < n; q += S2D_T) dst[q] = src[q];
}

// ---------------------------------------------------------------------------------------------------------------
// element kernel
// ---------------------------------------------------------------------------------------------------------------
//
// OVERINT folded: eles::evaluate_invFlux_over_int (src/eles.cpp:1480-1545) between the staging of U and of D, with D and Gr as
// scratch.  The cubature points are walked in chunks of CH = NU:
//   stage   the chunk's rows of opp_over_int_cubpts (A, [point][k], point fastest) and columns of over_int_filter (Fl, as in memory)
//           -> the D region
//   flux    lane (element, cubature point m): u_m = sum_k A(m, k) U[k], ascending k; calc_invf; the transform with the point's OWN
//           four entries of JGinv_over_int_cubpts -> Gr[m - m0][element][field + NF * l]
//   filter  lane (element, solution point j): its TRIPS points' 8 accumulators += sum_m Fl(j, m) Gr[m - m0], ascending m
// The accumulators stay in registers until P3, which adds the transformed viscous flux to them and never calls calc_invf.
// OVERINT unfolded: P3 reads the transformed inviscid flux from tdisf_upts instead (hfx_eles_evaluate_invFlux_over_int ran before
// the launch).  OVERINT none is the code without any of it.
//
// LES: the eddy-viscosity / similarity closure of an LES run (eles::calc_sgsf_upts, src/eles.cpp:2395-2650; sgs_model 0, 1, 2, 4 on
// a viscous run, OVERINT none).  The reference adds F_sgs to the total flux at the solution points (src/eles.cpp:2360-2392) and, at
// the flux points, extrapolates the TRANSFORMED SGS flux (opp_0), takes it back to physical space with Jacobian_fpts and adds it to
// each side's viscous flux in the common-flux sweep (src/eles.cpp:2817-2893, src/int_inters.cpp:299-313).  What the face kernels
// need of that is F_sgs . n = (F~_sgs . n~) / tdA = (sum_d opp_1[d] F~_sgs,d) / tdA (the identity of general.hip's LESG form, which
// holds where Jacobian_fpts belongs to the block's own metrics: les_jacobian_residual), so Fn carries it and no sgsf array exists:
//   P2   forms Fn as ever but KEEPS a lane's flux points (TRIPS_F x 4 doubles) in registers instead of storing them
//   P3   calc_sgsf_fast on the physical gradient the point physics holds; the transformed inviscid + viscous flux stays in
//        registers (TRIPS x 8 doubles), the transformed SGS flux ALONE goes to the lane's Gr point
//   P3b  lane (element, flux point j) -- the q -> (element, flux point) map of P2, so the lane holds Fn of the point --:
//        s = sum_k opp_1[0](j, k) Gr[k](f) + opp_1[1](j, k) Gr[k](f + NF), ascending k; Fn += s / tdA_fpts: the ONE store of Fn
//   then every lane adds its register flux to its Gr point, and P4 runs on the total flux as ever.
// With LES false the kernel is the code without any of it.
template <int NU, int NFP, int G, S2dOverInt OVERINT, bool LES = false>
__global__ __launch_bounds__(S2D_T) void simplex2d_element_kernel_t(const S2dArgs a)
{
  static_assert(!LES || OVERINT == S2dOverInt::none, "the LES form is not built beside over-integration");
  constexpr int NF = S2D_NF, ND = S2D_ND, T = S2D_T, GP = G + 1, NC = NF * ND;
  constexpr int CH = NU;                      // cubature points per chunk
  constexpr int TRIPS = (NU * G + T - 1) / T; // solution points of a group per lane
  constexpr int TRIPS_F = (NFP * G + T - 1) / T; // flux points of a group per lane
  static_assert(OVERINT != S2dOverInt::folded || 2 * CH * NU <= NFP * GP * NF, "a chunk's operator slices fit the D region");
  extern __shared__ double lds[];
  // operators, dense column-major as registered
  double *o4 = lds;                     // [2][NU x NU]
  double *o5 = o4 + 2 * NU * NU;        // [2][NU x NFP]
  double *o6 = o5 + 2 * NU * NFP;       // NFP x NU
  double *o0 = o6 + NFP * NU;           // NFP x NU
  double *o2 = o0 + NFP * NU;           // [2][NU x NU]
  double *o1 = o2 + 2 * NU * NU;        // [2][NFP x NU]
  double *U = o1 + 2 * NFP * NU;        // [NU][GP][NF]   the state
  double *D = U + NU * GP * NF;         // [NFP][GP][NF]  delta_disu_fpts
  double *Gr = D + NFP * GP * NF;       // [NU][GP][NC]   reference-space gradient, then the transformed total flux; c = field + NF * dim
  static_assert(simplex2d_element_lds_bytes(NU, NFP, G) == sizeof(double) * (simplex2d_element_ops(NU, NFP) + (size_t)GP * (NU * NF + NFP * NF + NU * NC)), "LDS image");
  const int tid = threadIdx.x;
  const bool visc = a.P.viscous != 0;
  const long plane_u = (long)NU * a.n_eles, plane_f = (long)NFP * a.n_eles;
  s2d_stage_ops(lds, a.ops, (int)simplex2d_element_ops(NU, NFP), tid);

  const int n_walk = a.groups ? a.n_list : a.n_groups;
  for (int it = blockIdx.x; it < n_walk; it += gridDim.x)
  {
    const int grp = a.groups ? a.groups[it] : it; // (within a group nothing changes: one contiguous run per field)
    const long e0 = (long)grp * G;
    const int nval = (int)min((long)G, a.n_eles - e0);
    const int items_u = NU * nval, items_f = NFP * nval; // (a last partial group: its elements alone; nothing is read or written past them)

    // ---- P0: the state and the LDG corrections of the group -> [row][element][field]
    for (int q = tid; q < items_u; q += T)
    {
      const int el = q / NU, k = q - el * NU;
      double r[NF];
#pragma unroll
      for (int f = 0; f < NF; f++) r[f] = a.u0[e0 * NU + q + f * plane_u];
#pragma unroll
      for (int f = 0; f < NF; f++) U[(k * GP + el) * NF + f] = r[f];
    }
    [[maybe_unused]] double oi[TRIPS][NC]; // (folded: the de-aliased transformed inviscid flux of the lane's solution points)
    if constexpr (OVERINT == S2dOverInt::folded)
    {
      __syncthreads(); // (U is complete; every lane has left the P4 of the group before, which read Gr)
      double *A = D, *Fl = D + CH * NU;
      const int n_cub = a.n_cub;
      const double *JGo = a.JG_oi + (size_t)4 * n_cub * e0;
#pragma unroll
      for (int t = 0; t < TRIPS; t++)
#pragma unroll
        for (int c = 0; c < NC; c++) oi[t][c] = 0.0;
      for (int m0 = 0; m0 < n_cub; m0 += CH)
      {
        const int ch = min(CH, n_cub - m0);
        for (int q = tid; q < CH * NU; q += T)
        {
          const int k = q / CH, mm = q - k * CH;
          if (mm < ch) A[q] = a.oi_ops[m0 + mm + (size_t)n_cub * k];
        }
        for (int q = tid; q < NU * ch; q += T) Fl[q] = a.oi_ops[(size_t)n_cub * NU + (size_t)NU * m0 + q];
        __syncthreads();
        for (int q = tid; q < CH * nval; q += T)
        {
          const int el = q / CH, mm = q - el * CH;
          if (mm >= ch) continue;
          double JG[4];
#pragma unroll
          for (int c = 0; c < 4; c++) JG[c] = JGo[((size_t)el * n_cub + m0 + mm) * 4 + c];
          double u[NF], F[NC];
#pragma unroll
          for (int f = 0; f < NF; f++) u[f] = 0.0;
#pragma unroll 2
          for (int k = 0; k < NU; k++)
          {
            const double m = A[mm + CH * k];
#pragma unroll
            for (int f = 0; f < NF; f++) u[f] += m * U[(k * GP + el) * NF + f];
          }
          calc_invf<ND, true>(a.P.gamma, u, F);
#pragma unroll
          for (int f = 0; f < NF; f++)
#pragma unroll
            for (int l = 0; l < ND; l++)
            {
              double t = 0.0;
#pragma unroll
              for (int n = 0; n < ND; n++) t += JG[l + ND * n] * F[f + NF * n];
              Gr[(mm * GP + el) * NC + f + NF * l] = t;
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < TRIPS; t++)
        {
          const int q = tid + t * T;
          if (q < items_u)
          {
            const int el = q / NU, j = q - el * NU;
            for (int mm = 0; mm < ch; mm++)
            {
              const double m = Fl[j + NU * mm];
#pragma unroll
              for (int c = 0; c < NC; c++) oi[t][c] += m * Gr[(mm * GP + el) * NC + c];
            }
          }
        }
        __syncthreads(); // (the next chunk's slices, or the corrections, overwrite D; the next chunk's fluxes Gr)
      }
    }
    if (visc)
      for (int q = tid; q < items_f; q += T)
      {
        const int el = q / NFP, j = q - el * NFP;
        const long o = e0 * NFP + q;
        double r[NF];
        if (a.nbr == nullptr)
        {
#pragma unroll
          for (int f = 0; f < NF; f++) r[f] = a.delta[o + f * plane_f];
        }
        else
        {
          // delta = u_common - u_own, u_common = (u_L + u_R)/2 - beta (u_L - u_R) on the pair's orientation (src/inters.cpp:637)
          const int w = a.nbr[o];
          const bool remote = w >= 0 && (w & 4); // the partner of a partition point: in the receive record
          const double *pp = (w < 0) ? a.delta + o : (remote ? a.in_disu : a.disu) + (w >> 4);
          const long stride = remote ? (long)a.nfpi : plane_f;
          double own[NF], oth[NF];
#pragma unroll
          for (int f = 0; f < NF; f++)
          {
            own[f] = a.disu[o + f * plane_f];
            oth[f] = pp[f * stride];
          }
          const double beta = ldg_beta(w, a.P);
#pragma unroll
          for (int f = 0; f < NF; f++)
          {
            const double ul = (w & 1) ? oth[f] : own[f], ur = (w & 1) ? own[f] : oth[f];
            const double uc = 0.5 * (ul + ur) - beta * (ul - ur);
            r[f] = (w < 0) ? oth[f] : uc - own[f];
          }
        }
#pragma unroll
        for (int f = 0; f < NF; f++) D[(j * GP + el) * NF + f] = r[f];
      }
    __syncthreads();

    [[maybe_unused]] double fnr[LES ? TRIPS_F : 1][NF]; // (LES: the projected viscous flux of the lane's flux points, P2 to P3b)
    if (visc)
    {
      // ---- P1: reference-space corrected gradient at the solution points (calculate_gradient + first half of correct_gradient,
      //          src/eles.cpp:1823,1900): Gr(f,d) = opp_4[d] U(f) + opp_5[d] D(f)
      for (int q = tid; q < items_u; q += T)
      {
        const int el = q / NU, i = q - el * NU;
        double acc[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = 0.0;
#pragma unroll 2
        for (int k = 0; k < NU; k++)
        {
          const double m0 = o4[i + NU * k], m1 = o4[NU * NU + i + NU * k];
#pragma unroll
          for (int f = 0; f < NF; f++)
          {
            const double u = U[(k * GP + el) * NF + f];
            acc[f] += m0 * u;
            acc[f + NF] += m1 * u;
          }
        }
#pragma unroll 2
        for (int j = 0; j < NFP; j++)
        {
          const double m0 = o5[i + NU * j], m1 = o5[NU * NFP + i + NU * j];
#pragma unroll
          for (int f = 0; f < NF; f++)
          {
            const double dl = D[(j * GP + el) * NF + f];
            acc[f] += m0 * dl;
            acc[f + NF] += m1 * dl;
          }
        }
#pragma unroll
        for (int c = 0; c < NC; c++) Gr[(i * GP + el) * NC + c] = acc[c];
      }
      __syncthreads();

      // ---- P2: gradient at the flux points (second half of correct_gradient: opp_6, then the transform with the flux points' own
      //          metrics, src/eles.cpp:1930,1998) and the viscous flux there, projected on the point's normal
      // (LES: trip t takes the lane's ONE point tid + t T -- the inner loop runs at most once -- so that its Fn stays in fnr[t])
      constexpr int P2_TRIPS = LES ? TRIPS_F : 1, P2_STEP = LES ? T * TRIPS_F : T;
#pragma unroll
      for (int t = 0; t < P2_TRIPS; t++)
      for (int q = tid + t * T; q < items_f; q += P2_STEP)
      {
        const int el = q / NFP, j = q - el * NFP;
        const long o = e0 * NFP + q;
        double JG[4], n[ND];
#pragma unroll
        for (int c = 0; c < 4; c++) JG[c] = a.JGinv_fpts[o * 4 + c];
        const double dj = a.detjac_fpts[o];
#pragma unroll
        for (int m = 0; m < ND; m++) n[m] = a.norm_fpts[o + m * plane_f];
        const bool bdy = a.grad_fpts != nullptr && (a.meta[o] & 4);
        double acc[NC], u[NF];
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = 0.0;
#pragma unroll
        for (int f = 0; f < NF; f++) u[f] = 0.0;
#pragma unroll 2
        for (int k = 0; k < NU; k++)
        {
          const double m6 = o6[j + NFP * k], m0 = o0[j + NFP * k];
#pragma unroll
          for (int c = 0; c < NC; c++) acc[c] += m6 * Gr[(k * GP + el) * NC + c];
#pragma unroll
          for (int f = 0; f < NF; f++) u[f] += m0 * U[(k * GP + el) * NF + f];
        }
        double g[NC], fv[NC];
        const double idj = 1.0 / dj;
#pragma unroll
        for (int f = 0; f < NF; f++)
        {
          const double tg[ND] = {acc[f], acc[f + NF]};
          double cg[ND];
          s2d_to_physical(idj, JG, tg, cg);
#pragma unroll
          for (int d = 0; d < ND; d++) g[f + NF * d] = cg[d];
        }
        if (bdy) // boundary point: the boundary kernel reads the gradient
#pragma unroll
          for (int c = 0; c < NC; c++) a.grad_fpts[o + c * plane_f] = g[c];
        calc_visf<ND, true>(a.P, u, g, fv);
#pragma unroll
        for (int f = 0; f < NF; f++)
        {
          double s = 0.0;
#pragma unroll
          for (int m = 0; m < ND; m++) s += fv[f + NF * m] * n[m];
          if constexpr (LES) fnr[t][f] = s; // (stored once, by P3b)
          else a.fn[o + f * plane_f] = s;
        }
      }
      __syncthreads();
    }

    // ---- P3: point physics at the solution points (evaluate_invFlux, the transform of correct_gradient, evaluate_viscFlux;
    //          src/eles.cpp:1415,1973,2285): Gr(f,d) <- transformed total flux
    if constexpr (LES)
    {
      double tiv[TRIPS][NC]; // transformed inviscid + viscous flux of the lane's solution points
#pragma unroll
      for (int t = 0; t < TRIPS; t++)
      {
        const int q = tid + t * T;
        if (q < items_u)
        {
          const int el = q / NU, i = q - el * NU;
          const long o = e0 * NU + q;
          double JG[4];
#pragma unroll
          for (int c = 0; c < 4; c++) JG[c] = a.JGinv_upts[o * 4 + c];
          const double idj = 1.0 / a.detjac_upts[o], len2 = a.les_len2[o];
          double u[NF], F[NC], g[NC], fv[NC], sg[NC];
#pragma unroll
          for (int f = 0; f < NF; f++) u[f] = U[(i * GP + el) * NF + f];
          calc_invf<ND, true>(a.P.gamma, u, F);
#pragma unroll
          for (int f = 0; f < NF; f++)
          {
            const double tg[ND] = {Gr[(i * GP + el) * NC + f], Gr[(i * GP + el) * NC + f + NF]};
            double cg[ND];
            s2d_to_physical(idj, JG, tg, cg);
#pragma unroll
            for (int d = 0; d < ND; d++) g[f + NF * d] = cg[d];
          }
          calc_visf<ND, true>(a.P, u, g, fv);
          calc_sgsf_fast<ND>(a.P, a.les, u, g, len2, o, plane_u, sg);
#pragma unroll
          for (int f = 0; f < NF; f++)
#pragma unroll
            for (int l = 0; l < ND; l++)
            {
              double tt = 0.0, ts = 0.0;
#pragma unroll
              for (int m = 0; m < ND; m++)
              {
                tt += JG[l + ND * m] * (F[f + NF * m] + fv[f + NF * m]);
                ts += JG[l + ND * m] * sg[f + NF * m];
              }
              tiv[t][f + NF * l] = tt;
              Gr[(i * GP + el) * NC + f + NF * l] = ts;
            }
        }
      }
      __syncthreads();
      // ---- P3b: F~_sgs . n~ at the flux points (opp_1) joins the Fn of P2, which is stored here
#pragma unroll
      for (int t = 0; t < TRIPS_F; t++)
      {
        const int q = tid + t * T;
        if (q < items_f)
        {
          const int el = q / NFP, j = q - el * NFP;
          const long o = e0 * NFP + q;
          const double tdA = a.tdA_fpts[o];
          double acc[NF];
#pragma unroll
          for (int f = 0; f < NF; f++) acc[f] = 0.0;
#pragma unroll 2
          for (int k = 0; k < NU; k++)
          {
            const double m0 = o1[j + NFP * k], m1 = o1[NFP * NU + j + NFP * k];
#pragma unroll
            for (int f = 0; f < NF; f++) acc[f] += m0 * Gr[(k * GP + el) * NC + f] + m1 * Gr[(k * GP + el) * NC + f + NF];
          }
#pragma unroll
          for (int f = 0; f < NF; f++) a.fn[o + f * plane_f] = fnr[t][f] + acc[f] / tdA;
        }
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < TRIPS; t++)
      {
        const int q = tid + t * T;
        if (q < items_u)
        {
          const int el = q / NU, i = q - el * NU;
#pragma unroll
          for (int c = 0; c < NC; c++) Gr[(i * GP + el) * NC + c] += tiv[t][c];
        }
      }
    }
    else if constexpr (OVERINT == S2dOverInt::none)
    {
      for (int q = tid; q < items_u; q += T)
      {
        const int el = q / NU, i = q - el * NU;
        const long o = e0 * NU + q;
        double JG[4];
#pragma unroll
        for (int c = 0; c < 4; c++) JG[c] = a.JGinv_upts[o * 4 + c];
        const double dj = visc ? a.detjac_upts[o] : 1.0;
        double u[NF], F[NC];
#pragma unroll
        for (int f = 0; f < NF; f++) u[f] = U[(i * GP + el) * NF + f];
        calc_invf<ND, true>(a.P.gamma, u, F);
        if (visc)
        {
          const double idj = 1.0 / dj;
          double g[NC], fv[NC];
#pragma unroll
          for (int f = 0; f < NF; f++)
          {
            const double tg[ND] = {Gr[(i * GP + el) * NC + f], Gr[(i * GP + el) * NC + f + NF]};
            double cg[ND];
            s2d_to_physical(idj, JG, tg, cg);
#pragma unroll
            for (int d = 0; d < ND; d++) g[f + NF * d] = cg[d];
          }
          calc_visf<ND, true>(a.P, u, g, fv);
#pragma unroll
          for (int c = 0; c < NC; c++) F[c] += fv[c];
        }
#pragma unroll
        for (int f = 0; f < NF; f++)
#pragma unroll
          for (int l = 0; l < ND; l++)
          {
            double t = 0.0;
#pragma unroll
            for (int m = 0; m < ND; m++) t += JG[l + ND * m] * F[f + NF * m];
            Gr[(i * GP + el) * NC + f + NF * l] = t;
          }
      }
    }
    else
    {
      // (over-integration: the transformed inviscid flux is the de-aliased one -- the lane's accumulators, or tdisf_upts -- and the
      // transformed viscous flux is added to it as eles::evaluate_viscFlux does; calc_invf is not called here)
#pragma unroll
      for (int t = 0; t < TRIPS; t++)
      {
        const int q = tid + t * T;
        if (q < items_u)
        {
          const int el = q / NU, i = q - el * NU;
          const long o = e0 * NU + q;
          double td[NC];
#pragma unroll
          for (int c = 0; c < NC; c++)
          {
            if constexpr (OVERINT == S2dOverInt::folded) td[c] = oi[t][c];
            else td[c] = a.tdisf_in[o + c * plane_u];
          }
          if (visc)
          {
            double JG[4];
#pragma unroll
            for (int c = 0; c < 4; c++) JG[c] = a.JGinv_upts[o * 4 + c];
            const double idj = 1.0 / a.detjac_upts[o];
            double u[NF], g[NC], fv[NC];
#pragma unroll
            for (int f = 0; f < NF; f++) u[f] = U[(i * GP + el) * NF + f];
#pragma unroll
            for (int f = 0; f < NF; f++)
            {
              const double tg[ND] = {Gr[(i * GP + el) * NC + f], Gr[(i * GP + el) * NC + f + NF]};
              double cg[ND];
              s2d_to_physical(idj, JG, tg, cg);
#pragma unroll
              for (int d = 0; d < ND; d++) g[f + NF * d] = cg[d];
            }
            calc_visf<ND, true>(a.P, u, g, fv);
#pragma unroll
            for (int f = 0; f < NF; f++)
#pragma unroll
              for (int l = 0; l < ND; l++)
#pragma unroll
                for (int m = 0; m < ND; m++) td[f + NF * l] += JG[l + ND * m] * fv[f + NF * m];
          }
#pragma unroll
          for (int c = 0; c < NC; c++) Gr[(i * GP + el) * NC + c] = td[c];
        }
      }
    }
    __syncthreads();

    // ---- P4: discontinuous divergence (opp_2) and normal flux at the flux points (opp_1), summed over the dimensions
    //          (calculate_divergence, extrapolate_totalFlux; src/eles.cpp:1651,1549)
    for (int q = tid; q < items_u + items_f; q += T)
    {
      const bool is_div = q < items_u;
      const int qq = is_div ? q : q - items_u, n = is_div ? NU : NFP;
      const int el = qq / n, r = qq - el * n;
      const double *op = is_div ? o2 : o1;
      double acc[NF];
#pragma unroll
      for (int f = 0; f < NF; f++) acc[f] = 0.0;
#pragma unroll 2
      for (int k = 0; k < NU; k++)
      {
        const double m0 = op[r + n * k], m1 = op[n * NU + r + n * k];
#pragma unroll
        for (int f = 0; f < NF; f++) acc[f] += m0 * Gr[(k * GP + el) * NC + f] + m1 * Gr[(k * GP + el) * NC + f + NF];
      }
      double *out = is_div ? a.div + e0 * NU + qq : a.ntd + e0 * NFP + qq;
      const long plane = is_div ? plane_u : plane_f;
#pragma unroll
      for (int f = 0; f < NF; f++) out[f * plane] = acc[f];
    }
    // (the next group's P0 writes U and D, which P4 does not read; its P1 writes Gr behind a barrier every thread has passed)
  }
}

// ---------------------------------------------------------------------------------------------------------------
// update kernel: div_tdisf + opp_3 (norm_tconf - norm_tdisf) -> RK update -> disu_fpts of the new state
// (calculate_corrected_divergence, AdvanceSolution, extrapolate_solution; src/eles.cpp:1738,1080,1360); as general_update_kernel
//
// SHOCK: eles::shock_capture (src/eles.cpp:2918-2959) with the triangle's own sensor (eles_tris::shock_det_persson,
// src/eles_tris.cpp:472-524) between the RK update and the opp_0 pass, on the group's new state in LDS:
//   modal   lane (element, mode m): u^_m = sum_k inv_vandermonde(m, k) S[k][element][field], ascending k; u^_m^2 -> M
//   sensor  one lane per element: tail (m >= NHI = p (p + 1) / 2) and all modes summed in ascending order (accumulate), divided,
//           stored to sensor(n_eles) and kept in LDS.  Every mode norm is one; nothing crosses lanes: bit-reproducible
//   filter  the lanes of an element with sensor >= s0 (a NaN compares false) form exp_filter . S for the four fields in registers,
//           the others take their own point; behind a barrier every lane stores its point ONCE to disu_upts(0), the filtered
//           ones to S as well, so that the opp_0 pass extrapolates the filtered state
// With SHOCK false the kernel is the code without any of it.
// ---------------------------------------------------------------------------------------------------------------
template <int NU, int NFP, int G, bool SHOCK>
__global__ __launch_bounds__(S2D_T) void simplex2d_update_kernel_t(const S2dArgs a)
{
  constexpr int NF = S2D_NF, T = S2D_T, GP = G + 1;
  constexpr int NHI = simplex2d_first_high_mode(NU);
  constexpr int TRIPS = (NU * G + T - 1) / T; // points of a group per lane
  extern __shared__ double lds[];
  double *o3 = lds;              // NU x NFP
  double *o0 = o3 + NU * NFP;    // NFP x NU
  double *iv = o0 + NFP * NU;    // NU x NU  inv_vandermonde  (SHOCK)
  double *ef = iv + NU * NU;     // NU x NU  exp_filter       (SHOCK)
  double *X = o0 + NFP * NU + (SHOCK ? 2 * NU * NU : 0); // [NFP][GP][NF]  norm_tconf - norm_tdisf
  double *S = X + NFP * GP * NF; // [NU][GP][NF]   the new state
  double *M = S + NU * GP * NF;  // [GP][NU]       squared modal coefficients of the sensor field (SHOCK)
  double *Sen = M + NU * GP;     // [GP]           the group's sensors (SHOCK)
  static_assert(simplex2d_update_lds_bytes(NU, NFP, G, SHOCK) ==
                    sizeof(double) * (simplex2d_update_ops(NU, NFP, SHOCK) + (size_t)GP * (NU * NF + NFP * NF + (SHOCK ? NU + 1 : 0))), "LDS image");
  static_assert(simplex2d_update_lds_bytes(NU, NFP, G, SHOCK) <= SIMPLEX2D_LDS_BUDGET, "LDS budget");
  static_assert(G <= T, "one lane per element in the sensor pass");
  const int tid = threadIdx.x;
  const long plane_u = (long)NU * a.n_eles, plane_f = (long)NFP * a.n_eles;
  s2d_stage_ops(lds, a.ops, (int)simplex2d_update_ops(NU, NFP, SHOCK), tid);

  const int n_walk = a.groups ? a.n_list : a.n_groups;
  for (int it = blockIdx.x; it < n_walk; it += gridDim.x)
  {
    const int grp = a.groups ? a.groups[it] : it;
    const long e0 = (long)grp * G;
    const int nval = (int)min((long)G, a.n_eles - e0);
    const int items_u = NU * nval, items_f = NFP * nval;
    for (int q = tid; q < items_f; q += T)
    {
      const int el = q / NFP, j = q - el * NFP;
      const long o = e0 * NFP + q;
      double r[NF];
#pragma unroll
      for (int f = 0; f < NF; f++) r[f] = a.tconf[o + f * plane_f] + -1.0 * a.ntd[o + f * plane_f]; // the daxpy of src/eles.cpp:1746
#pragma unroll
      for (int f = 0; f < NF; f++) X[(j * GP + el) * NF + f] = r[f];
    }
    __syncthreads();
    for (int q = tid; q < items_u; q += T)
    {
      const int el = q / NU, i = q - el * NU;
      const long p = e0 * NU + q;
      // the update's inputs are requested before the contraction
      const double dj = a.detjac_upts[p];
      const double dt = a.dt_local_on ? a.dt_local[e0 + el] : a.dt;
      double dvin[NF], un[NF], u1v[NF], sv[NF];
#pragma unroll
      for (int f = 0; f < NF; f++)
      {
        const long ok = p + f * plane_u;
        dvin[f] = a.div[ok];
        un[f] = a.u0w[ok];
        u1v[f] = a.need_u1 ? a.u1[ok] : 0.0;
        sv[f] = a.src ? a.src[ok] : 0.0;
      }
      double acc[NF];
#pragma unroll
      for (int f = 0; f < NF; f++) acc[f] = 0.0;
#pragma unroll 2
      for (int j = 0; j < NFP; j++)
      {
        const double m = o3[i + NU * j];
#pragma unroll
        for (int f = 0; f < NF; f++) acc[f] += m * X[(j * GP + el) * NF + f];
      }
#pragma unroll
      for (int f = 0; f < NF; f++)
      {
        const long ok = p + f * plane_u;
        const double dv = dvin[f] + acc[f];
        if (dv != dv) atomicMin(a.nan_flag, (unsigned long long)ok);
        if (a.write_div) a.div[ok] = dv;
        const double s = sv[f];
        const double dd = dv / dj;
        double u = un[f];
        if (a.adv_type == 0)
          u -= dt * (dd - s);
        else if (a.adv_type == 1)
        {
          if (a.in_step == 0) a.u1[ok] = u;
          if (a.in_step < 3)
            u -= dt / 3.0 * (dd - s);
          else
          {
            const double rhs = -dd + s;
            u = 3.0 / 4.0 * u + 1.0 / 4.0 * u1v[f] + dt / 4.0 * rhs;
          }
        }
        else if (a.adv_type == 2)
        {
          if (a.in_step == 0) a.u1[ok] = u;
          if (a.in_step < 2 || a.in_step == 3)
            u -= dt / 2.0 * (dd - s);
          else if (a.in_step == 2)
          {
            const double rhs = -dd + s;
            u = 1.0 / 3.0 * u + 2.0 / 3.0 * u1v[f] + dt / 6.0 * rhs;
          }
        }
        else
        {
          const double rhs = -dd + s;
          const double r1 = a.rk_a * u1v[f] + dt * rhs;
          a.u1[ok] = r1;
          u += a.rk_b * r1;
        }
        if constexpr (!SHOCK) a.u0w[ok] = u; // (SHOCK: stored once, behind the filter)
        S[(i * GP + el) * NF + f] = u;
      }
    }
    __syncthreads();
    if constexpr (SHOCK)
    {
      // ---- modal coefficients of the sensor field, squared
      for (int q = tid; q < items_u; q += T)
      {
        const int el = q / NU, m = q - el * NU;
        double acc = 0.0;
#pragma unroll 2
        for (int k = 0; k < NU; k++) acc += iv[m + NU * k] * S[(k * GP + el) * NF + a.sens_field];
        M[q] = acc * acc;
      }
      __syncthreads();
      // ---- the sensor, one lane per element of the group (a padded element of the last group has none)
      if (tid < nval)
      {
        double hi = 0.0, all = 0.0;
        for (int m = NHI; m < NU; m++) hi += M[tid * NU + m];
        for (int m = 0; m < NU; m++) all = all + M[tid * NU + m];
        const double sen = hi / all;
        a.sensor[e0 + tid] = sen;
        Sen[tid] = sen;
      }
      __syncthreads();
      // ---- the filter where the sensor fires; every point reaches disu_upts(0) from here
      double r[TRIPS][NF];
      bool filt[TRIPS];
#pragma unroll
      for (int t = 0; t < TRIPS; t++)
      {
        const int q = tid + t * T;
        filt[t] = false;
        if (q < items_u)
        {
          const int el = q / NU, i = q - el * NU;
          filt[t] = Sen[el] >= a.s0;
          if (filt[t])
          {
#pragma unroll
            for (int f = 0; f < NF; f++) r[t][f] = 0.0;
#pragma unroll 2
            for (int k = 0; k < NU; k++)
            {
              const double m = ef[i + NU * k];
#pragma unroll
              for (int f = 0; f < NF; f++) r[t][f] += m * S[(k * GP + el) * NF + f];
            }
          }
          else
#pragma unroll
            for (int f = 0; f < NF; f++) r[t][f] = S[(i * GP + el) * NF + f];
        }
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < TRIPS; t++)
      {
        const int q = tid + t * T;
        if (q < items_u)
        {
          const int el = q / NU, i = q - el * NU;
#pragma unroll
          for (int f = 0; f < NF; f++) a.u0w[e0 * NU + q + f * plane_u] = r[t][f];
          if (filt[t])
#pragma unroll
            for (int f = 0; f < NF; f++) S[(i * GP + el) * NF + f] = r[t][f];
        }
      }
      __syncthreads();
    }
    for (int q = tid; q < items_f; q += T)
    {
      const int el = q / NFP, j = q - el * NFP;
      double acc[NF];
#pragma unroll
      for (int f = 0; f < NF; f++) acc[f] = 0.0;
#pragma unroll 2
      for (int k = 0; k < NU; k++)
      {
        const double m = o0[j + NFP * k];
#pragma unroll
        for (int f = 0; f < NF; f++) acc[f] += m * S[(k * GP + el) * NF + f];
      }
#pragma unroll
      for (int f = 0; f < NF; f++) a.disu_next[e0 * NFP + q + f * plane_f] = acc[f];
    }
    // (the next group's staging writes X, which the opp_0 pass does not read; its opp_3 pass writes S behind a barrier)
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static int simplex2d_size_class(const hfx_eles *e)
{
  const int first = e->ele_type == 1 ? N_SIMPLEX2D_SIZES : 0, last = e->ele_type == 1 ? N_S2D_CLASSES : N_SIMPLEX2D_SIZES;
  for (int i = first; i < last; i++)
    if (e->n_upts == s2d_class_row(i)[0] && e->n_fpts == s2d_class_row(i)[1]) return i;
  return -1;
}

static bool is_block2d(const hfx_eles *e) { return e && e->n_dims == 2 && (e->ele_type == 0 || e->ele_type == 1); }

bool simplex2d_runs(const hfx_eles *e)
{
  return is_simplex2d(e) || (is_block2d(e) && e->ctx->opt.blocks_2d && e->simplex2d && e->simplex2d->built);
}

bool simplex2d_stage_call(hfx_eles *const *eles, int neb)
{
  for (int i = 0; i < neb; i++)
    if (!simplex2d_runs(eles[i])) return false;
  return neb > 0;
}

bool simplex2d_takes(hfx_eles *const *eles, int neb, bool partitioned)
{
  bool tri = false, any2d = false;
  for (int i = 0; i < neb; i++)
  {
    tri = tri || is_simplex2d(eles[i]);
    any2d = any2d || eles[i]->n_dims == 2;
  }
  return tri || (any2d && eles[0]->ctx->opt.blocks_2d && !(partitioned && neb == 1));
}

// the operators of `list` one behind the other, each dense column-major as registered; an operator the run does not have: zeros
static int packed_operators(DevBuf<double> &dst, std::initializer_list<const Operator *> list, std::initializer_list<size_t> sizes)
{
  std::vector<double> h;
  auto sz = sizes.begin();
  for (const Operator *op : list)
  {
    const size_t n = *sz++, at = h.size();
    h.resize(at + n, 0.0);
    if (!op->present()) continue;
    HFX_CHECK((size_t)op->m * op->k == n, "2-D simplex fused stage: an operator of %d x %d where %zu entries are expected", op->m, op->k, n);
    HFX_HIP(hipMemcpy(h.data() + at, op->dense, sizeof(double) * n, hipMemcpyDeviceToHost));
  }
  return dst.upload(h);
}

// The update kernel hard-codes the sensor of eles_tris::shock_det_persson (src/eles_tris.cpp:472-524): every mode norm one, the
// numerator's modes exactly those of total degree p, j >= p (p + 1) / 2.  nullptr: the registration (as hfx_eles_set_shock_capture
// kept it on the host) has that form; else what differs
static const char *shock_form_refusal(const hfx_eles *e)
{
  const int nu = e->n_upts, first = simplex2d_first_high_mode(nu);
  if ((int)e->h_persson_den.size() != nu || (int)e->h_persson_num.size() != nu) return "no registration is kept on the host";
  for (int j = 0; j < nu; j++)
    if (e->h_persson_den[j] != 1.0) return "a norm_basis_persson entry is not 1";
  for (int j = 0; j < nu; j++)
    if ((e->h_persson_num[j] != 0.0) != (j >= first)) return "high_modes is not the set of the modes of total degree p, j >= p (p + 1) / 2";
  return nullptr;
}

// The element kernel's LES form projects the SGS flux with the block's OWN metrics (opp_1, tdA_fpts) and never reads the registered
// Jacobian_fpts, with which hfx_eles_extrapolate_sgsFlux takes the extrapolated flux back to physical space: the two agree where
// sum_k Jacobian_fpts(i, k) JGinv_fpts(k, j) = detjac_fpts delta_ij at every flux point.  -> the largest miss, relative to
// max |detjac_fpts| (checked once per registration, on the host, a chunk of flux points at a time)
static int les_jacobian_residual(const hfx_eles *e, double *residual)
{
  const size_t plane_f = (size_t)e->n_fpts * e->n_eles, CHUNK = (size_t)1 << 18; // (flux points copied at a time: 18 MiB of host vectors)
  HFX_CHECK(e->Jacobian_fpts && e->JGinv_fpts && e->detjac_fpts, "2-D simplex fused stage: an LES closure without the flux points' metrics");
  std::vector<double> J(4 * std::min(plane_f, CHUNK)), JG(J.size()), dj(J.size() / 4);
  double miss = 0.0, scale = 0.0;
  for (size_t p0 = 0; p0 < plane_f; p0 += CHUNK)
  {
    const size_t n = std::min(CHUNK, plane_f - p0);
    HFX_HIP(hipMemcpy(J.data(), e->Jacobian_fpts.get() + 4 * p0, sizeof(double) * 4 * n, hipMemcpyDeviceToHost));
    HFX_HIP(hipMemcpy(JG.data(), e->JGinv_fpts.get() + 4 * p0, sizeof(double) * 4 * n, hipMemcpyDeviceToHost));
    HFX_HIP(hipMemcpy(dj.data(), e->detjac_fpts.get() + p0, sizeof(double) * n, hipMemcpyDeviceToHost));
    for (size_t p = 0; p < n; p++)
    {
      scale = std::max(scale, std::fabs(dj[p]));
      for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++)
        {
          double s = (i == j) ? -dj[p] : 0.0;
          for (int k = 0; k < 2; k++) s += J[4 * p + i + 2 * k] * JG[4 * p + k + 2 * j];
          miss = std::max(miss, std::fabs(s));
          if (s != s) miss = HUGE_VAL; // (a NaN in the registration conforms to nothing)
        }
    }
  }
  *residual = scale > 0.0 ? miss / scale : HUGE_VAL;
  return 0;
}

static int simplex2d_build(hfx_eles *e, hfx_inters *const *faces, int nfb, hfx_eles *const *blocks, int neb)
{
  HFX_CHECK(e->n_fields == 4, "2-D simplex fused stage: Navier-Stokes / Euler blocks only; run per method (fused 0)");
  HFX_CHECK(simplex2d_size_class(e) >= 0, "2-D simplex fused stage: built for triangles of orders 1..5 and quadrilaterals of orders 1..4 (%d solution, "
            "%d flux points on element class %d); run per method (fused 0)", e->n_upts, e->n_fpts, e->ele_type);
  HFX_CHECK(!(e->les_ready && e->over_int_ready), "2-D simplex fused stage: an LES closure beside over-integration runs per method (fused 0)");
  // (a conforming closure beside a conforming shock registration: the LES element kernel and the SHOCK update kernel -- or, with
  // option fold_shock 0, the filter behind the stage -- each as it runs alone)
  if (e->les_ready)
  {
    const int model = e->les.sgs_model;
    HFX_CHECK(e->ctx->params.viscous, "2-D simplex fused stage: an LES closure on an inviscid context runs per method (fused 0)");
    HFX_CHECK(model != 0 || e->wall_distance, "2-D simplex fused stage: an LES closure of the Smagorinsky model without wall_distance runs per method (fused 0)");
    HFX_CHECK(model < 2 || (e->filter_upts.present() && e->les.Lu && e->les.Le),
              "2-D simplex fused stage: an LES closure of model %d without filter_upts (hfx_eles_set_les_filter) runs per method (fused 0)", model);
    // (SVV filters the state after its flux-point values have left for the neighbours, as on the general stage)
    for (int b = 0; b < nfb; b++)
      HFX_CHECK(!faces[b]->is_mpi || model != 3, "2-D simplex fused stage: the SVV LES closure on partitioned blocks runs per method (fused 0)");
    if (model != 3)
    {
      double residual = 0.0;
      if (les_jacobian_residual(e, &residual)) return 1;
      HFX_CHECK(residual <= 1e-9, "2-D simplex fused stage: a registered LES closure whose Jacobian_fpts is not the block's own (Jacobian_fpts . JGinv_fpts "
                                  "misses detjac_fpts by %.3g of its largest value; the stage projects the SGS flux with tdA_fpts and opp_1) runs per method (fused 0)",
                residual);
    }
  }
  if (e->over_int_ready)
  {
    // (eles_tris::set_over_int, src/eles_tris.cpp:674-700: the cubature rule of over_int_order o = 0..7 has (o + 1)(o + 2) / 2 points)
    HFX_CHECK(simplex2d_cubature_order(e->n_cubpts) >= 0, "2-D simplex fused stage: registered over-integration with %d cubature points, "
              "which no triangle rule of over_int_order 0..7 has ((o + 1)(o + 2) / 2: 1..36), runs per method (fused 0)", e->n_cubpts);
    HFX_CHECK(e->opp_over_int_cubpts.present() && e->over_int_filter.present(), "2-D simplex fused stage: over-integration without its operators");
    HFX_CHECK(e->JGinv_over_int_cubpts.size() == (size_t)4 * e->n_cubpts * e->n_eles,
              "2-D simplex fused stage: JGinv_over_int_cubpts holds %zu doubles where 4 x %d x %d are expected", e->JGinv_over_int_cubpts.size(), e->n_cubpts, e->n_eles);
  }
  if (e->shock_ready)
  {
    const char *why = shock_form_refusal(e);
    HFX_CHECK(!why, "2-D simplex fused stage: registered shock capturing that is not the triangle's own sensor (eles_tris::shock_det_persson: %s) "
                    "runs per method (fused 0)", why);
    HFX_CHECK(e->inv_vandermonde.present() && e->exp_filter.present(), "2-D simplex fused stage: shock capturing without its operators");
  }
  const bool visc = e->ctx->params.viscous != 0;
  HFX_CHECK(!visc || e->viscous_ops, "2-D simplex fused stage: viscous run but the block has no opp_4/5/6");
  for (const Operator *op : {&e->opp_0, &e->opp_3, &e->opp_1[0], &e->opp_1[1], &e->opp_2[0], &e->opp_2[1]})
    HFX_CHECK(op->present(), "2-D simplex fused stage: an operator is missing");
  if (!e->simplex2d) e->simplex2d.reset(new Simplex2dData());
  Simplex2dData *g = e->simplex2d.get();
  g->built = false; // (until every table below is this registration's)
  const size_t nu = e->n_upts, nfp = e->n_fpts;
  if (packed_operators(g->element_ops, {&e->opp_4[0], &e->opp_4[1], &e->opp_5[0], &e->opp_5[1], &e->opp_6, &e->opp_0, &e->opp_2[0], &e->opp_2[1], &e->opp_1[0], &e->opp_1[1]},
                       {nu * nu, nu * nu, nu * nfp, nu * nfp, nfp * nu, nfp * nu, nu * nu, nu * nu, nfp * nu, nfp * nu}))
    return 1;
  if (packed_operators(g->update_ops, {&e->opp_3, &e->opp_0}, {nu * nfp, nfp * nu})) return 1;
  g->shock = false;
  g->update_shock_ops.reset();
  if (e->shock_ready && packed_operators(g->update_shock_ops, {&e->opp_3, &e->opp_0, &e->inv_vandermonde, &e->exp_filter}, {nu * nfp, nfp * nu, nu * nu, nu * nu}))
    return 1;
  g->shock = e->shock_ready;
  g->shock_serial = e->shock_serial;
  g->over_int = false;
  g->overint_ops.reset();
  if (e->over_int_ready && packed_operators(g->overint_ops, {&e->opp_over_int_cubpts, &e->over_int_filter}, {(size_t)e->n_cubpts * nu, nu * (size_t)e->n_cubpts}))
    return 1;
  g->over_int = e->over_int_ready;
  g->over_int_serial = e->over_int_serial;
  g->n_cub = e->over_int_ready ? e->n_cubpts : 0;
  g->les = false;
  g->les_len2.reset();
  const bool les = e->les_ready && e->les.sgs_model != 3; // (SVV has no SGS flux: the plain kernels behind the step loop's filter)
  if (les && les_len2_upload(e, g->les_len2)) return 1;
  g->les = les;
  g->les_serial = e->les_serial;
  // per flux point: the LDG switch of the pair it is the LEFT point of (exact tests on the left normal, decided once), whether a
  // boundary face owns it, and its partner word; every flux point must belong to exactly one registered face
  const long plane_f = (long)nfp * e->n_eles;
  HFX_CHECK(plane_f < (1L << 27), "2-D simplex fused stage: %ld flux points do not fit a partner word", plane_f);
  std::vector<unsigned char> meta(plane_f, 0);
  std::vector<char> owned(plane_f, 0);
  std::vector<int> nbr(plane_f, -1);
  std::vector<double> norm((size_t)plane_f * 2);
  HFX_HIP(hipMemcpy(norm.data(), e->norm_fpts, sizeof(double) * norm.size(), hipMemcpyDeviceToHost));
  g->any_bdy = g->any_int = g->any_mpi = false;
  g->n_cross_pts = 0;
  // partition faces (the partitioned stage): a partition point is owned by its face like every other point and carries no boundary
  // bit; its common flux comes from the one-sided kernels of kernels_mpi.hpp.  Its LDG correction: with ONE partition-face block
  // the element kernel reads the partner from that block's receive record (remote word; the switch from the point's OWN normal, as
  // mpi_delta_kernel<2> decides it); with several blocks the word stays -1 and mpi_delta_kernel<2> writes delta_disu_fpts
  int n_mpi_blocks = 0;
  for (int b = 0; b < nfb; b++) n_mpi_blocks += faces[b]->is_mpi && faces[b]->n_inters > 0;
  g->remote_face = nullptr;
  const int G = s2d_class_row(simplex2d_size_class(e))[2];
  const int n_groups = (e->n_eles + G - 1) / G;
  std::vector<char> partition_group(n_groups, 0);
  for (int b = 0; b < nfb; b++)
  {
    hfx_inters *f = faces[b];
    if (f->left != e && f->right != e) continue; // (a face block of the call's other element blocks)
    if (f->is_mpi)
    {
      const long np = (long)f->n_inters * f->n_fpts_per_inter;
      const bool remote = n_mpi_blocks == 1 && np * e->n_fields < (1L << 27);
      if (remote && np > 0) g->remote_face = f;
      for (long q = 0; q < np; q++)
      {
        const int il = f->hL[q];
        owned[il]++;
        partition_group[(il / (int)nfp) / G] = 1;
        g->any_mpi = true;
        if (!remote) continue;
        const double n[2] = {norm[il], norm[il + plane_f]};
        const int flip = ldg_switch<2>(1.0, n) < 0 ? 2 : 0;
        const long i = q / f->n_fpts_per_inter;
        const long slot = f->hR[q] + (long)f->n_fpts_per_inter * e->n_fields * i; // field 0 of the partner in the record of face i
        nbr[il] = (int)(slot << 4) | 4 | flip;
      }
      continue;
    }
    if (f->is_bdy)
    {
      g->any_bdy = g->any_bdy || f->n_inters > 0;
      for (int o : f->hL) { meta[o] |= 4; owned[o]++; }
      continue;
    }
    const long np = (long)f->n_inters * f->n_fpts_per_inter;
    if (f->left != f->right)
    {
      // a cross block: its left points are this block's where it is the left one (with the pair's switch bit, from the left
      // normal), its right points where it is the right one; the partner word stays -1 (the partner lies in another block's
      // arrays) and face_delta_kernel<2> writes the correction
      const bool is_left = f->left == e;
      const std::vector<int> &mine = is_left ? f->hL : f->hR;
      for (long q = 0; q < np; q++)
      {
        const int o = mine[q];
        HFX_CHECK(o >= 0 && o < plane_f, "2-D simplex fused stage: a face block addresses flux point %d of a block with %ld", o, plane_f);
        owned[o]++;
        if (is_left)
        {
          const double n[2] = {norm[o], norm[o + plane_f]};
          meta[o] |= ldg_switch<2>(1.0, n) < 0 ? 2 : 0;
        }
      }
      g->n_cross_pts += np;
      continue;
    }
    for (long q = 0; q < np; q++)
    {
      const int il = f->hL[q], ir = f->hR[q];
      owned[il]++; owned[ir]++;
      const double n[2] = {norm[il], norm[il + plane_f]};
      const int flip = ldg_switch<2>(1.0, n) < 0 ? 2 : 0;
      meta[il] |= flip;
      nbr[il] = (ir << 4) | flip;
      nbr[ir] = (il << 4) | flip | 1;
      g->any_int = true;
    }
  }
  for (long o = 0; o < plane_f; o++) HFX_CHECK(owned[o] == 1, "2-D simplex fused stage: flux point %ld belongs to %d registered faces", o, (int)owned[o]);
  if (g->meta.upload(meta) || g->nbr.upload(nbr)) return 1;
  if (g->disu_alt.ensure((size_t)plane_f * e->n_fields) || g->fn_fpts.ensure((size_t)plane_f * e->n_fields)) return 1;
  {
    // the two group lists of the partitioned stage (the last partial group is on the list its elements put it on)
    std::vector<int> part, inter;
    for (int grp = 0; grp < n_groups; grp++) (partition_group[grp] ? part : inter).push_back(grp);
    g->n_partition_groups = (int)part.size();
    g->n_interior_groups = (int)inter.size();
    g->partition_groups.reset();
    g->interior_groups.reset();
    if (!part.empty() && g->partition_groups.upload(part)) return 1;
    if (!inter.empty() && g->interior_groups.upload(inter)) return 1;
  }
  g->built_with.assign(faces, faces + nfb);
  g->built_blocks.assign(blocks, blocks + neb);
  g->built = true;
  return 0;
}

// Several two-dimensional blocks, or one block of quadrilaterals (option blocks_2d): each block its own tables, made from the face
// blocks that touch it.  Only the plain stage: whatever a block has registered beyond it is refused here, before anything is launched
static int simplex2d_prepare_blocks(hfx_eles *const *eles, int neb, hfx_inters *const *faces, int nfb)
{
  for (int i = 0; i < neb; i++)
  {
    const hfx_eles *e = eles[i];
    HFX_CHECK(e->n_dims == 2, "2-D simplex fused stage: a three-dimensional block beside a two-dimensional one runs per method (fused 0)");
    HFX_CHECK(is_block2d(e), "2-D simplex fused stage: element class %d is neither triangles nor quadrilaterals; run per method (fused 0)", e->ele_type);
    HFX_CHECK(e->n_eles > 0, "2-D simplex fused stage: empty element block");
    HFX_CHECK(e->order == eles[0]->order, "2-D simplex fused stage: element blocks of different order (%d beside %d) run per method (fused 0)",
              e->order, eles[0]->order);
    HFX_CHECK(!e->les_ready, "2-D simplex fused stage: a registered LES closure on one of several blocks, or on quadrilaterals, runs per method (fused 0)");
    HFX_CHECK(!e->over_int_ready, "2-D simplex fused stage: registered over-integration on one of several blocks, or on quadrilaterals, runs per method (fused 0)");
    HFX_CHECK(!e->shock_ready, "2-D simplex fused stage: registered shock capturing on one of several blocks, or on quadrilaterals, runs per method (fused 0)");
    HFX_CHECK(!e->ctx->params.viscous || e->viscous_ops, "2-D simplex fused stage: viscous run but a block has no opp_4/5/6");
  }
  for (int b = 0; b < nfb; b++)
    HFX_CHECK(!faces[b]->is_mpi, "2-D simplex fused stage: a partition-face block on several two-dimensional blocks, or on quadrilaterals, runs per method (fused 0)");
  for (int i = 0; i < neb; i++)
  {
    const Simplex2dData *g = eles[i]->simplex2d.get();
    if (g && g->built && !g->shock && !g->over_int && !g->les && g->built_with.size() == (size_t)nfb && std::equal(g->built_with.begin(), g->built_with.end(), faces) &&
        g->built_blocks.size() == (size_t)neb && std::equal(g->built_blocks.begin(), g->built_blocks.end(), eles))
      continue;
    if (simplex2d_build(eles[i], faces, nfb, eles, neb)) return 1;
  }
  return 0;
}

int simplex2d_prepare(hfx_eles *const *eles, int neb, hfx_inters *const *faces, int nfb, bool partitioned)
{
  const bool blocks_2d = eles[0]->ctx->opt.blocks_2d != 0;
  HFX_CHECK(neb == 1 || (blocks_2d && !partitioned),
            "2-D simplex fused stage: several element blocks of which one is two-dimensional (a mixed quadrilateral / triangle mesh) run per method "
            "(fused 0)%s", partitioned ? " in the partitioned loop" : "; hfx_run_steps_blocks takes them with option blocks_2d 1");
  if (neb > 1 || !is_simplex2d(eles[0])) return simplex2d_prepare_blocks(eles, neb, faces, nfb);
  hfx_eles *e = eles[0];
  HFX_CHECK(e->n_eles > 0, "2-D simplex fused stage: empty element block");
  if (!partitioned)
    for (int b = 0; b < nfb; b++)
      HFX_CHECK(!faces[b]->is_mpi, "2-D simplex fused stage: partition faces on a triangle block run in the partitioned loop "
                                   "(hfx_run_steps_partitioned_blocks) or per method (fused 0)");
  for (int b = 0; b < nfb; b++)
    HFX_CHECK(faces[b]->left == e && (faces[b]->right == nullptr || faces[b]->right == e), "face block %d refers to an element block that is not part of this call", b);
  // (what refuses a block is asked every time: a closure registered, or a context made viscous, behind the first stage must not
  // run on the tables of the stage before)
  HFX_CHECK(!e->ctx->params.viscous || e->viscous_ops, "2-D simplex fused stage: viscous run but the block has no opp_4/5/6");
  const Simplex2dData *g = e->simplex2d.get();
  // (shock capturing: the tables are those of the registration they were made from; a later one, conforming or not, rebuilds them)
  // (over-integration likewise: over_int_serial; an LES closure: les_serial -- and what refuses a closure depends on the context and
  // on the face blocks, so a block with a closure is rebuilt unless it is the one the tables took, on a viscous context)
  const bool les_same = g && (e->les_ready ? g->les_serial == e->les_serial && g->les == (e->les.sgs_model != 3) && e->ctx->params.viscous != 0 && !e->over_int_ready
                                           : !g->les);
  if (g && g->built && les_same && g->shock == e->shock_ready && g->shock_serial == e->shock_serial &&
      g->over_int == e->over_int_ready && g->over_int_serial == e->over_int_serial &&
      g->built_with.size() == (size_t)nfb &&
      std::equal(g->built_with.begin(), g->built_with.end(), faces) && g->built_blocks.size() == 1 && g->built_blocks[0] == e)
    return 0;
  return simplex2d_build(e, faces, nfb, eles, 1);
}

Simplex2dPlan simplex2d_plan(const hfx_eles *e)
{
  Simplex2dPlan pl;
  pl.size_class = simplex2d_size_class(e);
  if (pl.size_class < 0) return pl;
  const int *s = s2d_class_row(pl.size_class);
  pl.group = s[2];
  pl.gather = e->ctx->opt.gather_delta && e->ctx->params.viscous && e->simplex2d && (e->simplex2d->any_int || e->simplex2d->remote_face);
  pl.element_lds = simplex2d_element_lds_bytes(s[0], s[1], s[2]);
  pl.update_lds = simplex2d_update_lds_bytes(s[0], s[1], s[2]);
  pl.update_shock_lds = simplex2d_update_lds_bytes(s[0], s[1], s[2], true);
  const Simplex2dData *g = e->simplex2d.get();
  pl.fold_shock = e->ctx->opt.fold_shock && e->shock_ready && g && g->built && g->shock && g->shock_serial == e->shock_serial;
  pl.over_int = e->over_int_ready && g && g->built && g->over_int && g->over_int_serial == e->over_int_serial;
  pl.fold_over_int = pl.over_int && e->ctx->opt.fold_over_int;
  pl.n_cubpts = pl.over_int ? g->n_cub : 0;
  pl.over_int_chunk = s[0];
  pl.sgs_model = e->les_ready ? e->les.sgs_model : -1;
  pl.les = e->les_ready && e->les.sgs_model != 3 && e->ctx->params.viscous && g && g->built && g->les && g->les_serial == e->les_serial;
  pl.les_terms = pl.les && (e->les.sgs_model == 2 || e->les.sgs_model == 4);
  return pl;
}

bool simplex2d_folds_shock(const hfx_eles *e) { return simplex2d_runs(e) && simplex2d_plan(e).fold_shock; }

Simplex2dPartitionPlan simplex2d_partition_plan(const hfx_eles *e)
{
  Simplex2dPartitionPlan pp;
  const Simplex2dData *g = e->simplex2d.get();
  if (!g || !g->built) return pp;
  pp.partition_groups = g->n_partition_groups;
  pp.interior_groups = g->n_interior_groups;
  pp.gather_remote = simplex2d_plan(e).gather && g->remote_face != nullptr;
  return pp;
}

const double *simplex2d_fn_fpts(const hfx_eles *e) { return e->simplex2d ? e->simplex2d->fn_fpts.get() : nullptr; }

static S2dArgs s2d_args(hfx_eles *e, const Simplex2dPlan &pl, int in_step, S2dList list = S2dList::all)
{
  Simplex2dData *g = e->simplex2d.get();
  const hfx_params &p = e->ctx->params;
  S2dArgs a{};
  a.n_eles = e->n_eles; a.n_groups = (e->n_eles + pl.group - 1) / pl.group;
  if (list != S2dList::all)
  {
    a.groups = list == S2dList::partition ? g->partition_groups.get() : g->interior_groups.get();
    a.n_list = list == S2dList::partition ? g->n_partition_groups : g->n_interior_groups;
  }
  a.u0 = e->arr[HFX_DISU_UPTS0]; a.delta = e->arr[HFX_DELTA_DISU_FPTS]; a.disu = e->arr[HFX_DISU_FPTS];
  a.nbr = pl.gather ? g->nbr.get() : nullptr;
  if (g->remote_face)
  {
    a.in_disu = g->remote_face->in_disu;
    a.nfpi = g->remote_face->n_fpts_per_inter;
  }
  a.detjac_upts = e->detjac_upts; a.JGinv_upts = e->JGinv_upts; a.detjac_fpts = e->detjac_fpts; a.JGinv_fpts = e->JGinv_fpts;
  a.norm_fpts = e->norm_fpts; a.meta = g->meta;
  a.div = e->arr[HFX_DIV_TCONF_UPTS]; a.ntd = e->arr[HFX_NORM_TDISF_FPTS]; a.fn = g->fn_fpts;
  a.grad_fpts = (g->any_bdy && p.viscous) ? e->arr[HFX_GRAD_DISU_FPTS].get() : nullptr;
  a.P = e->ctx->phys();
  a.u0w = e->arr[HFX_DISU_UPTS0]; a.u1 = e->arr[HFX_DISU_UPTS1];
  a.tconf = e->arr[HFX_NORM_TCONF_FPTS];
  a.src = e->src_nonzero ? e->arr[HFX_SRC_UPTS].get() : nullptr;
  a.dt_local = e->arr[HFX_DT_LOCAL];
  a.disu_next = g->disu_alt;
  a.nan_flag = e->nan_flag;
  a.adv_type = p.adv_type; a.in_step = in_step; a.dt_local_on = p.dt_type == 2; a.dt = p.dt;
  a.rk_a = (p.adv_type >= 3) ? p.RK_a[in_step] : 0.0;
  a.rk_b = (p.adv_type >= 3) ? p.RK_b[in_step] : 0.0;
  // (low-storage schemes: a stage whose RK_a is 0.0 -- the first of a step -- takes 0.0 for the register instead of reading it)
  a.need_u1 = (p.adv_type >= 3 && a.rk_a != 0.0) || (p.adv_type == 1 && in_step == 3) || (p.adv_type == 2 && in_step == 2);
  a.write_div = 1; // the element kernel left the discontinuous part there: always complete it (the monitors read it)
  a.sens_field = e->shock_det_field == 0 ? 0 : e->n_dims + 1;
  a.s0 = e->s0;
  a.sensor = e->arr[HFX_SENSOR];
  if (pl.over_int)
  {
    a.oi_ops = g->overint_ops; a.JG_oi = e->JGinv_over_int_cubpts; a.n_cub = pl.n_cubpts;
    a.tdisf_in = e->arr[HFX_TDISF_UPTS];
  }
  if (pl.les)
  {
    a.les = e->les; a.les_len2 = g->les_len2; a.tdA_fpts = e->tdA_fpts;
  }
  return a;
}

// the instantiation of the plan's size class (s2d_class_row(I), I counting up; the quadrilateral classes: the plain kernels alone)
template <int I = 0>
static int launch_s2d(hfx_eles *e, S2dArgs a, const Simplex2dPlan &pl, bool element, bool shock = false)
{
  if constexpr (I == N_S2D_CLASSES)
  {
    HFX_CHECK(false, "2-D simplex fused stage: no kernel for this element size");
    return 1;
  }
  else
  {
    if (pl.size_class != I) return launch_s2d<I + 1>(e, a, pl, element, shock);
    constexpr int NU = s2d_class_row(I)[0], NFP = s2d_class_row(I)[1], G = s2d_class_row(I)[2];
    const size_t lds = element ? pl.element_lds : shock ? pl.update_shock_lds : pl.update_lds;
    HFX_CHECK(lds <= SIMPLEX2D_LDS_BUDGET, "2-D simplex fused stage: an LDS image of %zu bytes exceeds the budget of %zu", lds, SIMPLEX2D_LDS_BUDGET);
    a.ops = element ? e->simplex2d->element_ops : shock ? e->simplex2d->update_shock_ops : e->simplex2d->update_ops;
    HFX_CHECK(a.ops && (!shock || a.sensor), "2-D simplex fused stage: a table of the launch is missing");
    const bool oi = element && pl.over_int;
    HFX_CHECK(!oi || (pl.fold_over_int ? a.oi_ops && a.JG_oi && a.n_cub > 0 : a.tdisf_in != nullptr), "2-D simplex fused stage: a table of over-integration is missing");
    const bool les = element && pl.les;
    HFX_CHECK(!les || (!oi && a.les_len2 && a.tdA_fpts && (!pl.les_terms || (a.les.Lu && a.les.Le))), "2-D simplex fused stage: a table of the LES closure is missing");
    // as many workgroups as are resident (LDS; at most 8 of four waves), walking the groups grid-stride
    const long per_cu = std::max<long>(1, std::min<long>(8, (long)(160 * 1024 / lds)));
    const long work = a.groups ? a.n_list : a.n_groups; // the groups this launch walks
    const int grid = persistent_grid(e, element ? SLOT_ELEMENT : SLOT_UPDATE, work, std::min<long>(work, per_cu * e->ctx->n_cu));
    auto launch = [&](auto kernel) -> int {
      if (lds > 48 * 1024) HFX_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(S2D_T), lds, e->ctx->stream, a);
      HFX_HIP(hipGetLastError());
      return 0;
    };
    if constexpr (I >= N_SIMPLEX2D_SIZES)
    {
      HFX_CHECK(!oi && !les && !shock, "2-D simplex fused stage: quadrilaterals run the plain kernels only");
      return element ? launch(simplex2d_element_kernel_t<NU, NFP, G, S2dOverInt::none>) : launch(simplex2d_update_kernel_t<NU, NFP, G, false>);
    }
    else
    return oi      ? (pl.fold_over_int ? launch(simplex2d_element_kernel_t<NU, NFP, G, S2dOverInt::folded>)
                                       : launch(simplex2d_element_kernel_t<NU, NFP, G, S2dOverInt::unfolded>))
           : les     ? launch(simplex2d_element_kernel_t<NU, NFP, G, S2dOverInt::none, true>)
           : element ? launch(simplex2d_element_kernel_t<NU, NFP, G, S2dOverInt::none>)
           : shock ? launch(simplex2d_update_kernel_t<NU, NFP, G, true>)
                   : launch(simplex2d_update_kernel_t<NU, NFP, G, false>);
  }
}

// the pairs of an interior-face block: each side the arrays of its own element block, switch bit and normal the left block's
static FacePairArgs s2d_face_args(hfx_inters *f)
{
  auto side = [](hfx_eles *x) {
    FaceSide s{};
    s.plane = (long)x->n_fpts * x->n_eles;
    s.disu = x->arr[HFX_DISU_FPTS]; s.fn = x->simplex2d->fn_fpts; s.tdA = x->tdA_fpts;
    s.delta = x->arr[HFX_DELTA_DISU_FPTS]; s.tconf = x->arr[HFX_NORM_TCONF_FPTS];
    return s;
  };
  hfx_eles *x = f->left;
  FacePairArgs a{};
  a.npairs = (long)f->n_inters * f->n_fpts_per_inter;
  a.L = f->L; a.R = f->R; a.meta = x->simplex2d->meta; a.norm = x->norm_fpts;
  a.l = side(x); a.r = f->right == x ? a.l : side(f->right);
  return a;
}

static bool s2d_interior(const hfx_inters *f) { return !f->is_bdy && !f->is_mpi && (long)f->n_inters * f->n_fpts_per_inter > 0; }
static bool s2d_cross(const hfx_inters *f) { return f->left != f->right; }
// face_delta_kernel<2> writes the corrections of this interior-face block: a cross block always, a block inside one element block
// unless that block's element kernel gathers
static bool s2d_needs_delta(const hfx_inters *f) { return s2d_cross(f) || !simplex2d_plan(f->left).gather; }

int simplex2d_interior_ldg(hfx_eles *e, hfx_inters *const *faces, int nfb)
{
  hfx_ctx *ctx = e->ctx;
  if (!ctx->params.viscous) return 0;
  for (int b = 0; b < nfb; b++)
  {
    if (faces[b]->is_bdy && hfx_bdy_launch_internal(faces[b], 0, 1)) return 1; // ghost state -> inviscid common flux, LDG common solution
    if (!s2d_interior(faces[b]) || !s2d_needs_delta(faces[b])) continue; // (partition faces: the partitioned stage's one-sided kernels)
    const FacePairArgs a = s2d_face_args(faces[b]);
    hipLaunchKernelGGL(face_delta_kernel<2>, dim3((unsigned)((a.npairs + 255) / 256)), dim3(256), 0, ctx->stream, a, ctx->phys());
  }
  HFX_HIP(hipGetLastError());
  return 0;
}

// an empty list launches nothing (its device buffer does not exist, and a NULL list means ALL groups to the kernels)
static bool s2d_list_empty(const hfx_eles *e, S2dList list)
{
  const Simplex2dData *g = e->simplex2d.get();
  return (list == S2dList::partition && g->n_partition_groups == 0) || (list == S2dList::interior && g->n_interior_groups == 0);
}

int simplex2d_over_int_unfolded(hfx_eles *e)
{
  const Simplex2dPlan pl = simplex2d_plan(e);
  if (!pl.over_int || pl.fold_over_int) return 0;
  return hfx_eles_evaluate_invFlux_over_int(e);
}

int simplex2d_element_kernel(hfx_eles *e, int in_step, S2dList list)
{
  if (s2d_list_empty(e, list)) return 0;
  const Simplex2dPlan pl = simplex2d_plan(e);
  return launch_s2d(e, s2d_args(e, pl, in_step, list), pl, true);
}

int simplex2d_common_fluxes(hfx_eles *e, hfx_inters *const *faces, int nfb)
{
  hfx_ctx *ctx = e->ctx;
  const Phys P = ctx->phys();
  // (an inviscid run: the boundary faces' one sweep, which the viscous run launched before the element kernel)
  for (int b = 0; b < nfb; b++)
    if (faces[b]->is_bdy && hfx_bdy_launch_internal(faces[b], P.viscous ? 1 : 0, 1)) return 1;
  for (int b = 0; b < nfb; b++)
  {
    if (!s2d_interior(faces[b])) continue;
    const FacePairArgs a = s2d_face_args(faces[b]);
    const dim3 grid((unsigned)((a.npairs + 255) / 256));
    if (s2d_cross(faces[b])) // (each side its own block's arrays: the kernel's two-sided form)
      with_riemann_solver(P.riemann, [&](auto RS) {
        hipLaunchKernelGGL((face_flux2_kernel<2, decltype(RS)::value, FacePairArgs>), grid, dim3(256), 0, ctx->stream, a, P);
      });
    else
    {
      const FaceBlockArgs blk(a);
      with_riemann_solver(P.riemann, [&](auto RS) { hipLaunchKernelGGL((face_flux2_kernel<2, decltype(RS)::value>), grid, dim3(256), 0, ctx->stream, blk, P); });
    }
  }
  HFX_HIP(hipGetLastError());
  return 0;
}

int simplex2d_update_kernel(hfx_eles *e, int in_step, S2dList list, bool shock)
{
  if (s2d_list_empty(e, list)) return 0;
  const Simplex2dPlan pl = simplex2d_plan(e);
  const bool fold = shock && pl.fold_shock;
  if (launch_s2d(e, s2d_args(e, pl, in_step, list), pl, false, fold)) return 1;
  if (fold) e->stale &= ~(1u << HFX_SENSOR); // (both lists of a partitioned stage together write every element's)
  if (list == S2dList::all) simplex2d_swap_disu_fpts(e);
  return 0;
}

void simplex2d_swap_disu_fpts(hfx_eles *e) { std::swap(e->arr[HFX_DISU_FPTS], e->simplex2d->disu_alt); }

// ALGORITHMIC HBM bytes per launch of the four steps (doubles listed per element), priced from the plan
void simplex2d_kernel_bytes(const hfx_eles *e, double *bytes)
{
  const double nu = e->n_upts, nfp = e->n_fpts, nf = e->n_fields, nd = e->n_dims, ne = e->n_eles;
  const bool visc = e->ctx->params.viscous != 0;
  const Simplex2dPlan pl = simplex2d_plan(e);
  if (visc && !pl.gather) bytes[0] += ne * (8.0 * (2 * nfp * nf) + 4.0 * nfp + nfp * 0.5); // disu r, delta w, index + meta
  else if (visc && e->simplex2d) bytes[0] += (double)e->simplex2d->n_cross_pts * (8.0 * (2 * nf) + 4.0 + 0.5); // (the cross blocks' points alone)
  // u, metrics at the solution points r; div, norm_tdisf w
  bytes[1] += ne * 8.0 * (nu * nf + nu * nd * nd + nu * nf + nfp * nf);
  // viscous: delta (or the partner's disu and the own, and a partner word), detjac at both point sets, the flux points' metrics and normals r; Fn w
  if (visc) bytes[1] += ne * (8.0 * ((pl.gather ? 2 : 1) * nfp * nf + nu + nfp * (nd * nd + 1) + nfp * nd + nfp * nf) + (pl.gather ? 4.0 * nfp : 0.0));
  bytes[2] += ne * (8.0 * (nfp * nf + (visc ? nfp * nf : 0.0) + 0.5 * nfp * nd + nfp + nfp * nf) + 4.0 * nfp); // disu, Fn, normal(left), tdA r; tconf w
  bytes[3] += ne * 8.0 * (3 * nu * nf + nu + 2 * nfp * nf + 3 * nu * nf + nfp * nf);                          // u0,u1,div,detjac,tconf,ntd r; u0,u1,div,disu w
  if (pl.fold_shock) bytes[3] += ne * 8.0; // the folded shock filter: sensor w (the state it filters is the group's in LDS)
  // the LES form: len2 per solution point, tdA per flux point and, for the similarity models, Lu (3) and Le (2) per solution point r
  if (pl.les) bytes[1] += ne * (8.0 * nu + 8.0 * nfp + (pl.les_terms ? 40.0 * nu : 0.0));
  if (pl.fold_over_int) bytes[1] += ne * 8.0 * (nd * nd * pl.n_cubpts); // the folded over-integration: the cubature points' metrics r
  else if (pl.over_int)
  {
    // unfolded: the per-method kernels (u r, u_cub w | u_cub, metrics r, t_cub w | t_cub r, tdisf_upts w) in their own slot, and
    // the element kernel reads tdisf_upts
    const double nc = pl.n_cubpts;
    bytes[SLOT_OVER_INT] += ne * 8.0 * (nu * nf + nc * nf + nc * nf + nc * nd * nd + nc * nf * nd + nc * nf * nd + nu * nf * nd);
    bytes[1] += ne * 8.0 * (nu * nf * nd);
  }
}

Simplex2dStagePlan simplex2d_stage_plan(hfx_eles *const *eles, int neb)
{
  Simplex2dStagePlan sp;
  sp.blocks = neb;
  const bool visc = eles[0]->ctx->params.viscous != 0;
  int bdy = 0;
  for (const hfx_inters *f : eles[0]->simplex2d->built_with) // (every block's tables were made from the call's whole face list)
  {
    bdy += f->is_bdy && f->n_inters > 0;
    if (!s2d_interior(f)) continue;
    sp.interior_face_blocks++;
    sp.cross_face_blocks += s2d_cross(f);
    sp.delta_launches += visc && s2d_needs_delta(f);
  }
  // boundary sweeps: viscous runs one in front of the element kernels and one behind, inviscid runs the one behind
  sp.launches = (visc ? 2 : 1) * bdy + sp.delta_launches + neb + sp.interior_face_blocks + neb;
  return sp;
}

} // namespace hfx

extern "C" int hfx_simplex2d_stage_plan(hfx_eles *const *eles, int neb, int out[8])
{
  HFX_CHECK(eles && neb > 0 && eles[0] && out, "hfx_simplex2d_stage_plan: bad argument");
  HFX_IMMEDIATE(eles[0]->ctx, 0);
  for (int i = 0; i < neb; i++)
  {
    const hfx::Simplex2dData *g = eles[i] ? eles[i]->simplex2d.get() : nullptr;
    HFX_CHECK(g && g->built && hfx::simplex2d_runs(eles[i]), "hfx_simplex2d_stage_plan: no 2-D simplex fused stage has prepared block %d (run fused 4 first)", i);
    HFX_CHECK(g->built_blocks.size() == (size_t)neb && std::equal(g->built_blocks.begin(), g->built_blocks.end(), eles),
              "hfx_simplex2d_stage_plan: block %d was prepared in another call's list of blocks", i);
  }
  const hfx::Simplex2dStagePlan sp = hfx::simplex2d_stage_plan(eles, neb);
  const int v[8] = {sp.blocks, sp.interior_face_blocks, sp.cross_face_blocks, sp.delta_launches, sp.launches, 0, 0, 0};
  for (int i = 0; i < 8; i++) out[i] = v[i];
  return 0;
}

extern "C" int hfx_simplex2d_plan(hfx_eles *e, int out[8])
{
  HFX_CHECK(e && out, "hfx_simplex2d_plan: bad argument");
  HFX_IMMEDIATE(e->ctx, 0);
  HFX_CHECK(e->simplex2d && e->simplex2d->built, "hfx_simplex2d_plan: no 2-D simplex fused stage has prepared this block (run fused 4 first)");
  const hfx::Simplex2dPlan pl = hfx::simplex2d_plan(e);
  const int v[8] = {pl.size_class, pl.group, pl.waves, pl.gather, (int)pl.element_lds, (int)pl.update_lds, 0, 0};
  for (int i = 0; i < 8; i++) out[i] = v[i];
  return 0;
}

extern "C" int hfx_simplex2d_shock_plan(hfx_eles *e, int out[4])
{
  HFX_CHECK(e && out, "hfx_simplex2d_shock_plan: bad argument");
  HFX_IMMEDIATE(e->ctx, 0);
  HFX_CHECK(e->simplex2d && e->simplex2d->built, "hfx_simplex2d_shock_plan: no 2-D simplex fused stage has prepared this block (run fused 4 first)");
  const hfx::Simplex2dPlan pl = hfx::simplex2d_plan(e);
  out[0] = pl.fold_shock;
  out[1] = (int)(pl.fold_shock ? pl.update_shock_lds : pl.update_lds);
  out[2] = hfx::simplex2d_first_high_mode(e->n_upts);
  // behind a stage that does not fold a registered filter (general_shock_capture): two dense contractions, the sensor and the
  // selection kernel, and the extrapolation of the filtered state
  out[3] = (e->shock_ready && !pl.fold_shock) ? 5 : 0;
  return 0;
}

extern "C" int hfx_simplex2d_over_int_plan(hfx_eles *e, int out[8])
{
  HFX_CHECK(e && out, "hfx_simplex2d_over_int_plan: bad argument");
  HFX_IMMEDIATE(e->ctx, 0);
  HFX_CHECK(e->simplex2d && e->simplex2d->built, "hfx_simplex2d_over_int_plan: no 2-D simplex fused stage has prepared this block (run fused 4 first)");
  const hfx::Simplex2dPlan pl = hfx::simplex2d_plan(e);
  const int chunks = pl.over_int ? (pl.n_cubpts + pl.over_int_chunk - 1) / pl.over_int_chunk : 0;
  // in front of a stage that does not fold a registered over-integration (hfx_eles_evaluate_invFlux_over_int): the interpolation
  // to the cubature points, the flux there and the projection back
  const int v[8] = {pl.fold_over_int, pl.n_cubpts, pl.over_int ? pl.over_int_chunk : 0, chunks, (int)pl.element_lds,
                    (pl.over_int && !pl.fold_over_int) ? 3 : 0, 0, 0};
  for (int i = 0; i < 8; i++) out[i] = v[i];
  return 0;
}

extern "C" int hfx_simplex2d_les_plan(hfx_eles *e, int out[8])
{
  HFX_CHECK(e && out, "hfx_simplex2d_les_plan: bad argument");
  HFX_IMMEDIATE(e->ctx, 0);
  HFX_CHECK(e->simplex2d && e->simplex2d->built, "hfx_simplex2d_les_plan: no 2-D simplex fused stage has prepared this block (run fused 4 first)");
  const hfx::Simplex2dPlan pl = hfx::simplex2d_plan(e);
  // kernels in front of a step's FIRST stage of a closure that filters the solution (hfx_eles_calc_sgs_terms): the filter and the
  // products kernel; the similarity models: and the two contractions of the products and the Leonard kernel; SVV: and, behind the
  // copy of the filtered state, its extrapolation (ClosureFilter::filtering_refresh_svv)
  const int in_front = pl.sgs_model < 2 ? 0 : pl.sgs_model == 3 ? 3 : 5;
  const int v[8] = {pl.les, pl.sgs_model, pl.les_terms, in_front, (int)pl.element_lds, 0, 0, 0};
  for (int i = 0; i < 8; i++) out[i] = v[i];
  return 0;
}

extern "C" int hfx_simplex2d_partition_plan(hfx_eles *e, int out[4])
{
  HFX_CHECK(e && out, "hfx_simplex2d_partition_plan: bad argument");
  HFX_IMMEDIATE(e->ctx, 0);
  HFX_CHECK(e->simplex2d && e->simplex2d->built, "hfx_simplex2d_partition_plan: no 2-D simplex fused stage has prepared this block");
  const hfx::Simplex2dPartitionPlan pp = hfx::simplex2d_partition_plan(e);
  out[0] = pp.partition_groups; out[1] = pp.interior_groups; out[2] = pp.gather_remote; out[3] = 0;
  return 0;
}
