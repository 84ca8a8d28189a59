// general.hip -- the fused RK stage for GENERAL (non-tensor-product) element classes: tetrahedra, triangular prisms.
//
// Reference side: the same 17 calls of CalcResidual + AdvanceSolution as everywhere (src/solver.cpp:50-223,
// src/HiFiLES.cpp:201-217); on these classes the seven operators (src/eles.cpp:3074-3596, built by src/eles_tets.cpp and
// src/eles_pris.cpp) are DENSE -- P3: 40 x 20 / 20 x 20 / 20 x 40 doubles on tetrahedra, 68 x 40 / 40 x 40 / 40 x 68 on
// prisms -- so the per-method path is a stream of 15+ dense GEMM and point kernels per stage (820 B per DOF-update).
// Here the stage is cut at the two places where data must cross elements, exactly like the split stage of the
// tensor-product classes (fused_hex.hip, fused = 3), and is FOUR launches per element block and stage:
//
//   face_delta_kernel    thread per interior flux-point pair: LDG common solution -> delta_disu_fpts (both sides, which
//                        may belong to different element blocks: prism | tetrahedron faces)
//   general_flux_kernel  workgroup per batch of 16 elements: corrected gradient at the solution points
//                        (opp_4, opp_5), its extrapolation to the flux points (opp_6), both point physics blocks, the
//                        discontinuous divergence (opp_2) and normal flux (opp_1); leaves div_tdisf, norm_tdisf and
//                        each side's viscous flux projected on its own normal (Fn, 5 instead of 15 doubles per point)
//   gface_flux_multi_kernel  thread per pair, all face blocks in one launch: Riemann + LDG common flux from u and Fn of both sides -> norm_tconf
//   general_update_kernel  batch of 16 elements: opp_3 (norm_tconf - norm_tdisf), RK update, opp_0 of the new state
//
// Contractions run on the FP64 matrix cores (v_mfma_f64_16x16x4_f64).  A batch is 16 elements because 16 is the tile
// edge: the MFMA's "row" index is the ELEMENT of the batch, its "column" index an operator row, so one instruction
// applies 16 operator rows to 16 elements for 4 operator columns.  An accumulator register then holds 16 consecutive
// operator rows of one element: results go to HBM as 128-byte runs straight from the registers, and the flux-point
// physics is evaluated on the accumulators without a trip through LDS.  Operators are zero-padded on the host to
// (16 m') x (4 k') so that no tile needs a bounds check on its loads; they are the same ~100-300 kB for every workgroup
// and stay cache resident.  Element data sits in LDS as [operator column k][16 elements] planes (one per field /
// field x dimension) with the element index XOR-swizzled by the row: operand reads, accumulator writes and the
// point-wise passes are all bank-conflict free.
#include <algorithm>
#include <type_traits>

#include "general.hpp"
#include "step_loop.hpp"
#include "simplex2d.hpp"
#include "face_kernels.hpp" // the pairwise kernels (face_delta_kernel<3>, gface_flux_multi_kernel are instantiated here)

namespace hfx
{

typedef double g_f64x4 __attribute__((ext_vector_type(4)));

struct GeneralData
{
  int KU = 0, KF = 0, MU = 0, MF = 0; // n_upts / n_fpts padded to 4 (contraction length) and to 16 (output rows)
  // zero-padded operators, column-major with leading dimension M*: o4/o5/o2 (MU rows), o6/o1/o0 (MF rows), o3 (MU rows)
  DevBuf<double> o0, o1[3], o2[3], o3, o4[3], o5[3], o6;
  DevBuf<unsigned char> meta; // (n_fpts, n_eles): bit1 beta sign flipped (LEFT point of a pair), bit2 boundary point
  DevBuf<double> disu_alt;    // second disu_fpts buffer (the update kernel writes the new state's flux-point solution)
  DevBuf<double> fn_fpts;     // (n_fpts, n_eles, n_fields) viscous flux projected on the point's own normal
  DevBuf<int> nbr;            // (n_fpts, n_eles) partner word of every flux point whose pair lies inside this block (GenArgs::nbr)
  DevBuf<double> o2f[3];      // opp_2[d] - opp_3 opp_1[d], padded like o2: the folded correction (GenArgs::fold)
  hfx_eles *blocks[4] = {};   // the element blocks the partner words refer to (bits 3:2 of a word), captured at build
  int n_blocks = 0;
  bool any_bdy = false;
  bool built = false;
  DevBuf<long long> stamps;
  DevBuf<double> les_len2; // (n_upts, n_eles) squared length scale of an LES closure (les_len2_upload)
};

void general_invalidate(hfx_eles *e)
{
  if (e && e->general) e->general->built = false;
  simplex2d_invalidate(e);
}

void GeneralDelete::operator()(GeneralData *p) const { delete p; }

// LDS plane [row][16 elements], the element index swizzled by the row
__device__ __forceinline__ int sw(int row, int col) { return row * GB + (col ^ (row & 15)); }

// g_phys(d) = sum_l (inv_detjac * g_ref(l)) * JGinv(l,d)   (BLAS=NO branch of src/eles.cpp:1975-1979)
__device__ __forceinline__ void g_to_physical(const double inv_detjac, const double (&JG)[9], const double (&tg)[3], double (&cg)[3])
{
#pragma unroll
  for (int d = 0; d < 3; d++) cg[d] = 0.0;
#pragma unroll
  for (int l = 0; l < 3; l++)
  {
    const double temp = inv_detjac * tg[l];
#pragma unroll
    for (int d = 0; d < 3; d++) cg[d] += temp * JG[l + 3 * d];
  }
}

// NA output tiles at once, sharing the operator fragments: acc[j] += op[rt*16 + (0..15)][0 .. 4 ksteps) . plane_j[k][16 elements],
// plane_j = plane + j * pstride.  op: zero-padded operator, leading dimension M; lane: li = lane & 15, lk = lane >> 4.
// The operator fragments of UK k-steps are requested together (they come from L2 / L1: one latency per UK * NA MFMAs).
template <int NA>
__device__ __forceinline__ void tile_mac(g_f64x4 (&acc)[NA], const double *__restrict__ op, int M, int rt, const double *plane, int pstride,
                                         int ksteps, int li, int lk)
{
  constexpr int UK = (NA > 5) ? 2 : 8; // k-steps whose operator fragments are requested together (15 tiles: their LDS operands fill the registers)
  // sw(4 s + lk, li) = 64 s + 16 lk + ((li ^ lk) ^ 4 (s & 3)): four per-lane offsets, the rest is an immediate
  const int lx = li ^ lk;
  const int ob[4] = {16 * lk + lx, 16 * lk + (lx ^ 4), 16 * lk + (lx ^ 8), 16 * lk + (lx ^ 12)};
  const double *ap = op + rt * 16 + li + (long)M * lk;
  const long ast = (long)M * 4;
  double av[UK], an[UK];
#pragma unroll
  for (int u = 0; u < UK; u++) av[u] = (u < ksteps) ? ap[ast * u] : 0.0;
  for (int s0 = 0; s0 < ksteps; s0 += UK)
  {
    // the next chunk's fragments are in flight while this chunk's MFMAs issue
    const double *apn = ap + ast * (s0 + UK);
#pragma unroll
    for (int u = 0; u < UK; u++) an[u] = (s0 + UK + u < ksteps) ? apn[ast * u] : 0.0;
    const double *pb = plane + 64 * s0;
#pragma unroll
    for (int u = 0; u < UK; u++)
      if (s0 + u < ksteps)
      {
#pragma unroll
        for (int j = 0; j < NA; j++)
          acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(pb[j * pstride + 64 * u + ob[(UK % 4 == 0) ? (u & 3) : ((s0 + u) & 3)]], av[u], acc[j], 0, 0, 0);
      }
#pragma unroll
    for (int u = 0; u < UK; u++) av[u] = an[u];
  }
}

// n items of NF = 5 field tiles each over W waves: whole rounds item by item; the r = n % W items of the last round are
// cut into field groups so that W / r waves share one item (item(it, integral_constant<int, fields>, first field))
template <int W, class F>
__device__ __forceinline__ void split_rounds(int n, int wave, F &&item)
{
  const int whole = (n / W) * W, r = n - whole;
  for (int it = wave; it < whole; it += W) item(it, std::integral_constant<int, 5>{}, 0);
  if (r == 0) return;
  const int share = W / r; // waves per remaining item (>= 1)
  const int it = whole + wave / share, part = wave % share;
  if (it >= n) return; // (W not a multiple of r: the last few waves have nothing)
  if (share == 1)
    item(it, std::integral_constant<int, 5>{}, 0);
  else if (share == 2)
  {
    if (part == 0) item(it, std::integral_constant<int, 3>{}, 0);
    else item(it, std::integral_constant<int, 2>{}, 3);
  }
  else if (share == 3)
  {
    if (part == 0) item(it, std::integral_constant<int, 2>{}, 0);
    else if (part == 1) item(it, std::integral_constant<int, 2>{}, 2);
    else item(it, std::integral_constant<int, 1>{}, 4);
  }
  else if (share == 4)
  {
    if (part == 0) item(it, std::integral_constant<int, 2>{}, 0);
    else item(it, std::integral_constant<int, 1>{}, part + 1);
  }
  else if (part < 5)
    item(it, std::integral_constant<int, 1>{}, part);
}

// ---------------------------------------------------------------------------------------------------------------
// flux kernel: u, delta -> div_tdisf, norm_tdisf, Fn   (steps 3-4, 8 (both halves), 10-12 of CalcResidual's sequence)
// ---------------------------------------------------------------------------------------------------------------
// NUc, NFPc: the element class's point counts as compile-time constants (0: read from the arguments); the common sizes
// are instantiated so that trip counts, LDS offsets and the index divisions fold
// LESG: the eddy-viscosity / similarity closure of an LES run (eles::calc_sgsf_upts, src/eles.cpp:2395-2650) evaluated in P3 on the
// physical gradient the point physics holds.  The reference adds F_sgs to the total flux at the solution points
// (src/eles.cpp:2360-2392) and, at the flux points, extrapolates the TRANSFORMED SGS flux (opp_0), takes it back to physical space
// and adds it to each side's viscous flux in the common-flux sweep (src/eles.cpp:2817-2893, src/int_inters.cpp:299-313).  What the
// face kernel needs of that is F_sgs . n = (F~_sgs . n~) / tdA = (sum_d opp_1[d] F~_sgs,d) / tdA -- the contraction P4 runs for
// norm_tdisf in the form without the folded correction.  So P3 first leaves the transformed SGS flux ALONE in G (the rest of the
// point's transformed flux waits in registers), one more contraction adds its normal projection to the Fn this workgroup stored
// in P2, and then the rest joins G for P4.
template <int W, int NUc, int NFPc, bool LESG = false>
__global__ __launch_bounds__(64 * W, 2) void general_flux_kernel(const GenArgs a)
{
  static_assert(!LESG || NUc != 0, "the LES form is instantiated for the element classes with compile-time sizes");
  constexpr int NF = 5, ND = 3, T = 64 * W;
  extern __shared__ double lds[];
  const int nu = NUc ? NUc : a.nu, nfp = NFPc ? NFPc : a.nfp;
  const int KU = (nu + 3) & ~3, KF = (nfp + 3) & ~3, MU = (nu + 15) & ~15, MF = (nfp + 15) & ~15;
  const unsigned inv_nu = NUc ? (unsigned)(4294967296ull / (unsigned)(NUc ? NUc : 1)) + 1u : a.inv_nu;
  const unsigned inv_nfp = NFPc ? (unsigned)(4294967296ull / (unsigned)(NFPc ? NFPc : 1)) + 1u : a.inv_nfp;
  double *U = lds;                 // [NF][KU][16]      the state; later: nothing
  double *D = U + NF * KU * GB;    // [NF][KF][16]      delta_disu_fpts
  double *G = D + NF * KF * GB;    // [NF*ND][KU][16]   reference-space gradient, then the transformed total flux
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const long e0 = (long)blockIdx.x * GB;
  const int nval = (int)min((long)GB, a.n_eles - e0);
  const long plane_u = (long)nu * a.n_eles, plane_f = (long)nfp * a.n_eles;
  const bool visc = a.P.viscous != 0;
  auto stamp = [&](int slot) {
    if (a.stamps != nullptr && blockIdx.x == gridDim.x / 2 && lane == 0) a.stamps[wave * 16 + slot] = clock64();
  };
  stamp(0);

  // ---- P0: stage the state (and delta) of the batch: contiguous nu x 16 doubles per field in HBM -> [k][element].
  // ALL loads of a thread are requested before the first one is used (one memory latency for the batch instead of one per
  // trip of the staging loop: the stamps showed 21 000 - 48 000 of a batch's 100 000 cycles here)
  {
    constexpr int MAXQ_U = general_staged((NUc + 3) & ~3, W), MAXQ_D = general_staged((NFPc + 3) & ~3, W);
    if constexpr (NUc != 0 && NFPc != 0 && general_flux_batched(NUc, NFPc, W)) // (more would not fit the registers)
    {
      double ru[NF][MAXQ_U], rd[NF][MAXQ_D];
#pragma unroll
      for (int f = 0; f < NF; f++)
      {
        const double *src = a.u0 + e0 * nu + f * plane_u;
#pragma unroll
        for (int i = 0; i < MAXQ_U; i++)
        {
          const int q = tid + T * i;
          const int el = (int)__umulhi((unsigned)q, inv_nu);
          ru[f][i] = (q < nu * GB && el < nval) ? src[q] : 0.0;
        }
        if (visc && a.nbr == nullptr)
        {
          const double *sd = a.delta + e0 * nfp + f * plane_f;
#pragma unroll
          for (int i = 0; i < MAXQ_D; i++)
          {
            const int q = tid + T * i;
            const int el = (int)__umulhi((unsigned)q, inv_nfp);
            rd[f][i] = (q < nfp * GB && el < nval) ? sd[q] : 0.0;
          }
        }
      }
      if (visc && a.nbr != nullptr)
      {
        // LDG corrections formed here (the pairwise kernel is not launched for pairs inside this block): the point's partner
        // word, then its own and its partner's flux-point solution -- or the correction itself where the word is -1 --
        // delta = u_common - u_own, u_common = (u_L + u_R)/2 - beta (u_L - u_R) on the pair's orientation (src/inters.cpp:637)
        int w[MAXQ_D];
        bool okq[MAXQ_D];
#pragma unroll
        for (int i = 0; i < MAXQ_D; i++)
        {
          const int q = tid + T * i;
          const int el = (int)__umulhi((unsigned)q, inv_nfp);
          okq[i] = q < nfp * GB && el < nval;
          w[i] = okq[i] ? a.nbr[e0 * nfp + q] : -1;
        }
        double ro[NF][MAXQ_D];
#pragma unroll
        for (int i = 0; i < MAXQ_D; i++)
        {
          const long own = e0 * nfp + (okq[i] ? tid + T * i : 0);
          const int blk = (w[i] >> 2) & 3;
          const double *po = a.disu + own, *pp = (w[i] < 0) ? a.delta + own : a.disu_b[blk] + (w[i] >> 4);
          const long pstr = (w[i] < 0) ? plane_f : a.plane_b[blk];
#pragma unroll
          for (int f = 0; f < NF; f++)
          {
            ro[f][i] = po[f * plane_f];
            rd[f][i] = pp[f * pstr];
          }
        }
#pragma unroll
        for (int i = 0; i < MAXQ_D; i++)
        {
          const double beta = ldg_beta(w[i], a.P);
#pragma unroll
          for (int f = 0; f < NF; f++)
          {
            const double ul = (w[i] & 1) ? rd[f][i] : ro[f][i], ur = (w[i] & 1) ? ro[f][i] : rd[f][i];
            const double uc = 0.5 * (ul + ur) - beta * (ul - ur);
            rd[f][i] = !okq[i] ? 0.0 : ((w[i] < 0) ? rd[f][i] : uc - ro[f][i]);
          }
        }
      }
#pragma unroll
      for (int f = 0; f < NF; f++)
      {
#pragma unroll
        for (int i = 0; i < MAXQ_U; i++)
        {
          const int q = tid + T * i;
          if (q < KU * GB)
          {
            const int el = (int)__umulhi((unsigned)q, inv_nu), k = q - el * nu;
            const int p = q - nu * GB; // >= 0: one of the (KU - nu) * 16 padding entries
            U[f * KU * GB + ((q < nu * GB) ? sw(k, el) : sw(nu + p / GB, p % GB))] = ru[f][i];
          }
        }
        if (visc)
        {
#pragma unroll
          for (int i = 0; i < MAXQ_D; i++)
          {
            const int q = tid + T * i;
            if (q < KF * GB)
            {
              const int el = (int)__umulhi((unsigned)q, inv_nfp), k = q - el * nfp;
              const int p = q - nfp * GB;
              D[f * KF * GB + ((q < nfp * GB) ? sw(k, el) : sw(nfp + p / GB, p % GB))] = rd[f][i];
            }
          }
        }
      }
    }
    else
    {
      for (int f = 0; f < NF; f++)
      {
        const double *src = a.u0 + e0 * nu + f * plane_u;
        for (int q = tid; q < KU * GB; q += T)
        {
          const int el = (int)__umulhi((unsigned)q, inv_nu), k = q - el * nu; // q < nu*16: a real entry; the rest of the plane: K padding
          if (q < nu * GB)
            U[f * KU * GB + sw(k, el)] = (el < nval) ? src[q] : 0.0;
          else
          {
            const int p = q - nu * GB; // (KU - nu) * 16 padding entries
            U[f * KU * GB + sw(nu + p / GB, p % GB)] = 0.0;
          }
        }
        if (visc)
        {
          const double *sd = a.delta + e0 * nfp + f * plane_f;
          for (int q = tid; q < KF * GB; q += T)
          {
            const int el = (int)__umulhi((unsigned)q, inv_nfp), k = q - el * nfp;
            if (q < nfp * GB)
              D[f * KF * GB + sw(k, el)] = (el < nval) ? sd[q] : 0.0;
            else
            {
              const int p = q - nfp * GB;
              D[f * KF * GB + sw(nfp + p / GB, p % GB)] = 0.0;
            }
          }
        }
      }
    }
  }
  // K padding rows of G (read as zero by the opp_6 / opp_1 / opp_2 tiles)
  const int pad_rows = (KU - nu) * GB, pad_div = pad_rows > 0 ? pad_rows : 1; // (no padding rows where n_upts is a multiple of 4)
  for (int q = tid; q < NF * ND * pad_rows; q += T)
  {
    const int c = q / pad_div, p = q - c * pad_rows;
    G[c * KU * GB + sw(nu + p / GB, p % GB)] = 0.0;
  }
  stamp(1);
  __syncthreads();
  stamp(2);

  // ---- P3: point physics at the solution points (evaluate_invFlux, the transform of correct_gradient, evaluate_viscFlux;
  //          src/eles.cpp:1415,1973,2285): G(f,d) <- transformed total flux.  Points first, first + stride, ...
  auto p3_points = [&](int first, int stride) {
  // the point's metrics are requested one trip ahead (a trip is one memory latency otherwise: 7 000 cycles measured)
  double JGn[9], djn = 1.0;
  auto request_metrics = [&](int q) {
    const int el = (int)__umulhi((unsigned)q, inv_nu), pt = q - el * nu;
    const bool ok = q < nu * GB && el < nval;
    const long o = ok ? pt + (long)nu * (e0 + el) : 0;
#pragma unroll
    for (int c = 0; c < 9; c++) JGn[c] = ok ? a.JGinv_upts[o * 9 + c] : 0.0;
    djn = (ok && visc) ? a.detjac_upts[o] : 1.0;
  };
  request_metrics(first);
  for (int q = first; q < nu * GB; q += stride)
  {
    const int el = (int)__umulhi((unsigned)q, inv_nu), pt = q - el * nu;
    double JG[9];
#pragma unroll
    for (int c = 0; c < 9; c++) JG[c] = JGn[c];
    const double dj = djn;
    request_metrics(q + stride);
    if (el < nval)
    {
      const int so = sw(pt, el);
      double u[NF], F[NF * ND];
#pragma unroll
      for (int k = 0; k < NF; k++) u[k] = U[k * KU * GB + so];
      const bool oi = a.tdisf_in != nullptr;
      double td[NF * ND];
      if (oi)
      {
        const long o = pt + (long)nu * (e0 + el);
#pragma unroll
        for (int c = 0; c < NF * ND; c++)
        {
          td[c] = a.tdisf_in[o + c * plane_u];
          F[c] = 0.0;
        }
      }
      else
      {
#pragma unroll
        for (int c = 0; c < NF * ND; c++) td[c] = 0.0;
        calc_invf<ND, true>(a.P.gamma, u, F);
      }
      if (visc)
      {
        const double idj = 1.0 / dj;
        double g[NF * ND], fv[NF * ND];
#pragma unroll
        for (int k = 0; k < NF; k++)
        {
          double tg[ND], cg[ND];
#pragma unroll
          for (int d = 0; d < ND; d++) tg[d] = G[(k + NF * d) * KU * GB + so];
          g_to_physical(idj, JG, tg, cg);
#pragma unroll
          for (int d = 0; d < ND; d++) g[k + NF * d] = cg[d];
        }
        calc_visf<ND, true>(a.P, u, g, fv);
#pragma unroll
        for (int c = 0; c < NF * ND; c++) F[c] += fv[c];
      }
#pragma unroll
      for (int k = 0; k < NF; k++)
#pragma unroll
        for (int l = 0; l < ND; l++)
        {
          double t = td[k + NF * l];
#pragma unroll
          for (int m = 0; m < ND; m++) t += JG[l + ND * m] * F[k + NF * m];
          G[(k + NF * l) * KU * GB + so] = t;
        }
    }
    else
    {
      const int pt2 = q - el * nu, so = sw(pt2, el);
#pragma unroll
      for (int c = 0; c < NF * ND; c++) G[c * KU * GB + so] = 0.0;
    }
  }
  };

  if (visc)
  {
    // ---- P1: reference-space corrected gradient at the solution points (calculate_gradient + first half of
    //          correct_gradient, src/eles.cpp:1823,1900): G(f,d) = opp_4[d] U(f) + opp_5[d] D(f)
    const int n_rt = MU / 16;
    // one item = (row tile, dimension): NF output tiles that share the operator fragments.  Whole rounds of W items; the
    // items of the last, partial round are split by FIELD among the waves (W / r waves per item), so that no wave sits
    // idle while another does a whole second item
    auto p1_item = [&](int it, auto nf_c, int f0) {
      constexpr int NFS = decltype(nf_c)::value;
      const int d = it % ND, rt = it / ND;
      g_f64x4 acc[NFS];
#pragma unroll
      for (int f = 0; f < NFS; f++) acc[f] = g_f64x4{0.0, 0.0, 0.0, 0.0};
      tile_mac<NFS>(acc, a.o4[d], MU, rt, U + f0 * KU * GB, KU * GB, KU / 4, li, lk);
      tile_mac<NFS>(acc, a.o5[d], MU, rt, D + f0 * KF * GB, KF * GB, KF / 4, li, lk);
      const int row = rt * 16 + li;
      if (row < nu)
#pragma unroll
        for (int f = 0; f < NFS; f++)
#pragma unroll
          for (int rg = 0; rg < 4; rg++) G[(f0 + f + NF * d) * KU * GB + sw(row, lk + 4 * rg)] = acc[f][rg];
    };
    split_rounds<W>(n_rt * ND, wave, p1_item);
    stamp(3);
    __syncthreads();
    stamp(4);

    // ---- P2: gradient at the flux points (second half of correct_gradient: opp_6, then the transform with the flux
    //          points' own metrics, src/eles.cpp:1930,1998) and the viscous flux there, projected on the point's normal
    const int n_ft = MF / 16;
    for (int rt = wave; rt < n_ft; rt += W)
    {
      g_f64x4 acc[NF * ND];
#pragma unroll
      for (int c = 0; c < NF * ND; c++) acc[c] = g_f64x4{0.0, 0.0, 0.0, 0.0};
      // the point inputs of (row, element lk + 4 rg) are requested one point ahead: rg = 0 before the MFMA loop
      const int row = rt * 16 + li;
      double pu[2][NF], pJ[2][9], pd[2], pn[2][ND];
      unsigned char pm[2] = {0, 0}; // the point's flag byte (bit2: boundary point), with the other inputs
      auto request = [&](int slot, int rg) {
        const int el = lk + 4 * rg;
        const bool ok = row < nfp && el < nval;
        // a lane without a point reads point 0 of the block (its values are not used): UNCONDITIONAL loads -- behind a
        // predicate every pass waited for the loads it had just issued for the next one (s_waitcnt vmcnt(0) at the join)
        const long o = ok ? row + (long)nfp * (e0 + el) : 0;
#pragma unroll
        for (int k = 0; k < NF; k++) pu[slot][k] = a.disu[o + k * plane_f];
#pragma unroll
        for (int q = 0; q < 9; q++) pJ[slot][q] = a.JGinv_fpts[o * 9 + q];
        pd[slot] = a.detjac_fpts[o];
#pragma unroll
        for (int m = 0; m < ND; m++) pn[slot][m] = a.norm_fpts[o + m * plane_f];
        if (a.grad_fpts != nullptr) pm[slot] = a.meta[o];
      };
      request(0, 0);
      tile_mac<NF * ND>(acc, a.o6, MF, rt, G, KU * GB, KU / 4, li, lk);
#pragma unroll
      for (int rg = 0; rg < 4; rg++)
      {
        const int el = lk + 4 * rg, sl = rg & 1;
        if (rg < 3) request(sl ^ 1, rg + 1);
        if (row < nfp && el < nval)
        {
          const long o = row + (long)nfp * (e0 + el);
          double g[NF * ND], fv[NF * ND];
          const double idj = 1.0 / pd[sl];
#pragma unroll
          for (int k = 0; k < NF; k++)
          {
            double tg[ND], cg[ND];
#pragma unroll
            for (int d = 0; d < ND; d++) tg[d] = acc[k + NF * d][rg];
            g_to_physical(idj, pJ[sl], tg, cg);
#pragma unroll
            for (int d = 0; d < ND; d++) g[k + NF * d] = cg[d];
          }
          if (a.grad_fpts != nullptr && (pm[sl] & 4)) // boundary point: the boundary kernel reads the gradient
#pragma unroll
            for (int c = 0; c < NF * ND; c++) a.grad_fpts[o + c * plane_f] = g[c];
          calc_visf<ND, true>(a.P, pu[sl], g, fv);
#pragma unroll
          for (int k = 0; k < NF; k++)
          {
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < ND; m++) s += fv[k + NF * m] * pn[sl][m];
            a.fn[o + k * plane_f] = s;
          }
        }
      }
    }
    stamp(5);
    __syncthreads();
    stamp(6);
  }

  if constexpr (LESG)
  {
    constexpr int TRIPS = (NUc * GB + T - 1) / T;
    double Tiv[TRIPS][NF * ND]; // transformed inviscid + viscous flux of this thread's points
#pragma unroll
    for (int tr = 0; tr < TRIPS; tr++)
    {
      const int q = tid + T * tr;
      const int el = (int)__umulhi((unsigned)q, inv_nu), pt = q - el * nu;
      const bool in = q < nu * GB, ok = in && el < nval;
      const long o = ok ? pt + (long)nu * (e0 + el) : 0;
      double JG[9];
#pragma unroll
      for (int c = 0; c < 9; c++) JG[c] = a.JGinv_upts[o * 9 + c];
      const double dj = a.detjac_upts[o], len2 = a.les_len2[o];
      const int so = sw(in ? pt : 0, in ? el : 0);
      double u[NF], F[NF * ND], g[NF * ND], fv[NF * ND], sg[NF * ND];
#pragma unroll
      for (int k = 0; k < NF; k++) u[k] = ok ? U[k * KU * GB + so] : 1.0;
      calc_invf<ND, true>(a.P.gamma, u, F);
      const double idj = 1.0 / dj;
#pragma unroll
      for (int k = 0; k < NF; k++)
      {
        double tg[ND], cg[ND];
#pragma unroll
        for (int d = 0; d < ND; d++) tg[d] = G[(k + NF * d) * KU * GB + so];
        g_to_physical(idj, JG, tg, cg);
#pragma unroll
        for (int d = 0; d < ND; d++) g[k + NF * d] = ok ? cg[d] : 0.0;
      }
      calc_visf<ND, true>(a.P, u, g, fv);
      calc_sgsf_fast<ND>(a.P, a.les, u, g, len2, o, plane_u, sg);
#pragma unroll
      for (int k = 0; k < NF; k++)
#pragma unroll
        for (int l = 0; l < ND; l++)
        {
          double t = 0.0, ts = 0.0;
#pragma unroll
          for (int m = 0; m < ND; m++)
          {
            t += JG[l + ND * m] * (F[k + NF * m] + fv[k + NF * m]);
            ts += JG[l + ND * m] * sg[k + NF * m];
          }
          Tiv[tr][k + NF * l] = ok ? t : 0.0;
          if (in) G[(k + NF * l) * KU * GB + so] = ok ? ts : 0.0;
        }
    }
    __syncthreads();
    // F~_sgs . n~ at the flux points, joined to the Fn of P2: rows of opp_1[d] against G(., d), as P4's norm_tdisf tiles
    {
      const int n_ft = MF / 16;
      auto sgs_item = [&](int rt, auto nf_c, int f0) {
        constexpr int NFS = decltype(nf_c)::value;
        g_f64x4 acc[NFS];
#pragma unroll
        for (int f = 0; f < NFS; f++) acc[f] = g_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int d = 0; d < ND; d++) tile_mac<NFS>(acc, a.o1[d], MF, rt, G + (f0 + NF * d) * KU * GB, KU * GB, KU / 4, li, lk);
        const int row = rt * 16 + li;
        if (row < nfp)
#pragma unroll
          for (int rg = 0; rg < 4; rg++)
          {
            const int el = lk + 4 * rg;
            if (el < nval)
            {
              const long o = row + (long)nfp * (e0 + el);
              const double itd = 1.0 / a.tdA_fpts[o];
#pragma unroll
              for (int f = 0; f < NFS; f++)
              {
                // (the value another wave of this workgroup stored in P2: read past the first-level cache)
                double *p = a.fn + o + (f0 + f) * plane_f;
                const double old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                *p = old + acc[f][rg] * itd;
              }
            }
          }
      };
      split_rounds<W>(n_ft, wave, sgs_item);
    }
    __syncthreads();
#pragma unroll
    for (int tr = 0; tr < TRIPS; tr++)
    {
      const int q = tid + T * tr;
      const int el = (int)__umulhi((unsigned)q, inv_nu), pt = q - el * nu;
      if (q < nu * GB)
      {
        const int so = sw(pt, el);
#pragma unroll
        for (int c = 0; c < NF * ND; c++) G[c * KU * GB + so] += Tiv[tr][c];
      }
    }
  }
  else
    p3_points(tid, T);
  stamp(7);
  __syncthreads();
  stamp(8);

  // ---- P4: discontinuous divergence (opp_2) and normal flux at the flux points (opp_1), summed over the dimensions
  //          (calculate_divergence, extrapolate_totalFlux; src/eles.cpp:1651,1549) -> HBM, 128-byte runs
  {
    const int n_ut = MU / 16, n_ft = MF / 16;
    auto p4_item = [&](int t, auto nf_c, int f0) {
      constexpr int NFS = decltype(nf_c)::value;
      const bool is_div = t < n_ut;
      const int rt = is_div ? t : t - n_ut;
      g_f64x4 acc[NFS];
#pragma unroll
      for (int f = 0; f < NFS; f++) acc[f] = g_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int d = 0; d < ND; d++)
        tile_mac<NFS>(acc, is_div ? a.o2[d] : a.o1[d], is_div ? MU : MF, rt, G + (f0 + NF * d) * KU * GB, KU * GB, KU / 4, li, lk);
      const int row = rt * 16 + li, n = is_div ? nu : nfp;
      double *out = is_div ? a.div : a.ntd;
      const long plane = is_div ? plane_u : plane_f;
      if (row < n)
#pragma unroll
        for (int f = 0; f < NFS; f++)
#pragma unroll
          for (int rg = 0; rg < 4; rg++)
          {
            const int el = lk + 4 * rg;
            if (el < nval) out[row + (long)n * (e0 + el) + (f0 + f) * plane] = acc[f][rg];
          }
    };
    split_rounds<W>(a.fold ? n_ut : n_ut + n_ft, wave, p4_item); // (folded: the divergence tiles only)
  }
  stamp(9);
}

// ---------------------------------------------------------------------------------------------------------------
// update kernel: div_tdisf + opp_3 (norm_tconf - norm_tdisf) -> RK update -> disu_fpts of the new state
// (calculate_corrected_divergence, AdvanceSolution, extrapolate_solution; src/eles.cpp:1738,1080,1360)
// ---------------------------------------------------------------------------------------------------------------
template <int W, int NUc, int NFPc>
__global__ __launch_bounds__(64 * W) void general_update_kernel(const GenArgs a)
{
  constexpr int NF = 5, T = 64 * W;
  extern __shared__ double lds[];
  const int nu = NUc ? NUc : a.nu, nfp = NFPc ? NFPc : a.nfp;
  const int KU = (nu + 3) & ~3, KF = (nfp + 3) & ~3, MU = (nu + 15) & ~15, MF = (nfp + 15) & ~15;
  const unsigned inv_nu = NUc ? (unsigned)(4294967296ull / (unsigned)(NUc ? NUc : 1)) + 1u : a.inv_nu;
  const unsigned inv_nfp = NFPc ? (unsigned)(4294967296ull / (unsigned)(NFPc ? NFPc : 1)) + 1u : a.inv_nfp;
  double *X = lds;               // [NF][KF][16]  norm_tconf - norm_tdisf
  double *S = X + NF * KF * GB;  // [NF][KU][16]  the correction, then the new state
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const long e0 = (long)blockIdx.x * GB;
  const int nval = (int)min((long)GB, a.n_eles - e0);
  const long plane_u = (long)nu * a.n_eles, plane_f = (long)nfp * a.n_eles;

  // every load of a thread is requested before the first one is used (one memory latency per staging step, as in the
  // flux kernel's P0)
  constexpr int MAXQ_D = general_staged((NFPc + 3) & ~3, W), MAXQ_U = general_staged(NUc, W);
  constexpr bool BATCH = NUc != 0 && NFPc != 0 && general_update_batched(NUc, NFPc, W);
  if constexpr (BATCH)
  {
    double rt_[NF][MAXQ_D], rn_[NF][MAXQ_D];
#pragma unroll
    for (int f = 0; f < NF; f++)
    {
      const double *tc = a.tconf + e0 * nfp + f * plane_f, *nt = a.ntd + e0 * nfp + f * plane_f;
#pragma unroll
      for (int i = 0; i < MAXQ_D; i++)
      {
        const int q = tid + T * i;
        const int el = (int)__umulhi((unsigned)q, inv_nfp);
        const bool ok = q < nfp * GB && el < nval;
        rt_[f][i] = ok ? tc[q] : 0.0;
        rn_[f][i] = (ok && !a.fold) ? nt[q] : 0.0;
      }
    }
#pragma unroll
    for (int f = 0; f < NF; f++)
    {
#pragma unroll
      for (int i = 0; i < MAXQ_D; i++)
      {
        const int q = tid + T * i;
        if (q < KF * GB)
        {
          const int el = (int)__umulhi((unsigned)q, inv_nfp), k = q - el * nfp;
          const int p = q - nfp * GB;
          X[f * KF * GB + ((q < nfp * GB) ? sw(k, el) : sw(nfp + p / GB, p % GB))] = rt_[f][i] + -1.0 * rn_[f][i]; // the daxpy of src/eles.cpp:1746
        }
      }
      for (int q = tid; q < (KU - nu) * GB; q += T) S[f * KU * GB + sw(nu + q / GB, q % GB)] = 0.0;
    }
  }
  else
  {
  for (int f = 0; f < NF; f++)
  {
    const double *tc = a.tconf + e0 * nfp + f * plane_f, *nt = a.ntd + e0 * nfp + f * plane_f;
    for (int q = tid; q < KF * GB; q += T)
    {
      const int el = (int)__umulhi((unsigned)q, inv_nfp), k = q - el * nfp;
      if (q < nfp * GB)
        X[f * KF * GB + sw(k, el)] = (el < nval) ? (a.fold ? tc[q] : tc[q] + -1.0 * nt[q]) : 0.0; // the daxpy of src/eles.cpp:1746
      else
      {
        const int p = q - nfp * GB;
        X[f * KF * GB + sw(nfp + p / GB, p % GB)] = 0.0;
      }
    }
    for (int q = tid; q < (KU - nu) * GB; q += T) S[f * KU * GB + sw(nu + q / GB, q % GB)] = 0.0;
  }
  }
  __syncthreads();
  {
    const int n_rt = MU / 16;
    for (int rt = wave; rt < n_rt; rt += W)
    {
      g_f64x4 acc[NF];
#pragma unroll
      for (int f = 0; f < NF; f++) acc[f] = g_f64x4{0.0, 0.0, 0.0, 0.0};
      tile_mac<NF>(acc, a.o3, MU, rt, X, KF * GB, KF / 4, li, lk);
      const int row = rt * 16 + li;
      if (row < nu)
#pragma unroll
        for (int f = 0; f < NF; f++)
#pragma unroll
          for (int rg = 0; rg < 4; rg++) S[f * KU * GB + sw(row, lk + 4 * rg)] = acc[f][rg];
    }
  }
  // the update's inputs, requested before the barrier that ends the opp_3 tiles (BATCH: all of them at once)
  double pdv[BATCH ? NF : 1][BATCH ? MAXQ_U : 1], pu0[BATCH ? NF : 1][BATCH ? MAXQ_U : 1], pu1[BATCH ? NF : 1][BATCH ? MAXQ_U : 1],
      pdj[BATCH ? MAXQ_U : 1];
  if constexpr (BATCH)
  {
#pragma unroll
    for (int i = 0; i < MAXQ_U; i++)
    {
      const int q = tid + T * i;
      const int el = (int)__umulhi((unsigned)q, inv_nu);
      const bool okq = q < nu * GB && el < nval;
      const long p = e0 * nu + q;
      pdj[i] = okq ? a.detjac_upts[p] : 1.0;
#pragma unroll
      for (int f = 0; f < NF; f++)
      {
        const long ok = p + f * plane_u;
        pdv[f][i] = okq ? a.div_in[ok] : 0.0;
        pu0[f][i] = okq ? a.u0w[ok] : 0.0;
        pu1[f][i] = (okq && a.need_u1) ? a.u1[ok] : 0.0;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int f = 0; f < NF; f++)
  {
#pragma unroll
    for (int i = 0; i < (BATCH ? MAXQ_U : 1); i++)
    for (int q = BATCH ? tid + T * i : tid; q < nu * GB; q += BATCH ? (1 << 30) : T)
    {
      const int el = (int)__umulhi((unsigned)q, inv_nu), pt = q - el * nu;
      const int so = f * KU * GB + sw(pt, el);
      if (el >= nval)
      {
        S[so] = 0.0;
        continue;
      }
      const long p = e0 * nu + q, ok = p + f * plane_u;
      const double dv = (BATCH ? pdv[f][i] : a.div_in[ok]) + S[so];
      if (dv != dv) atomicMin(a.nan_flag, (unsigned long long)ok);
      if (a.write_div) a.div[ok] = dv;
      const double s = a.src ? a.src[ok] : 0.0;
      const double dt = a.dt_local_on ? a.dt_local[e0 + el] : a.dt;
      const double dd = dv / (BATCH ? pdj[i] : a.detjac_upts[p]);
      double un = BATCH ? pu0[f][i] : a.u0w[ok];
      const double u1v = BATCH ? pu1[f][i] : (a.need_u1 ? a.u1[ok] : 0.0);
      if (a.adv_type == 0)
        un -= dt * (dd - s);
      else if (a.adv_type == 1)
      {
        if (a.in_step == 0) a.u1[ok] = un;
        if (a.in_step < 3)
          un -= dt / 3.0 * (dd - s);
        else
        {
          const double rhs = -dd + s;
          un = 3.0 / 4.0 * un + 1.0 / 4.0 * u1v + dt / 4.0 * rhs;
        }
      }
      else if (a.adv_type == 2)
      {
        if (a.in_step == 0) a.u1[ok] = un;
        if (a.in_step < 2 || a.in_step == 3)
          un -= dt / 2.0 * (dd - s);
        else if (a.in_step == 2)
        {
          const double rhs = -dd + s;
          un = 1.0 / 3.0 * un + 2.0 / 3.0 * u1v + dt / 6.0 * rhs;
        }
      }
      else
      {
        const double rhs = -dd + s;
        const double r1 = a.rk_a * u1v + dt * rhs;
        a.u1[ok] = r1;
        un += a.rk_b * r1;
      }
      a.u0w[ok] = un;
      S[so] = un;
    }
  }
  __syncthreads();
  {
    const int n_ft = MF / 16;
    for (int rt = wave; rt < n_ft; rt += W)
    {
      g_f64x4 acc[NF];
#pragma unroll
      for (int f = 0; f < NF; f++) acc[f] = g_f64x4{0.0, 0.0, 0.0, 0.0};
      tile_mac<NF>(acc, a.o0, MF, rt, S, KU * GB, KU / 4, li, lk);
      const int row = rt * 16 + li;
      if (row < nfp)
#pragma unroll
        for (int f = 0; f < NF; f++)
#pragma unroll
          for (int rg = 0; rg < 4; rg++)
          {
            const int el = lk + 4 * rg;
            if (el < nval) a.disu_next[row + (long)nfp * (e0 + el) + f * plane_f] = acc[f][rg];
          }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static int padded_operator(DevBuf<double> &dst, const Operator &op, int M, int K)
{
  HFX_CHECK(op.present(), "general fused stage: an operator is missing");
  std::vector<double> h((size_t)op.m * op.k), p((size_t)M * K, 0.0);
  HFX_HIP(hipMemcpy(h.data(), op.dense, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
  for (int c = 0; c < op.k; c++)
    for (int r = 0; r < op.m; r++) p[r + (size_t)M * c] = h[r + (size_t)op.m * c];
  return dst.upload(p);
}

// the block's index in GENERAL_SIZES, or -1
static int general_size_class(const hfx_eles *e)
{
  for (int i = 0; i < N_GENERAL_SIZES; i++)
    if (e->n_upts == GENERAL_SIZES[i][0] && e->n_fpts == GENERAL_SIZES[i][1]) return i;
  return -1;
}

static int general_build(hfx_eles *e, hfx_inters *const *faces, int nfb, hfx_eles *const *eles, int neb)
{
  HFX_CHECK(e->n_dims == 3 && e->n_fields == 5, "general fused stage: three-dimensional Navier-Stokes / Euler blocks only; a two-dimensional "
            "block runs per method (fused 0), quadrilaterals of orders 1..4 also through the 2-D simplex stage with option blocks_2d 1");
  // (shock capturing follows the stage as its own step: general_shock_capture; an LES closure is evaluated in the flux kernel;
  // over-integration: the de-aliased flux is formed by the dense contractions before the flux kernel, which takes it in P3)
  HFX_CHECK(!(e->les_ready && e->over_int_ready), "general fused stage: an LES closure together with over-integration runs per method");
  if (e->les_ready)
  {
    HFX_CHECK(general_size_class(e) >= 0 && e->ctx->params.viscous, "general fused stage: the LES closure is built for tetrahedra / prisms of orders 1..3 on a viscous run");
    // (partitioned blocks: the projected flux a partition face sends already contains F_sgs . n -- no third message; the
    // SVV closure filters the state after its flux-point values have left for the neighbours)
    for (int b = 0; b < nfb; b++)
      HFX_CHECK(!faces[b]->is_mpi || e->les.sgs_model != 3, "general fused stage: the SVV closure on partitioned blocks runs per method");
  }
  if (!e->general) e->general.reset(new GeneralData());
  GeneralData *g = e->general.get();
  if (e->les_ready && e->les.sgs_model != 3 && les_len2_upload(e, g->les_len2)) return 1;
  const bool visc = e->ctx->params.viscous != 0;
  HFX_CHECK(!visc || e->viscous_ops, "general fused stage: viscous run but the block has no opp_4/5/6");
  const int nu = e->n_upts, nfp = e->n_fpts;
  g->KU = (nu + 3) & ~3; g->KF = (nfp + 3) & ~3; g->MU = (nu + 15) & ~15; g->MF = (nfp + 15) & ~15;
  HFX_CHECK(general_flux_lds_bytes(nu, nfp) <= 160 * 1024, "general fused stage: a batch of this element class (%d solution, %d flux points) does not fit LDS", nu, nfp);
  if (padded_operator(g->o0, e->opp_0, g->MF, g->KU) || padded_operator(g->o3, e->opp_3, g->MU, g->KF)) return 1;
  for (int d = 0; d < 3; d++)
    if (padded_operator(g->o1[d], e->opp_1[d], g->MF, g->KU) || padded_operator(g->o2[d], e->opp_2[d], g->MU, g->KU)) return 1;
  {
    // the folded operators: O2f[d] = opp_2[d] - opp_3 . opp_1[d] (sum over the flux points in ascending order)
    std::vector<double> o3((size_t)nu * nfp), o1((size_t)nfp * nu), o2((size_t)nu * nu), pad((size_t)g->MU * g->KU);
    HFX_HIP(hipMemcpy(o3.data(), e->opp_3.dense, sizeof(double) * o3.size(), hipMemcpyDeviceToHost));
    for (int d = 0; d < 3; d++)
    {
      HFX_HIP(hipMemcpy(o1.data(), e->opp_1[d].dense, sizeof(double) * o1.size(), hipMemcpyDeviceToHost));
      HFX_HIP(hipMemcpy(o2.data(), e->opp_2[d].dense, sizeof(double) * o2.size(), hipMemcpyDeviceToHost));
      std::fill(pad.begin(), pad.end(), 0.0);
      for (int c = 0; c < nu; c++)
        for (int r = 0; r < nu; r++)
        {
          double t = 0.0;
          for (int j = 0; j < nfp; j++) t += o3[r + (size_t)nu * j] * o1[j + (size_t)nfp * c];
          pad[r + (size_t)g->MU * c] = o2[r + (size_t)nu * c] - t;
        }
      if (g->o2f[d].upload(pad)) return 1;
    }
  }
  if (visc)
  {
    if (padded_operator(g->o6, e->opp_6, g->MF, g->KU)) return 1;
    for (int d = 0; d < 3; d++)
      if (padded_operator(g->o4[d], e->opp_4[d], g->MU, g->KU) || padded_operator(g->o5[d], e->opp_5[d], g->MU, g->KF)) return 1;
  }
  // per flux point: the LDG switch of the pair it is the LEFT point of (exact tests on the left normal, decided once),
  // and whether a boundary face owns it; every flux point must belong to exactly one registered face
  const long plane_f = (long)nfp * e->n_eles;
  std::vector<unsigned char> meta(plane_f, 0);
  std::vector<char> owned(plane_f, 0);
  std::vector<double> norm((size_t)plane_f * 3);
  HFX_HIP(hipMemcpy(norm.data(), e->norm_fpts, sizeof(double) * norm.size(), hipMemcpyDeviceToHost));
  g->any_bdy = false;
  for (int b = 0; b < nfb; b++)
  {
    hfx_inters *f = faces[b];
    if (f->is_mpi)
    {
      // partition faces (hfx_run_steps_partitioned_blocks): the point's correction and common flux come from the one-sided
      // kernels of kernels_mpi.hpp, like a boundary point's; what leaves for the neighbour is the point's Fn
      if (f->left == e)
        for (int o : f->hL) owned[o] = 1;
      continue;
    }
    if (f->is_bdy)
    {
      if (f->left != e) continue;
      g->any_bdy = true;
      for (int o : f->hL) { meta[o] |= 4; owned[o] = 1; }
      continue;
    }
    const long np = (long)f->n_inters * f->n_fpts_per_inter;
    if (f->left == e)
      for (long q = 0; q < np; q++)
      {
        const int il = f->hL[q];
        owned[il] = 1;
        const double n[3] = {norm[il], norm[il + plane_f], norm[il + 2 * plane_f]};
        if (ldg_switch<3>(1.0, n) < 0) meta[il] |= 2;
      }
    if (f->right == e)
      for (long q = 0; q < np; q++) owned[f->hR[q]] = 1;
  }
  for (long o = 0; o < plane_f; o++) HFX_CHECK(owned[o], "general fused stage: flux point %ld belongs to no registered face", o);
  {
    // partner words: pairs inside this block and pairs with another block of this call (mixed meshes: prism | tetrahedron faces);
    // the beta sign is the LEFT point's (decided above for this block's left points; for a pair whose left side lies in another
    // block it is decided here the same way, from that block's normals)
    std::vector<int> nbr(plane_f, -1);
    bool fits = neb <= 4, any = false;
    for (int i = 0; i < neb; i++) fits = fits && (long)eles[i]->n_fpts * eles[i]->n_eles < (1L << 27);
    auto block_of = [&](const hfx_eles *x) { for (int i = 0; i < neb; i++) if (eles[i] == x) return i; return -1; };
    for (int b = 0; b < nfb && fits; b++)
    {
      hfx_inters *f = faces[b];
      if (f->is_bdy || f->is_mpi || (f->left != e && f->right != e)) continue;
      const int bl = block_of(f->left), br = block_of(f->right);
      if (bl < 0 || br < 0) { fits = false; break; }
      const long np = (long)f->n_inters * f->n_fpts_per_inter;
      std::vector<double> nl;
      const long plane_l = (long)f->left->n_fpts * f->left->n_eles;
      if (f->left != e)
      {
        nl.resize((size_t)plane_l * 3);
        HFX_HIP(hipMemcpy(nl.data(), f->left->norm_fpts, sizeof(double) * nl.size(), hipMemcpyDeviceToHost));
      }
      for (long q = 0; q < np; q++)
      {
        const int il = f->hL[q], ir = f->hR[q];
        int flip;
        if (f->left == e)
          flip = meta[il] & 2;
        else
        {
          const double n[3] = {nl[il], nl[il + plane_l], nl[il + 2 * plane_l]};
          flip = ldg_switch<3>(1.0, n) < 0 ? 2 : 0;
        }
        if (f->left == e) nbr[il] = (ir << 4) | (br << 2) | flip;
        if (f->right == e) nbr[ir] = (il << 4) | (bl << 2) | flip | 1;
        any = true;
      }
    }
    g->nbr.reset();
    g->n_blocks = 0;
    if (fits && any)
    {
      if (g->nbr.upload(nbr)) return 1;
      g->n_blocks = neb;
      for (int i = 0; i < neb; i++) g->blocks[i] = eles[i];
    }
  }
  if (g->meta.upload(meta)) return 1;
  if (g->disu_alt.ensure((size_t)plane_f * e->n_fields) || g->fn_fpts.ensure((size_t)plane_f * e->n_fields)) return 1;
  g->built = true;
  return 0;
}

GeneralPlan general_plan(const hfx_eles *e)
{
  const hfx_ctx::Options &opt = e->ctx->opt;
  const int nu = e->n_upts, nfp = e->n_fpts, viscous = e->ctx->params.viscous;
  GeneralPlan pl;
  pl.size_class = general_size_class(e);
  pl.flux_waves = opt.general_waves ? opt.general_waves : general_flux_default_waves(nu, nfp);
  pl.flux_batched = pl.size_class >= 0 && general_flux_batched(nu, nfp, pl.flux_waves);
  pl.gather = opt.gather_delta && viscous && pl.flux_batched && e->general && e->general->nbr;
  pl.les = e->les_ready && e->les.sgs_model != 3 && viscous;
  pl.update_waves = opt.general_update_waves ? opt.general_update_waves : general_update_batched(nu, nfp, 4) ? 4 : 8;
  pl.flux_lds = general_flux_lds_bytes(nu, nfp); pl.update_lds = general_update_lds_bytes(nu, nfp);
  pl.fold = opt.fold_general != 0;
  return pl;
}

static GenArgs gen_args(hfx_eles *e, const GeneralPlan &pl, int in_step)
{
  GeneralData *g = e->general.get();
  const hfx_params &p = e->ctx->params;
  GenArgs a{};
  a.inv_nu = (unsigned)(4294967296ull / (unsigned)e->n_upts) + 1u; a.inv_nfp = (unsigned)(4294967296ull / (unsigned)e->n_fpts) + 1u;
  a.n_eles = e->n_eles; a.nu = e->n_upts; a.nfp = e->n_fpts; a.KU = g->KU; a.KF = g->KF; a.MU = g->MU; a.MF = g->MF;
  a.o0 = g->o0; a.o3 = g->o3; a.o6 = g->o6;
  a.fold = pl.fold ? 1 : 0;
  for (int d = 0; d < 3; d++) { a.o1[d] = g->o1[d]; a.o2[d] = a.fold ? g->o2f[d] : g->o2[d]; a.o4[d] = g->o4[d]; a.o5[d] = g->o5[d]; }
  a.u0 = e->arr[HFX_DISU_UPTS0]; a.delta = e->arr[HFX_DELTA_DISU_FPTS]; a.disu = e->arr[HFX_DISU_FPTS];
  a.detjac_upts = e->detjac_upts; a.JGinv_upts = e->JGinv_upts; a.detjac_fpts = e->detjac_fpts; a.JGinv_fpts = e->JGinv_fpts;
  a.norm_fpts = e->norm_fpts; a.meta = g->meta;
  a.nbr = pl.gather ? g->nbr : nullptr;
  for (int i = 0; i < 4; i++)
  {
    a.disu_b[i] = (i < g->n_blocks) ? g->blocks[i]->arr[HFX_DISU_FPTS] : nullptr;
    a.plane_b[i] = (i < g->n_blocks) ? (long)g->blocks[i]->n_fpts * g->blocks[i]->n_eles : 0;
  }
  a.div = e->arr[HFX_DIV_TCONF_UPTS]; a.ntd = e->arr[HFX_NORM_TDISF_FPTS]; a.fn = g->fn_fpts;
  a.grad_fpts = (g->any_bdy && p.viscous) ? e->arr[HFX_GRAD_DISU_FPTS] : nullptr;
  a.P = e->ctx->phys();
  a.u0w = e->arr[HFX_DISU_UPTS0]; a.u1 = e->arr[HFX_DISU_UPTS1];
  a.tconf = e->arr[HFX_NORM_TCONF_FPTS]; a.div_in = e->arr[HFX_DIV_TCONF_UPTS];
  a.src = e->src_nonzero ? e->arr[HFX_SRC_UPTS] : nullptr;
  a.dt_local = e->arr[HFX_DT_LOCAL];
  a.disu_next = g->disu_alt;
  a.nan_flag = e->nan_flag;
  a.adv_type = p.adv_type; a.in_step = in_step; a.dt_local_on = p.dt_type == 2; a.dt = p.dt;
  a.rk_a = (p.adv_type >= 3) ? p.RK_a[in_step] : 0.0;
  a.rk_b = (p.adv_type >= 3) ? p.RK_b[in_step] : 0.0;
  // (low-storage schemes: a stage whose RK_a is 0.0 -- the first of a step -- takes 0.0 for the register instead of reading it)
  a.need_u1 = (p.adv_type >= 3 && a.rk_a != 0.0) || (p.adv_type == 1 && in_step == 3) || (p.adv_type == 2 && in_step == 2);
  if (e->ctx->opt.flux_stamps) (void)g->stamps.ensure_zeroed(16 * 16); // (diagnostics: without the buffer the kernel takes none)
  a.stamps = g->stamps;
  a.les = e->les; a.les_len2 = g->les_len2; a.tdA_fpts = e->tdA_fpts;
  a.tdisf_in = e->over_int_ready ? e->arr[HFX_TDISF_UPTS] : nullptr;
  a.write_div = 1; // the flux kernel left the discontinuous part there: always complete it (the monitors read it)
  return a;
}

// the pairs of an interior-face block; its two sides may belong to different element blocks
static FacePairArgs gface_args(hfx_inters *f)
{
  auto side = [](hfx_eles *x) {
    FaceSide s{};
    s.plane = (long)x->n_fpts * x->n_eles;
    s.disu = x->arr[HFX_DISU_FPTS]; s.fn = x->general->fn_fpts; s.tdA = x->tdA_fpts;
    s.delta = x->arr[HFX_DELTA_DISU_FPTS]; s.tconf = x->arr[HFX_NORM_TCONF_FPTS];
    return s;
  };
  FacePairArgs a{};
  a.npairs = (long)f->n_inters * f->n_fpts_per_inter;
  a.L = f->L; a.R = f->R; a.meta = f->left->general->meta; a.norm = f->left->norm_fpts;
  a.l = side(f->left); a.r = side(f->right);
  return a;
}

template <int W, int NUc, int NFPc>
static int launch_element_kernels_t(hfx_eles *e, const GenArgs &a, const GeneralPlan &pl, bool flux)
{
  const dim3 grid((unsigned)((e->n_eles + GB - 1) / GB)), block(64 * W);
  // (function attributes are per device: set whenever the image exceeds the default, as launch_dense does -- a cached
  // "configured" size would be wrong for a second context on another GPU of the same process)
  auto launch = [&](auto kernel, size_t lds) -> int {
    if (lds > 48 * 1024) HFX_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, grid, block, lds, e->ctx->stream, a);
    HFX_HIP(hipGetLastError());
    return 0;
  };
  if (!flux) return launch(general_update_kernel<W, NUc, NFPc>, pl.update_lds);
  if constexpr (NUc != 0)
    if (pl.les) return launch(general_flux_kernel<W, NUc, NFPc, true>, pl.flux_lds);
  HFX_CHECK(!pl.les, "general fused stage: the LES closure is built for the element classes with compile-time sizes");
  return launch(general_flux_kernel<W, NUc, NFPc>, pl.flux_lds);
}

// the instantiation of the plan's size class (GENERAL_SIZES[I], I counting up), else the size-generic one
template <int W, int I = 0>
static int launch_element_kernels(hfx_eles *e, const GenArgs &a, const GeneralPlan &pl, bool flux)
{
  if constexpr (I == N_GENERAL_SIZES)
    return launch_element_kernels_t<W, 0, 0>(e, a, pl, flux);
  else
    return pl.size_class == I ? launch_element_kernels_t<W, GENERAL_SIZES[I][0], GENERAL_SIZES[I][1]>(e, a, pl, flux)
                              : launch_element_kernels<W, I + 1>(e, a, pl, flux);
}

static int launch_element_kernels(int waves, hfx_eles *e, const GenArgs &a, const GeneralPlan &pl, bool flux)
{
  return waves == 3 ? launch_element_kernels<3>(e, a, pl, flux) : waves == 4 ? launch_element_kernels<4>(e, a, pl, flux)
                                                                              : launch_element_kernels<8>(e, a, pl, flux);
}

GeneralStage::GeneralStage(hfx_eles *const *eles_, int neb_, hfx_inters *const *faces_, int nfb_, int in_step_, bool shock_)
    : eles(eles_), faces(faces_), neb(neb_), nfb(nfb_), simplex2d(simplex2d_stage_call(eles_, neb_)), in_step(in_step_), shock(shock_)
{
  if (simplex2d) return;
  for (int i = 0; i < neb; i++) args.push_back(gen_args(eles[i], plans.emplace_back(general_plan(eles[i])), in_step_));
}

int GeneralStage::interior_ldg() const
{
  if (simplex2d) return simplex2d_interior_ldg(eles[0], faces, nfb);
  hfx_ctx *ctx = eles[0]->ctx;
  if (!ctx->params.viscous) return 0;
  auto gathers = [&](const hfx_eles *x) { return plans[std::find(eles, eles + neb - 1, x) - eles].gather; }; // (x is a block of the call)
  for (int b = 0; b < nfb; b++)
  {
    if (faces[b]->is_bdy && hfx_bdy_launch_internal(faces[b], 0, 1)) return 1; // ghost state -> inviscid common flux, LDG common solution
    if (faces[b]->is_bdy || faces[b]->is_mpi) continue;
    if (gathers(faces[b]->left) && gathers(faces[b]->right)) continue; // both sides' flux kernels form these corrections themselves
    const FacePairArgs a = gface_args(faces[b]);
    if (a.npairs == 0) continue;
    hipLaunchKernelGGL(face_delta_kernel<3>, dim3((unsigned)((a.npairs + 255) / 256)), dim3(256), 0, ctx->stream, a, ctx->phys());
  }
  HFX_HIP(hipGetLastError());
  return 0;
}

int GeneralStage::flux_kernels() const
{
  // (a triangle block's over-integration: inside the element kernel, or -- option fold_over_int 0 -- per method in front of it)
  // (several blocks, option blocks_2d: one launch per block; none of them registered over-integration)
  if (simplex2d)
  {
    for (int i = 0; i < neb; i++)
      if (simplex2d_over_int_unfolded(eles[i]) || simplex2d_element_kernel(eles[i], in_step)) return 1;
    return 0;
  }
  for (int i = 0; i < neb; i++)
  {
    // polynomial de-aliasing (src/solver.cpp:82-91): tdisf_upts = over_int_filter . F(opp_over_int_cubpts . u)
    if (eles[i]->over_int_ready && hfx_eles_evaluate_invFlux_over_int(eles[i])) return 1;
    if (launch_element_kernels(plans[i].flux_waves, eles[i], args[i], plans[i], true)) return 1;
  }
  return 0;
}

int GeneralStage::common_fluxes() const
{
  if (simplex2d) return simplex2d_common_fluxes(eles[0], faces, nfb);
  hfx_ctx *ctx = eles[0]->ctx;
  const Phys P = ctx->phys();
  // boundary faces beside the interior ones: both need the flux kernels' results and write norm_tconf at disjoint points
  bool any_bdy = false;
  for (int b = 0; b < nfb; b++) any_bdy = any_bdy || (faces[b]->is_bdy && faces[b]->n_inters > 0);
  const bool beside = any_bdy && ctx->opt.bdy_beside;
  if (beside && side_stream_fork(ctx)) return 1;
  for (int b = 0; b < nfb; b++)
    if (faces[b]->is_bdy && hfx_bdy_launch_internal(faces[b], P.viscous ? 1 : 0, 1)) return 1;
  if (beside && side_stream_join(ctx)) return 1;
  // all interior-face blocks in one launch (groups of GFACE_MAX_BLOCKS)
  GFaceMulti m{};
  auto flush = [&]() {
    if (m.nb > 0)
      with_riemann_solver(P.riemann, [&](auto RS) { hipLaunchKernelGGL(gface_flux_multi_kernel<decltype(RS)::value>, dim3(m.wg_start[m.nb]), dim3(256), 0, ctx->stream, m); });
    m.nb = 0;
  };
  for (int b = 0; b < nfb; b++)
  {
    if (faces[b]->is_bdy || faces[b]->is_mpi) continue;
    const FacePairArgs a = gface_args(faces[b]);
    if (a.npairs == 0) continue;
    m.blk[m.nb] = {a, P};
    m.wg_start[m.nb + 1] = m.wg_start[m.nb] + (unsigned)((a.npairs + 255) / 256);
    if (++m.nb == GFACE_MAX_BLOCKS) flush();
  }
  flush();
  if (beside && side_stream_wait(ctx)) return 1;
  HFX_HIP(hipGetLastError());
  return 0;
}

int GeneralStage::update_kernels() const
{
  if (simplex2d)
  {
    for (int i = 0; i < neb; i++) // (each launch, then that block's disu_fpts buffers change places; no block reads another's here)
      if (simplex2d_update_kernel(eles[i], in_step, S2dList::all, shock)) return 1;
    return 0;
  }
  for (int i = 0; i < neb; i++)
    if (launch_element_kernels(plans[i].update_waves, eles[i], args[i], plans[i], false)) return 1;
  for (int i = 0; i < neb; i++) std::swap(eles[i]->arr[HFX_DISU_FPTS], eles[i]->general->disu_alt);
  return 0;
}

int general_prepare(hfx_eles *const *eles, int neb, hfx_inters *const *faces, int nfb, bool partitioned)
{
  hfx_ctx *ctx = eles[0]->ctx;
  for (int i = 0; i < neb; i++)
  {
    HFX_CHECK(eles[i] && eles[i]->ctx == ctx, "element blocks of different contexts");
    HFX_CHECK(eles[i]->n_eles > 0, "general fused stage: empty element block");
  }
  for (int b = 0; b < nfb; b++)
  {
    bool l = false, r = faces[b]->right == nullptr;
    for (int i = 0; i < neb; i++)
    {
      l = l || faces[b]->left == eles[i];
      r = r || faces[b]->right == eles[i];
    }
    HFX_CHECK(l && r, "face block %d refers to an element block that is not part of this call", b);
  }
  // a two-dimensional block of a non-tensor class (triangles): the 2-D simplex stage's tables (one block; partition faces in
  // the partitioned stage alone).  Option blocks_2d: several two-dimensional blocks, or one of quadrilaterals, likewise
  if (simplex2d_takes(eles, neb, partitioned)) return simplex2d_prepare(eles, neb, faces, nfb, partitioned);
  for (int i = 0; i < neb; i++)
  {
    GeneralData *g = eles[i]->general.get();
    bool same = g && g->built;
    if (same && g->n_blocks)
    {
      same = g->n_blocks == neb;
      for (int j = 0; j < neb && same; j++) same = g->blocks[j] == eles[j];
    }
    if (!same)
      if (general_build(eles[i], faces, nfb, eles, neb)) return 1;
  }
  return 0;
}

const double *general_fn_fpts(const hfx_eles *e)
{
  if (simplex2d_runs(e)) return simplex2d_fn_fpts(e);
  return e->general ? e->general->fn_fpts : nullptr;
}

// eles::shock_capture behind a general fused stage (src/HiFiLES.cpp:214-216): the modal filter changes the state of the elements
// the sensor marks, so the flux-point values the update kernel left for the next stage are extrapolated again
int general_shock_capture(hfx_eles *const *eles, int neb)
{
  for (int i = 0; i < neb; i++)
    if (eles[i]->shock_ready && !simplex2d_folds_shock(eles[i])) // (a triangle stage that folded the filter left the sensor, the filtered state and its disu_fpts)
    {
      if (hfx_eles_shock_capture(eles[i])) return 1;
      if (hfx_eles_extrapolate_solution(eles[i])) return 1;
    }
  return 0;
}

int general_run_steps(hfx_eles *const *eles, int neb, hfx_inters *const *faces, int nfb, int n_steps)
{
  if (general_prepare(eles, neb, faces, nfb)) return 1;
  if (n_steps <= 0) return 0; // (a call without steps prepares the blocks' tables and leaves the state alone)
  // disu_fpts of the current state (the caller may have changed disu_upts since the last call)
  for (int i = 0; i < neb; i++)
    if (hfx_eles_extrapolate_solution(eles[i])) return 1;
  StepLoop loop{eles, neb, faces, nfb, [&](int rk) { return GeneralStage(eles, neb, faces, nfb, rk).run() || general_shock_capture(eles, neb); }};
  loop.closure = ClosureFilter::filtering_refresh_svv;
  // the stage keeps the gradient on chip: the last stage of a step a gradient-reading monitor samples runs call by call
  loop.by_calls = monitor_reads_gradient(eles, neb);
  bool by_calls = false;
  if (run_step_loop(loop, n_steps, &by_calls)) return 1;
  for (int i = 0; i < neb; i++) note_gradients(eles[i], by_calls); // (the general stage keeps them on chip)
  return 0;
}

int general_time_kernels(hfx_eles *const *eles, int neb, hfx_inters *const *faces, int nfb, int reps, double *ms)
{
  if (general_prepare(eles, neb, faces, nfb)) return 1;
  const int nst = n_rk_stages(eles[0]->ctx->params);
  hipStream_t st = eles[0]->ctx->stream;
  // one set of events per repetition and ONE synchronisation at the end: a host synchronisation per stage let the queue
  // run dry, and the first kernel after it (the flux kernel) then measured 10 % slower than in the running pipeline
  std::vector<hipEvent_t> ev((size_t)reps * 5);
  // a triangle block whose over-integration runs per method in front of the element kernel: its own slot (SLOT_OVER_INT)
  const bool oi_slot = neb == 1 && is_simplex2d(eles[0]) && simplex2d_plan(eles[0]).over_int && !simplex2d_plan(eles[0]).fold_over_int;
  std::vector<hipEvent_t> ev_oi(oi_slot ? (size_t)reps : 0);
  for (auto &x : ev_oi) HFX_HIP(hipEventCreate(&x));
  for (auto &x : ev) HFX_HIP(hipEventCreate(&x));
  for (int i = 0; i < neb; i++)
    if (hfx_eles_extrapolate_solution(eles[i])) return 1;
  double acc[4] = {0, 0, 0, 0}, acc_oi = 0.0;
  for (int r = 0; r < reps; r++)
  {
    const GeneralStage stage(eles, neb, faces, nfb, r % nst);
    HFX_HIP(hipEventRecord(ev[5 * r], st));
    if (stage.interior_ldg()) return 1;
    HFX_HIP(hipEventRecord(ev[5 * r + 1], st));
    if (oi_slot)
    {
      if (simplex2d_over_int_unfolded(eles[0])) return 1;
      HFX_HIP(hipEventRecord(ev_oi[r], st));
      if (simplex2d_element_kernel(eles[0], r % nst)) return 1;
    }
    else if (stage.flux_kernels()) return 1;
    HFX_HIP(hipEventRecord(ev[5 * r + 2], st));
    if (stage.common_fluxes()) return 1;
    HFX_HIP(hipEventRecord(ev[5 * r + 3], st));
    if (stage.update_kernels()) return 1;
    HFX_HIP(hipEventRecord(ev[5 * r + 4], st));
  }
  HFX_HIP(hipStreamSynchronize(st));
  for (int r = 0; r < reps; r++)
    for (int w = 0; w < 4; w++)
    {
      float t = 0;
      HFX_HIP(hipEventElapsedTime(&t, ev[5 * r + w], ev[5 * r + w + 1]));
      acc[w] += t;
    }
  for (int r = 0; r < reps && oi_slot; r++)
  {
    float t = 0;
    HFX_HIP(hipEventElapsedTime(&t, ev[5 * r + 1], ev_oi[r]));
    acc_oi += t;
    acc[1] -= t;
  }
  for (auto &x : ev) (void)hipEventDestroy(x);
  for (auto &x : ev_oi) (void)hipEventDestroy(x);
  for (int i = 0; i < 8; i++) ms[i] = (i < 4) ? acc[i] / reps : 0.0;
  if (oi_slot) ms[SLOT_OVER_INT] = acc_oi / reps;
  for (int i = 0; i < neb; i++) note_gradients(eles[i], false);
  for (int i = 0; i < neb; i++)
  {
    GeneralData *g = eles[i]->general.get();
    if (!g || !g->stamps) continue;
    long long h[16 * 16];
    HFX_HIP(hipMemcpy(h, g->stamps, sizeof h, hipMemcpyDeviceToHost));
    for (int w = 0; w < 8 && h[w * 16] != 0; w++)
    {
      fprintf(stderr, "general flux kernel (block %d) wave %d cycles: ", i, w);
      for (int q = 1; q <= 9; q++) fprintf(stderr, "%s%lld", q > 1 ? " " : "", h[w * 16 + q] - h[w * 16 + q - 1]);
      fprintf(stderr, "   (P0 | bar | P1 | bar | P2 | bar | P3 | bar | P4)  total %lld\n", h[w * 16 + 9] - h[w * 16]);
    }
  }
  return 0;
}

// ALGORITHMIC HBM bytes per launch of the four kernels, summed over the element blocks (doubles listed per element)
void general_kernel_bytes(hfx_eles *const *eles, int neb, double *bytes)
{
  for (int i = 0; i < 8; i++) bytes[i] = 0.0;
  for (int i = 0; i < neb; i++)
  {
    const hfx_eles *e = eles[i];
    if (simplex2d_runs(e))
    {
      simplex2d_kernel_bytes(e, bytes);
      continue;
    }
    const double nu = e->n_upts, nfp = e->n_fpts, nf = e->n_fields, nd = e->n_dims, ne = e->n_eles;
    bytes[0] += ne * (8.0 * (2 * nfp * nf) + 4.0 * nfp + nfp * 0.5);                                        // disu r, delta w, index + meta
    bytes[1] += ne * 8.0 * (nu * nf + nfp * nf + nu * (nd * nd + 1) + nfp * (nd * nd + 1) + nfp * nd + nfp * nf // u, delta, metrics, normals, disu r
                            + nu * nf + 2 * nfp * nf);                                                       // div, norm_tdisf, Fn w
    bytes[2] += ne * (8.0 * (nfp * nf + nfp * nf + 0.5 * nfp * nd + nfp + nfp * nf) + 4.0 * nfp);            // disu, Fn, normal(left), tdA r; tconf w
    bytes[3] += ne * 8.0 * (3 * nu * nf + nu + 2 * nfp * nf + 3 * nu * nf + nfp * nf);                       // u0,u1,div,detjac,tconf,ntd r; u0,u1,div,disu w
    const GeneralPlan pl = general_plan(e);
    if (pl.fold)
    {
      // folded correction: norm_tdisf is neither written (flux kernel) nor read (update kernel)
      bytes[1] -= ne * 8.0 * nfp * nf;
      bytes[3] -= ne * 8.0 * nfp * nf;
    }
    if (pl.gather)
    {
      // LDG corrections formed in the flux kernel: the pairwise kernel is not launched for the pairs inside the block (the
      // partner values it reads are as many doubles as the corrections it no longer reads) + a partner word per point
      bytes[0] -= ne * (8.0 * (2 * nfp * nf) + 4.0 * nfp + nfp * 0.5);
      bytes[1] += ne * 4.0 * nfp;
    }
  }
}

} // namespace hfx

extern "C" int hfx_general_plan(hfx_eles *e, int out[8])
{
  HFX_CHECK(e && out, "hfx_general_plan: bad argument");
  HFX_IMMEDIATE(e->ctx, 0);
  HFX_CHECK(e->general && e->general->built, "hfx_general_plan: no general fused stage has prepared this block (run fused 4 first)");
  const hfx::GeneralPlan pl = hfx::general_plan(e);
  const int v[8] = {pl.size_class, pl.flux_waves, pl.flux_batched, pl.gather, pl.les, pl.update_waves, pl.fold, (int)pl.flux_lds};
  for (int i = 0; i < 8; i++) out[i] = v[i];
  return 0;
}
