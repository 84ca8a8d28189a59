// fused_hex.hip -- the split fused stage for tensor-product elements (hexes, quads): table setup (fused_build), the plan
// (split_plan), one stage as named steps (SplitStage::make and SplitStageT, one instantiation per element size), RK loops.
// Kernels: split_common.hpp (shared helpers), split2_kernels.hpp (variant 2), split3_kernels.hpp (variant 3, the default),
// split_partitioned.hpp (the steps of a stage on a partitioned block).
//
// One RK stage = the 17 calls of CalcResidual + AdvanceSolution
// (/root/reference/src/solver.cpp:50-223, src/HiFiLES.cpp:201-217).  Executed call by
// call they stream ~64 000 doubles per P4 hex through HBM.  Here the stage is cut at the two
// places where data must cross elements (the LDG common solution, the common fluxes) and everything element-local
// between two cuts is one kernel: four launches per stage, three when the flux kernel forms the LDG corrections itself
// (DESIGN.md 3.2).  Two variants:
//   fused = 2: keeps the reference's arrays (grad_disu_upts / grad_disu_fpts in HBM); carries the LES closure
//   fused = 3: the kernel that has the corrected gradient in registers goes straight on to the fluxes; the default
// plus the same stage cut into five phases for a partitioned block (hfx_stage_partitioned).
//
// Operator rows of the element kernels are either sum-factorised (1-D matrices through scalar registers, when the
// registered operators are bit-exactly tensor products) or DICTIONARY-COMPRESSED sparse rows: a tensor-product
// operator has only a handful of distinct values, so a row entry is 16 bits (value id, column), two per 32-bit
// register, the values in a 2 kB LDS table.  Hexes from P6 on have columns beyond 8 bits: their entries are 32 bits
// (value id << 16 | column), one per register (Geo::WIDE); only variant 2 runs them (split_plan).  The arithmetic is unchanged: the same non-zeros, multiplied in the same
// ascending-column order as the reference dgemm (src/funcs.cpp:110-117).
#include <vector>
#include "fused_hex.hpp"
#include "step_loop.hpp"
#include "tensor_ops.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "kernels_mpi.hpp"
#include "physics.hpp"
#include "split3_kernels.hpp" // -> split2_kernels.hpp -> split_common.hpp: the kernels of both variants

namespace hfx
{

void fused_invalidate(hfx_eles *e)
{
  if (!e || !e->fused) return;
  e->fused->built = false;
  e->fused->les_len2.reset(); // (follows the registered closure)
}

void FusedDelete::operator()(FusedData *p) const { delete p; }

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
static int tensor_n(const hfx_eles *e)
{
  // N with N^ND = n_upts and 2 ND N^(ND-1) = n_fpts, or 0
  for (int n = 2; n <= 8; n++)
    if (ipow(n, e->n_dims) == e->n_upts && 2 * e->n_dims * ipow(n, e->n_dims - 1) == e->n_fpts) return n;
  return 0;
}

// The element sizes (n_dims, points per direction) the split stage is instantiated for: every dispatch on the element size
// applies a macro X(ND, N) to this list
#define HFX_SPLIT_SIZES(X) X(3, 2) X(3, 3) X(3, 4) X(3, 5) X(3, 6) X(3, 7) X(3, 8) X(2, 2) X(2, 3) X(2, 4) X(2, 5) X(2, 6) X(2, 7) X(2, 8)

// runtime forms of split3_fits and loader_wave_fits
static bool split3_fits_rt(int nd, int N)
{
#define HFX_X(ND_, N_) \
  if (nd == ND_ && N == N_) return split3_fits<ND_, N_>();
  HFX_SPLIT_SIZES(HFX_X)
#undef HFX_X
  return false;
}
static bool loader_wave_fits_rt(int nd, int N)
{
#define HFX_X(ND_, N_) \
  if (nd == ND_ && N == N_) return loader_wave_fits<ND_, N_>();
  HFX_SPLIT_SIZES(HFX_X)
#undef HFX_X
  return false;
}

struct Dict
{
  std::vector<double> vals;
  Dict() { vals.push_back(0.0); } // id 0 = +0.0: padding entries multiply by it
  int id(double v)
  {
    for (size_t i = 0; i < vals.size(); i++)
      if (std::memcmp(&vals[i], &v, sizeof v) == 0) return (int)i;
    vals.push_back(v);
    return (int)vals.size() - 1;
  }
};

// pack `w` entries per row of an operator given in host ELL form (width hw) at word offset `off`: `epw` = 2 entries of
// 16 bits (value id << 8 | column) per word, or 1 wide entry (value id << 16 | column)
static int pack_rows(std::vector<unsigned> &pk, size_t off, int m, int w, const double *hv, const int *hi, int hw, Dict &dict, int epw)
{
  const int cbits = epw == 2 ? 8 : 16;
  for (int r = 0; r < m; r++)
    for (int q = 0; q < w; q++)
    {
      const double v = (q < hw) ? hv[r + (size_t)m * q] : 0.0;
      const int c = (q < hw) ? hi[r + (size_t)m * q] : hi[r];
      HFX_CHECK(c >= 0 && c < (1 << cbits), "fused path: column %d does not fit a %d-bit row entry", c, cbits);
      const unsigned ent = ((unsigned)dict.id(v) << cbits) | (unsigned)c;
      pk[off + (size_t)(q / epw) * m + r] |= ent << (16 * (q % epw));
    }
  return 0;
}

template <int ND, int N>
static int build_packed(hfx_eles *e, FusedData *F, const std::vector<double> &o1v, const std::vector<int> &o1i)
{
  using G = Geo<ND, N>;
  constexpr int NU = G::NU, NFP = G::NFP, WN = G::WN, EPW = G::EPW;
  auto hw = [](const Operator &op) { return std::max(op.nnz_max, 1); };
  {
    Dict dict;
    std::vector<unsigned> pk(G::R_END, 0u);
    for (int d = 0; d < ND; d++)
      if (pack_rows(pk, G::R_O2 + (size_t)d * WN * NU, NU, N, e->opp_2[d].h_val.data(), e->opp_2[d].h_idx.data(), hw(e->opp_2[d]), dict, EPW)) return 1;
    if (pack_rows(pk, G::R_O3, NU, 2 * ND, e->opp_3.h_val.data(), e->opp_3.h_idx.data(), hw(e->opp_3), dict, EPW)) return 1;
    if (pack_rows(pk, G::R_O0, NFP, N, e->opp_0.h_val.data(), e->opp_0.h_idx.data(), hw(e->opp_0), dict, EPW)) return 1;
    if (pack_rows(pk, G::R_O1, NFP, N, o1v.data(), o1i.data(), N, dict, EPW)) return 1;
    HFX_CHECK(dict.vals.size() <= MAX_TAB, "fused path: operators hold %zu distinct values (> %d)", dict.vals.size(), MAX_TAB);
    dict.vals.resize(MAX_TAB, 0.0);
    if (F->pk_r.upload(pk) || F->tab_r.upload(dict.vals)) return 1;
  }
  if (e->viscous_ops)
  {
    Dict dict;
    std::vector<unsigned> pk(G::G_END, 0u);
    for (int d = 0; d < ND; d++)
    {
      if (pack_rows(pk, G::G_O4 + (size_t)d * WN * NU, NU, N, e->opp_4[d].h_val.data(), e->opp_4[d].h_idx.data(), hw(e->opp_4[d]), dict, EPW)) return 1;
      if (pack_rows(pk, G::G_O5 + (size_t)d * G::W2 * NU, NU, 2, e->opp_5[d].h_val.data(), e->opp_5[d].h_idx.data(), hw(e->opp_5[d]), dict, EPW)) return 1;
    }
    if (pack_rows(pk, G::G_O0, NFP, N, e->opp_0.h_val.data(), e->opp_0.h_idx.data(), hw(e->opp_0), dict, EPW)) return 1;
    if (pack_rows(pk, G::G_O6, NFP, N, e->opp_6.h_val.data(), e->opp_6.h_idx.data(), hw(e->opp_6), dict, EPW)) return 1;
    HFX_CHECK(dict.vals.size() <= MAX_TAB, "fused path: operators hold %zu distinct values (> %d)", dict.vals.size(), MAX_TAB);
    dict.vals.resize(MAX_TAB, 0.0);
    if (F->pk_g.upload(pk) || F->tab_g.upload(dict.vals)) return 1;
  }
  return 0;
}

static int dispatch_build_packed(hfx_eles *e, FusedData *F, int N, const std::vector<double> &o1v, const std::vector<int> &o1i)
{
#define HFX_X(ND_, N_) \
  if (e->n_dims == ND_ && N == N_) return build_packed<ND_, N_>(e, F, o1v, o1i);
  HFX_SPLIT_SIZES(HFX_X)
#undef HFX_X
  set_error("fused path: no kernel for N = %d, n_dims = %d", N, e->n_dims);
  return 1;
}


// ---------------------------------------------------------------------------------------
// Tensor-product structure of the registered operators (checked bit for bit; anything else keeps
// the dictionary kernels).  With collocated solution / flux bases on a tensor-product element
//   opp_4[d](p, .) = opp_2[d](p, .) : N entries D[i_d(p)][m] on the pencil through p along d
//   opp_5[d](p, .)                  : the pencil's two flux points, c5[d][q][i_d(p)]
//   opp_0(f, .) = opp_6(f, .)       : N entries Lf[d][q][m] on the pencil that ends in f
//   opp_1 merged (f, .)             : the same pencil, L1[d][q][m]
// (definitions: /root/reference/src/eles.cpp:3074-3596).
// ---------------------------------------------------------------------------------------
static int line_of(int nd, int N, int d, int p, int &i_d)
{
  // pencil of point p along d: its index among the N^(nd-1) lines, and the position i_d on it
  const int S = ipow(N, d);
  i_d = (p / S) % N;
  const int base = p - i_d * S;
  if (nd == 2) return d == 0 ? base / N : base;
  if (d == 0) return base / N;                    // (j,k): base = N (j + N k)
  if (d == 1) return (base % N) + N * (base / (N * N)); // (i,k): base = i + N^2 k
  return base;                                    // (i,j)
}
static int base_of_line(int nd, int N, int d, int line)
{
  if (nd == 2) return d == 0 ? N * line : line;
  if (d == 0) return N * line;
  if (d == 1) return (line % N) + N * N * (line / N);
  return line;
}

static bool bits_equal(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static int tensor_build(hfx_eles *e, FusedData *F, int N, const std::vector<double> &o1v, const std::vector<int> &o1i,
                        const std::vector<int> &o1d)
{
  F->tensor_ok = false;
  const int nd = e->n_dims, nu = e->n_upts, nfp = e->n_fpts, L = ipow(N, nd - 1);
  auto V = [](const Operator &op, int r, int q) { return op.h_val[r + (size_t)op.m * q]; };
  auto I = [](const Operator &op, int r, int q) { return op.h_idx[r + (size_t)op.m * q]; };
  for (int d = 0; d < nd; d++)
    if (e->opp_2[d].nnz_max != N) return 0;
  if (e->opp_0.nnz_max != N) return 0;
  const bool visc = e->viscous_ops;
  std::vector<double> Dm((size_t)N * N), c5((size_t)nd * 2 * N, 0.0), Lf((size_t)nd * 2 * N), L1((size_t)nd * 2 * N);
  std::vector<int> pf((size_t)nd * L * 2, -1), fdq(nfp, -1), fbase(nfp, -1);
  for (int i = 0; i < N; i++)
    for (int m = 0; m < N; m++) Dm[i * N + m] = V(e->opp_2[0], i, m);
  if (visc)
    for (int d = 0; d < nd; d++)
    {
      if (e->opp_5[d].nnz_max != 2) return 0;
      for (int p = 0; p < nu; p++)
      {
        int i_d;
        if (line_of(nd, N, d, p, i_d) != 0) continue;
        for (int q = 0; q < 2; q++) c5[((size_t)d * 2 + q) * N + i_d] = V(e->opp_5[d], p, q);
      }
    }
  for (int d = 0; d < nd; d++)
  {
    const int S = ipow(N, d);
    for (int p = 0; p < nu; p++)
    {
      int i_d;
      const int line = line_of(nd, N, d, p, i_d), base = p - i_d * S;
      for (int m = 0; m < N; m++)
      {
        if (I(e->opp_2[d], p, m) != base + m * S || !bits_equal(V(e->opp_2[d], p, m), Dm[i_d * N + m])) return 0;
        if (visc && (e->opp_4[d].nnz_max != N || I(e->opp_4[d], p, m) != base + m * S ||
                     !bits_equal(V(e->opp_4[d], p, m), Dm[i_d * N + m])))
          return 0;
      }
      if (visc)
      {
        if (e->opp_5[d].nnz_max != 2) return 0;
        for (int q = 0; q < 2; q++)
        {
          int &slot = pf[((size_t)d * L + line) * 2 + q];
          const int f = I(e->opp_5[d], p, q);
          if (slot < 0) slot = f;
          if (slot != f) return 0;
          if (!bits_equal(V(e->opp_5[d], p, q), c5[((size_t)d * 2 + q) * N + i_d])) return 0;
        }
      }
    }
  }
  if (!visc)
  {
    // inviscid blocks have no opp_5: find the two flux points of a pencil from opp_0's columns
    for (int f = 0; f < nfp; f++)
    {
      const int c0 = I(e->opp_0, f, 0), S = I(e->opp_0, f, 1) - c0;
      int d = -1;
      for (int dd = 0; dd < nd; dd++)
        if (S == ipow(N, dd)) d = dd;
      if (d < 0) return 0;
      int i_d;
      const int line = line_of(nd, N, d, c0, i_d);
      if (i_d != 0) return 0;
      int *slot = &pf[((size_t)d * L + line) * 2];
      if (slot[0] < 0) slot[0] = f;
      else if (slot[1] < 0) slot[1] = f;
      else return 0;
    }
  }
  // every flux point is the end of exactly one pencil
  for (int d = 0; d < nd; d++)
    for (int line = 0; line < L; line++)
      for (int q = 0; q < 2; q++)
      {
        const int f = pf[((size_t)d * L + line) * 2 + q];
        if (f < 0 || f >= nfp || fdq[f] >= 0) return 0;
        fdq[f] = d * 2 + q;
        fbase[f] = base_of_line(nd, N, d, line);
        const int S = ipow(N, d);
        if (o1d[f] != d) return 0;
        for (int m = 0; m < N; m++)
        {
          if (I(e->opp_0, f, m) != fbase[f] + m * S || o1i[f + (size_t)nfp * m] != fbase[f] + m * S) return 0;
          if (visc && (e->opp_6.nnz_max != N || I(e->opp_6, f, m) != fbase[f] + m * S ||
                       !bits_equal(V(e->opp_6, f, m), V(e->opp_0, f, m))))
            return 0;
          double &lf = Lf[((size_t)d * 2 + q) * N + m], &l1 = L1[((size_t)d * 2 + q) * N + m];
          if (line == 0)
          {
            lf = V(e->opp_0, f, m);
            l1 = o1v[f + (size_t)nfp * m];
          }
          if (!bits_equal(lf, V(e->opp_0, f, m)) || !bits_equal(l1, o1v[f + (size_t)nfp * m])) return 0;
        }
      }
  for (int f = 0; f < nfp; f++)
    if (fdq[f] < 0) return 0;
  // merged opp_1 row = tnorm * opp_0 row with tnorm = +-1 (exact): keep the sign only
  for (int dq = 0; dq < nd * 2; dq++)
  {
    double sgn = 0.0;
    for (int m = 0; m < N; m++)
    {
      const double lf = Lf[(size_t)dq * N + m], l1 = L1[(size_t)dq * N + m];
      const double s_m = bits_equal(l1, lf) ? 1.0 : (bits_equal(l1, -lf) ? -1.0 : 0.0);
      if (s_m == 0.0) return 0;
      if (lf != 0.0)
      {
        if (sgn != 0.0 && s_m != sgn) return 0;
        sgn = s_m;
      }
    }
    if (sgn == 0.0) return 0;
    L1[(size_t)dq * N] = sgn;
  }
  // opp_3 (the divergence of the correction functions): row p has one entry per flux point at the ends of the ND pencils
  // through p, and the entry depends on (direction, end, position on the pencil) only.  The flux kernel then applies
  // -opp_3 . norm_tdisf pencil-wise, from the pencil values it holds in registers anyway (folded correction)
  std::vector<double> c3((size_t)nd * 2 * N, 0.0);
  {
    const int w3 = std::max(e->opp_3.nnz_max, 1);
    std::vector<char> have((size_t)nd * 2 * N, 0);
    for (int p = 0; p < nu; p++)
    {
      int seen = 0;
      for (int d = 0; d < nd; d++)
      {
        int i_d;
        const int line = line_of(nd, N, d, p, i_d);
        for (int q = 0; q < 2; q++)
        {
          const int f = pf[((size_t)d * L + line) * 2 + q];
          double v = 0.0;
          for (int c = 0; c < w3; c++)
            if (I(e->opp_3, p, c) == f && V(e->opp_3, p, c) != 0.0)
            {
              v = V(e->opp_3, p, c);
              seen++;
            }
          const size_t slot = ((size_t)d * 2 + q) * N + i_d;
          if (!have[slot])
          {
            c3[slot] = v;
            have[slot] = 1;
          }
          if (!bits_equal(c3[slot], v)) return 0;
        }
      }
      int nonzero = 0;
      for (int c = 0; c < w3; c++) nonzero += V(e->opp_3, p, c) != 0.0;
      if (nonzero != seen) return 0; // an entry outside the pencil ends
    }
  }
  std::vector<double> coef;
  coef.insert(coef.end(), Dm.begin(), Dm.end());
  coef.insert(coef.end(), c5.begin(), c5.end());
  coef.insert(coef.end(), Lf.begin(), Lf.end());
  coef.insert(coef.end(), L1.begin(), L1.end());
  coef.insert(coef.end(), c3.begin(), c3.end());
  std::vector<int> idx;
  idx.insert(idx.end(), pf.begin(), pf.end());
  idx.insert(idx.end(), fdq.begin(), fdq.end());
  idx.insert(idx.end(), fbase.begin(), fbase.end());
  if (F->t_coef.upload(coef)) return 1;
  F->h_coef = coef;
  if (F->t_idx.upload(idx)) return 1;
  F->tensor_ok = true;
  return 0;
}

// ---------------------------------------------------------------------------------------
// Affine blocks.  On a parallelepiped the map from the reference element is affine: JGinv and detjac are the same at every point
// of the element, the normal and tdA the same at every point of a face.  The registered arrays hold them evaluated point by
// point from the eight-node shape derivatives and the vertex coordinates, so they agree to the rounding of that arithmetic
// only.  A block is AFFINE when every element's metrics agree with the element's representative (the first solution point; on
// a face: the face's first flux point) within
//     tol = AFFINE_C * eps * (1 + R),   R = (block volume / element volume)^(1/n_dims),
// relative to the element's own max |JGinv|, |detjac| and tdA (normals: absolute, they are unit vectors).  Derivation
// ("Affine blocks"): a Jacobian entry is a sum of eight products dN_i x_i with sum |dN_i| <= 1, so its error
// is below 11 eps max|x| on an entry of size h / 2; JGinv entries (differences of two products of Jacobian entries) carry 4
// such relative errors, detjac (six triple products) up to 18, and two points are compared: 2 * 18 * 11 * 2 = 792 <= 1024
// times eps max|x| / h.  The block knows no coordinates: R, its own extent in element sizes, stands for max|x| / h.  One
// element outside the bound makes the block general.  The result: one AffRec per element (FusedData::aff_rec).
// ---------------------------------------------------------------------------------------
constexpr double AFFINE_C = 1024.0;

static int affine_detect(hfx_eles *e, FusedData *F)
{
  F->affine = false;
  F->affine_tol = F->affine_spread = 0.0;
  F->aff_rec.reset();
  const int nd = e->n_dims, nq = nd * nd, nu = e->n_upts, nfp = e->n_fpts, npf = nfp / (2 * nd);
  const long ne = e->n_eles, plane_f = (long)nfp * ne;
  if (!e->JGinv_upts || !e->detjac_upts || !e->JGinv_fpts || !e->detjac_fpts || !e->tdA_fpts || !e->norm_fpts) return 0;
  std::vector<double> dju((size_t)nu * ne);
  HFX_HIP(hipMemcpy(dju.data(), e->detjac_upts, sizeof(double) * dju.size(), hipMemcpyDeviceToHost));
  double vol = 0.0;
  for (long el = 0; el < ne; el++) vol += std::fabs(dju[(size_t)nu * el]);
  const double eps = 2.220446049250313e-16;
  std::vector<double> recs((size_t)AffRec::SIZE * ne, 0.0);
  // the per-point arrays in chunks of elements (an element's values are contiguous in each; the normal has a plane per dimension)
  const long chunk = 2048;
  std::vector<double> jgu, jgf, djf, tda, nrm;
  double spread = 0.0, tol_max = 0.0;
  bool ok = true;
  for (long e0 = 0; e0 < ne; e0 += chunk)
  {
    const long nc = std::min(chunk, ne - e0);
    jgu.resize((size_t)nq * nu * nc); jgf.resize((size_t)nq * nfp * nc); djf.resize((size_t)nfp * nc);
    tda.resize((size_t)nfp * nc); nrm.resize((size_t)nfp * nc * nd);
    HFX_HIP(hipMemcpy(jgu.data(), e->JGinv_upts + (size_t)nq * nu * e0, sizeof(double) * jgu.size(), hipMemcpyDeviceToHost));
    HFX_HIP(hipMemcpy(jgf.data(), e->JGinv_fpts + (size_t)nq * nfp * e0, sizeof(double) * jgf.size(), hipMemcpyDeviceToHost));
    HFX_HIP(hipMemcpy(djf.data(), e->detjac_fpts + (size_t)nfp * e0, sizeof(double) * djf.size(), hipMemcpyDeviceToHost));
    HFX_HIP(hipMemcpy(tda.data(), e->tdA_fpts + (size_t)nfp * e0, sizeof(double) * tda.size(), hipMemcpyDeviceToHost));
    for (int m = 0; m < nd; m++)
      HFX_HIP(hipMemcpy(nrm.data() + (size_t)nfp * nc * m, e->norm_fpts + (size_t)nfp * e0 + m * plane_f, sizeof(double) * nfp * nc, hipMemcpyDeviceToHost));
    for (long c = 0; c < nc; c++)
    {
      const long el = e0 + c;
      double *r = &recs[(size_t)AffRec::SIZE * el];
      const double *ju = &jgu[(size_t)nq * nu * c], *jf = &jgf[(size_t)nq * nfp * c];
      const double dj = dju[(size_t)nu * el];
      double sj = 0.0;
      for (int q = 0; q < nq; q++)
      {
        r[AffRec::JG + q] = ju[q];
        sj = std::max(sj, std::fabs(ju[q]));
      }
      r[AffRec::DJ] = dj;
      if (!(std::fabs(dj) > 0.0) || !(sj > 0.0) || !(vol > 0.0)) { ok = false; continue; }
      const double tol = AFFINE_C * eps * (1.0 + std::pow(vol / std::fabs(dj), 1.0 / nd));
      tol_max = std::max(tol_max, tol);
      double worst = 0.0; // largest difference from the representative, in units of its scale
      auto see = [&](double diff, double scale) { worst = std::max(worst, std::fabs(diff) / scale); };
      for (int p = 0; p < nu; p++)
      {
        for (int q = 0; q < nq; q++) see(ju[(size_t)nq * p + q] - ju[q], sj);
        see(dju[(size_t)nu * el + p] - dj, std::fabs(dj));
      }
      for (int j = 0; j < nfp; j++)
      {
        for (int q = 0; q < nq; q++) see(jf[(size_t)nq * j + q] - ju[q], sj);
        see(djf[(size_t)nfp * c + j] - dj, std::fabs(dj));
        const int f = j / npf, j0 = f * npf;
        double *rf = r + AffRec::FACE + AffRec::FACE_W * f;
        const double t0 = tda[(size_t)nfp * c + j0];
        if (!(t0 > 0.0)) { worst = 1.0; continue; }
        for (int m = 0; m < nd; m++)
        {
          const double n0 = nrm[(size_t)nfp * nc * m + (size_t)nfp * c + j0];
          rf[m] = n0;
          see(nrm[(size_t)nfp * nc * m + (size_t)nfp * c + j] - n0, 1.0);
        }
        rf[AffRec::TDA] = t0;
        see(tda[(size_t)nfp * c + j] - t0, t0);
      }
      spread = std::max(spread, worst);
      if (!(worst <= tol)) ok = false; // (NaN included)
    }
  }
  F->affine_tol = tol_max;
  F->affine_spread = spread;
  if (!ok) return 0;
  if (F->aff_rec.upload(recs)) return 1;
  F->affine = true;
  return 0;
}

static int fused_build(hfx_eles *e, hfx_inters *const *faces, int nfb, bool allow_unpaired = false)
{
  HFX_CHECK(e->ele_type == 4 || e->ele_type == 1, "fused path: tensor-product elements only (hexes, quads)");
  const int N = tensor_n(e);
  HFX_CHECK(N >= 2 && N <= 8, "fused path: built for orders 1..7 (n_upts %d, n_fpts %d)", e->n_upts, e->n_fpts);
  const int nd = e->n_dims, nfp = e->n_fpts;
  // the registered operators must have the collocated tensor-product sparsity the kernels are sized for
  HFX_CHECK(e->opp_0.nnz_max <= N && e->opp_3.nnz_max <= 2 * nd, "fused path: opp_0 / opp_3 are not tensor-product sparse");
  for (int d = 0; d < nd; d++)
  {
    HFX_CHECK(e->opp_1[d].nnz_max <= N && e->opp_2[d].nnz_max <= N, "fused path: opp_1 / opp_2 are not tensor-product sparse");
    if (e->viscous_ops)
      HFX_CHECK(e->opp_4[d].nnz_max <= N && e->opp_5[d].nnz_max <= 2, "fused path: opp_4 / opp_5 are not tensor-product sparse");
  }
  if (e->viscous_ops) HFX_CHECK(e->opp_6.nnz_max <= N, "fused path: opp_6 is not tensor-product sparse");
  HFX_CHECK(!e->ctx->params.viscous || e->viscous_ops, "fused path: viscous run but the block has no opp_4/5/6");
  // (the packed row entries: 8-bit columns up to 256 points per element, 16-bit ones above -- Geo::WIDE, checked in pack_rows)
  HFX_CHECK(e->n_upts < 65536 && e->n_fpts < 65536, "fused path: column indices must fit 16 bits");

  if (!e->fused) e->fused.reset(new FusedData());
  FusedData *F = e->fused.get();

  // opp_1 merged over the dimension slabs (row k of opp_1[d] is l_j(fpt_k) * tnorm(d,k): one d per row)
  {
    std::vector<double> mv((size_t)nfp * N, 0.0);
    std::vector<int> mi((size_t)nfp * N, 0), md(nfp, 0);
    for (int r = 0; r < nfp; r++)
    {
      int dsel = -1;
      for (int d = 0; d < nd; d++)
      {
        const Operator &op = e->opp_1[d];
        const int w = std::max(op.nnz_max, 1);
        bool any = false;
        for (int q = 0; q < w; q++) any = any || (op.h_val[r + (size_t)nfp * q] != 0.0);
        if (any)
        {
          HFX_CHECK(dsel < 0, "fused path: row %d of opp_1 has entries in two dimension slabs", r);
          dsel = d;
        }
      }
      if (dsel < 0) dsel = 0;
      const Operator &op = e->opp_1[dsel];
      const int w = std::max(op.nnz_max, 1);
      md[r] = dsel;
      for (int q = 0; q < N; q++)
      {
        mv[r + (size_t)nfp * q] = (q < w) ? op.h_val[r + (size_t)nfp * q] : 0.0;
        mi[r + (size_t)nfp * q] = (q < w) ? op.h_idx[r + (size_t)nfp * q] : op.h_idx[r];
      }
    }
    if (F->o1m_dim.upload(md)) return 1;
    if (dispatch_build_packed(e, F, N, mv, mi)) return 1;
    // (the sum-factorised tables serve variant 3 only: not built for the sizes it does not fit)
    F->tensor_ok = false;
    if (split3_fits_rt(nd, N) && tensor_build(e, F, N, mv, mi, md)) return 1;
  }
  // (whatever kernels the block runs: split_plan decides which of them read the record)
  if (affine_detect(e, F)) return 1;

  const long plane_f = (long)e->n_fpts * e->n_eles;
  std::vector<char> paired(plane_f, 0);
  std::vector<unsigned char> meta(plane_f, 0);
  std::vector<double> norm((size_t)plane_f * nd);
  HFX_HIP(hipMemcpy(norm.data(), e->norm_fpts, sizeof(double) * norm.size(), hipMemcpyDeviceToHost));
  for (int b = 0; b < nfb; b++)
  {
    hfx_inters *f = faces[b];
    if (f->is_bdy)
    {
      // boundary points: one-sided kernels; bit2 asks the flux kernel to store the gradient there
      HFX_CHECK(f->left == e, "fused path: boundary block of another element block");
      for (size_t q = 0; q < f->hL.size(); q++)
      {
        paired[f->hL[q]] = 1;
        meta[f->hL[q]] |= 4;
      }
      continue;
    }
    HFX_CHECK(f->left == e && f->right == e, "fused path: face blocks must connect the element block to itself");
    const long np = (long)f->n_inters * f->n_fpts_per_inter;
    for (long q = 0; q < np; q++)
    {
      const int il = f->hL[q], ir = f->hR[q];
      paired[il] = paired[ir] = 1;
      // the consistent switch of src/inters.cpp:568-581 on the LEFT normal (exact zero tests);
      // only the sign decision is stored
      const double n[3] = {norm[il], norm[il + plane_f], nd == 3 ? norm[il + 2 * plane_f] : 0.0};
      const double n2[2] = {n[0], n[1]};
      const unsigned char flip = ((nd == 3 ? ldg_switch<3>(1.0, n) : ldg_switch<2>(1.0, n2)) < 0) ? 2 : 0;
      meta[il] = flip;
      meta[ir] = flip | 1;
    }
  }
  if (!allow_unpaired)
    for (long o = 0; o < plane_f; o++)
      HFX_CHECK(paired[o], "fused path: flux point %ld belongs to no registered face (partition faces need "
                           "hfx_stage_partitioned / hfx_run_steps_partitioned)", o);
  F->upd_list_b.reset();
  F->upd_list_i.reset();
  F->n_list_b = F->n_list_i = 0;
  if (allow_unpaired)
  {
    // the elements with a partition-face point, and the others (split update launch of hfx_run_steps_partitioned)
    std::vector<int> lb, li;
    for (int el = 0; el < e->n_eles; el++)
    {
      bool any = false;
      for (int j = 0; j < nfp && !any; j++) any = !paired[(long)nfp * el + j];
      (any ? lb : li).push_back(el);
    }
    F->n_list_b = (long)lb.size();
    F->n_list_i = (long)li.size();
    F->n_list_i1 = F->n_list_i / 2;
    if (!lb.empty() && F->upd_list_b.upload(lb)) return 1;
    if (!li.empty() && F->upd_list_i.upload(li)) return 1;
  }
  if (F->meta.upload(meta)) return 1;
  {
    // partner of every interior flux point for the flux kernel that forms the LDG corrections itself:
    // (partner offset << 2) | beta-sign flipped << 1 | this point is the right side;  -1: boundary or partition-face point
    std::vector<int> nbr(plane_f, -1);
    bool fits = plane_f < (1L << 29);
    F->n_interior_fpts = 0;
    for (int b = 0; b < nfb; b++)
      if (!faces[b]->is_bdy) F->n_interior_fpts += 2L * faces[b]->n_inters * faces[b]->n_fpts_per_inter;
    for (int b = 0; b < nfb && fits; b++)
    {
      hfx_inters *f = faces[b];
      if (f->is_bdy) continue;
      const long np = (long)f->n_inters * f->n_fpts_per_inter;
      for (long q = 0; q < np; q++)
      {
        const int il = f->hL[q], ir = f->hR[q];
        nbr[il] = (ir << 2) | (meta[il] & 2);
        nbr[ir] = (il << 2) | (meta[il] & 2) | 1;
      }
    }
    F->nbr.reset();
    if (fits && F->nbr.upload(nbr)) return 1;
    // two-wave flux kernel: what every local face's would-be left-over points ask of Fn (FusedData::tw_need)
    F->tw_counted = false;
    const int n_left = nfp - 128, npf = nfp / (2 * nd);
    if (fits && nd == 3 && n_left > 0 && n_left <= npf)
    {
      for (auto &row : F->tw_need)
        for (long &c : row) c = 0;
      for (long el = 0; el < e->n_eles; el++)
        for (int face = 0; face < 2 * nd; face++)
        {
          int code = 0;
          for (int j = 0; j < n_left; j++)
          {
            const int nb = nbr[(long)nfp * el + npf * face + j];
            // weight of this side's Fn: 1/2 + beta on the pair's left side, 1/2 - beta on its right, beta's sign flipped with bit1
            code |= nb < 0 ? 1 : ((((nb & 1) ^ ((nb >> 1) & 1)) == 0) ? 2 : 4);
          }
          F->tw_need[face][code]++;
        }
      F->tw_counted = true;
    }
  }
  if (F->disu_alt.ensure((size_t)plane_f * e->n_fields)) return 1;
  F->built = true;
  return 0;
}

// workgroups of a persistent (grid-stride over elements) kernel that are resident on one CU at once -- registers and LDS
// decide.  A grid of exactly that many per CU has no workgroup waiting for a slot: with more, the late ones start when
// the others are part way through their elements and finish as a tail (LES residual kernel: five resident, 0.70 ms at
// five per CU, 1.00 ms at six, 0.81 ms at sixteen).
template <auto KERNEL>
static int resident_per_cu(int threads)
{
  static int n = 0;
  if (n == 0)
  {
    int q = 0;
    n = (hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, KERNEL, threads, 0) == hipSuccess && q > 0) ? q : 1;
  }
  return n;
}

// workgroups of a persistent element kernel: the resident ones, or `per_cu` of them per CU when the option asks -- what a
// launcher hands to persistent_grid (hfx_internal.hpp), which every launch's grid comes from.  `cap`:
// the streaming update kernel is fastest at three workgroups per CU (0.27 ms; 0.35 ms at the four that are resident, 0.29 ms
// at sixteen)
template <auto KERNEL>
static int element_grid(const hfx_eles *e, int threads, int per_cu, int cap = 1 << 30)
{
  const int pc = per_cu > 0 ? per_cu : std::min(cap, resident_per_cu<KERNEL>(threads));
  return (int)std::min<long>(e->n_eles, (long)e->ctx->n_cu * pc);
}

// launch of the loader-wave form, instantiated only for element sizes it fits (loader_wave_fits)
template <int ND, int N, bool OI, bool GA, bool LES, bool FITS, bool AFF = false>
struct LoaderWaveLaunch
{
  static void go(const hfx_eles *, int, hipStream_t, const Split2Args &, const double *, const int *) {}
};
template <int ND, int N, bool OI, bool GA, bool LES, bool AFF>
struct LoaderWaveLaunch<ND, N, OI, GA, LES, true, AFF>
{
  static void go(const hfx_eles *e, int per_cu, hipStream_t st, const Split2Args &e2, const double *coef, const int *idx)
  {
    constexpr int TB = SGeo<ND, N>::TB + 64;
    // (the over-integration form measured 3 % faster at sixteen workgroups per CU than at the two that are resident)
    if (OI && per_cu == 0) per_cu = 16;
    int grid = element_grid<split_flux_tensor_kernel<ND, N, 2, true, OI, true, GA, LES, AFF>>(e, TB, per_cu);
    if (e2.ele_list != nullptr) grid = (int)std::max<long>(1, std::min<long>(grid, e2.n_list));
    grid = persistent_grid(e, SLOT_ELEMENT, e2.ele_list != nullptr ? e2.n_list : (long)e->n_eles, grid);
    hipLaunchKernelGGL((split_flux_tensor_kernel<ND, N, 2, true, OI, true, GA, LES, AFF>), dim3(grid), dim3(TB), 0, st, e2, coef, idx);
  }
};

// Two-wave flux kernel: how many elements of the block need the projected viscous flux of one of the left-over points when these
// lie on local face f (need[f], from the partner words counted in fused_build and the run's ldg_beta: the kernel's own test of
// `needed`), and the face that asks least often (the lowest of equals) -- the left-over points go there
static int two_wave_face(const FusedData *F, double ldg_beta, long need[6], int forced = -1)
{
  int best = 0;
  for (int f = 0; f < 6; f++)
  {
    need[f] = 0;
    for (int code = 1; code < 8; code++)
      if ((code & 1) || ((code & 2) && 0.5 + ldg_beta != 0.0) || ((code & 4) && 0.5 - ldg_beta != 0.0)) need[f] += F->tw_need[f][code];
    if (need[f] < need[best]) best = f;
  }
  return forced >= 0 ? forced : best; // (option flux_two_wave_face)
}

// launch of the two-wave form, instantiated only for the element size it is written for (TwoWave::fits)
template <int ND, int N, bool FITS>
struct TwoWaveLaunch
{
  static void go(const hfx_eles *, int, hipStream_t, const Split2Args &, const double *, const int *, int) {}
  static void go_fold(const hfx_eles *, int, hipStream_t, const Split2Args &, const double *, const int *, int) {}
};
template <int ND, int N>
struct TwoWaveLaunch<ND, N, true>
{
  static void go(const hfx_eles *e, int per_cu, hipStream_t st, const Split2Args &e2, const double *coef, const int *idx, int face)
  {
    launch<false, 0>(e, per_cu, st, e2, coef, idx, face);
  }
  // the FOLD form (SplitPlan::fold_faces) with the run's Riemann solver: Rusanov, or HLLC as with_riemann_solver maps the others
  // (the plan does not fold a RoeM run)
  static void go_fold(const hfx_eles *e, int per_cu, hipStream_t st, const Split2Args &e2, const double *coef, const int *idx, int face)
  {
    e2.P.riemann == 0 ? launch<true, 0>(e, per_cu, st, e2, coef, idx, face) : launch<true, 3>(e, per_cu, st, e2, coef, idx, face);
  }
  template <bool FOLD, int RS>
  static void launch(const hfx_eles *e, int per_cu, hipStream_t st, const Split2Args &e2, const double *coef, const int *idx, int face)
  {
    constexpr int TB = TwoWave<ND, N>::TB;
    int grid = element_grid<split_flux_two_wave_kernel<ND, N, FOLD, RS>>(e, TB, per_cu);
    if (e2.ele_list != nullptr) grid = (int)std::max<long>(1, std::min<long>(grid, e2.n_list));
    grid = persistent_grid(e, SLOT_ELEMENT, e2.ele_list != nullptr ? e2.n_list : (long)e->n_eles, grid);
    hipLaunchKernelGGL((split_flux_two_wave_kernel<ND, N, FOLD, RS>), dim3(grid), dim3(TB), 0, st, e2, coef, idx, TwoWave<ND, N>::rotation(face));
  }
};
static bool two_wave_fits_rt(int nd, int N)
{
  return nd == 3 && N == 5 && TwoWave<3, 5>::fits;
}

// The squared length scale of the eddy-viscosity closures at every solution point (les_len2_upload, hfx.hip): the flux kernel
// reads it instead of evaluating a cube root per point and stage.
static int les_len2_build(hfx_eles *e)
{
  FusedData *F = e->fused.get();
  if (F->les_len2) return 0;
  return les_len2_upload(e, F->les_len2);
}

// What the split stage runs on this block when `requested_variant` is asked for (SplitPlan): from the options, the block's fused
// tables (fused_build; without them no sum-factorised form is planned), its flags and array sizes, its face blocks.
SplitPlan split_plan(const hfx_eles *e, hfx_inters *const *faces, int nfb, int requested_variant)
{
  const hfx_ctx::Options &opt = e->ctx->opt;
  const FusedData *F = (e->fused && e->fused->built) ? e->fused.get() : nullptr;
  const bool viscous = e->ctx->params.viscous != 0, oi = e->over_int_ready;
  const int N = tensor_n(e);
  // the sum-factorised kernels, and the options and element size of their loader-wave form
  const bool tensor = F && F->tensor_ok && !opt.dictionary_rows;
  const bool lw_form = tensor && loader_wave_fits_rt(e->n_dims, N) && opt.loader_wave && opt.buffer_addressing && opt.flux_waves == 2;
  bool any_bdy = false;
  for (int b = 0; b < nfb; b++) any_bdy = any_bdy || faces[b]->is_bdy;
  SplitPlan p;
  p.bdy_grad = any_bdy && viscous;

  // Every array a launch touches below 4 GiB (32-bit byte offsets), each test with its own count of the largest array: the
  // metric tensors, the n_fields * n_dims gradient-sized arrays when in use, the de-aliased flux -- over both point sets
  // (quads with N >= 5 have more solution points than flux points).
  auto below_4gib = [](double doubles) { return doubles * 8.0 < 4294967296.0; };
  const double plane_most = (double)std::max<long>((long)e->n_fpts * e->n_eles, (long)e->n_upts * e->n_eles);
  auto most = [&](bool grad) {
    double m = plane_most * std::max(e->n_dims * e->n_dims, e->n_fields);
    if (grad) m = std::max(m, plane_most * e->n_fields * e->n_dims);
    if (oi) m = std::max(m, (double)e->n_upts * e->n_eles * e->n_fields * e->n_dims);
    return m;
  };
  // LES in the flux kernel: the gradient-sized arrays always (a boundary block makes it store the flux-point gradient)
  p.les_fits_4gib = below_4gib(plane_most * e->n_fields * e->n_dims);
  // LDG corrections in the flux kernel: the gradient-sized arrays with any boundary face
  p.gather_fits_4gib = below_4gib(most(any_bdy));
  // buffer addressing of the flux kernel: the gradient-sized arrays with a boundary face on a viscous block
  p.flux_buf_fits_4gib = below_4gib(most(p.bdy_grad));
  // buffer addressing of the update kernel: the n_fields arrays
  p.update_fits_4gib = below_4gib(plane_most * e->n_fields);

  // The variant: 3 falls back to 2 where its kernels do not fit the element size (split3_fits: hexes from P6 on) and where an
  // LES closure cannot be evaluated in its flux kernel (its loader-wave form only); variant 2 keeps the gradient in HBM.
  p.les_in_flux = e->les_ready && viscous && !oi && opt.les_flux_kernel && lw_form && p.les_fits_4gib;
  p.variant = requested_variant;
  if (requested_variant == 3 && (!split3_fits_rt(e->n_dims, N) || (e->les_ready && !p.les_in_flux))) p.variant = 2;
  const bool v3 = p.variant == 3;

  // Over-integration (src/solver.cpp:82-91): the loader-wave flux kernel takes the sum-factorised kernel's result folded into
  // the divergence; a de-aliased flux that arrives whole (unfolded, dense) goes to the register pipeline.
  const bool oi_tensor = tensor_over_int_available(e) && e->ctx->contract_mode != HFX_CONTRACT_DENSE;
  const bool oi_fold_ok = !oi || (opt.over_int_fold && oi_tensor);
  p.oi_fold = v3 && oi && lw_form && oi_fold_ok;
  if (v3 && oi) p.over_int = p.oi_fold ? OverInt::folded_tensor : oi_tensor ? OverInt::tensor : OverInt::dense;

  // The LDG corrections of the interior points: formed by the loader-wave flux kernel itself, or by face_delta_kernel
  p.gather = v3 && viscous && opt.gather_delta && F && F->nbr && lw_form && oi_fold_ok && p.gather_fits_4gib;
  p.face_delta = viscous && !p.gather;

  // The flux kernel.  (les: a closure with an SGS flux -- every model but the spectral vanishing viscosity, a filter)
  p.flux = !tensor ? FluxForm::dictionary_rows
           : (lw_form && oi_fold_ok && p.flux_buf_fits_4gib) ? FluxForm::loader_wave : FluxForm::register_pipeline;
  p.oi = oi;
  p.les = e->les_ready && e->les.sgs_model != 3;
  p.buf = opt.buffer_addressing && p.flux_buf_fits_4gib;
  p.wv = (p.flux == FluxForm::register_pipeline && !oi && p.buf && opt.flux_waves != 2) ? 3 : 2;
  p.update_buf = opt.buffer_addressing && p.update_fits_4gib;
  // An affine block: the default form of the flux kernel (loader wave, corrections formed in the kernel, no over-integration, no
  // LES closure) has an AFF instantiation for every element size the loader wave fits; the update kernel follows it.
  // Every other form keeps the per-point metrics.
  p.affine = v3 && F && F->affine && opt.affine_metrics && p.flux == FluxForm::loader_wave && p.gather && !oi && !p.les;
  // ... and on P4 hexahedra, whose loader-wave form has four waves, the affine form runs as two-wave workgroups
  p.two_wave = p.affine && opt.flux_two_wave && two_wave_fits_rt(e->n_dims, N) && F->tw_counted;
  // ... and with one-sided LDG (one weight of every pair exactly 0.0: ldg_both_sides, face_physics.hpp) it forms the interior
  // pairs' common flux itself
  {
    const double b = e->ctx->params.ldg_beta;
    const bool one_sided = (0.5 + b) == 0.0 || (0.5 - b) == 0.0;
    // (not with RoeM: pow() in its dissipation costs the FOLD form 34 spilled registers, and at supersonic face states its last-bit
    // differences from the face kernel's inlining take the residual past the oracle's bound -- that solver keeps the face kernel)
    p.fold_faces = p.two_wave && viscous && one_sided && opt.fold_faces && e->ctx->params.riemann_solve_type != 2;
  }

  // a partitioned block: variant 3 sends the projected viscous flux; element lists for the flux kernel without over-integration
  // (which runs on all elements first), for the update without shock capturing (whose filter follows the whole update)
  p.projected = v3;
  p.split_flux = v3 && !oi;
  p.split_update = v3 && !e->shock_ready;

  p.names = v3 ? (tensor ? "face_delta_kernel,split_flux_tensor_kernel,face_flux2_kernel,split_update_kernel"
                         : "face_delta_kernel,split_flux_kernel,face_flux2_kernel,split_update_kernel")
               : "face_delta_kernel,split_gradient_kernel,face_flux_kernel,split_residual_kernel";
  if (p.over_int != OverInt::none)
    p.extra_names = p.over_int == OverInt::dense ? ",evaluate_invFlux_over_int (dense)" : ",overint_tensor_kernel";
  else if (p.variant == 2 && e->les_ready && viscous)
    p.extra_names = ",sgsf_upts_kernel + ell_apply_kernel (SGS flux)";
  else if (F && F->affine)
    // (no launch of its own: the flux and update kernels read the per-element metric record | the block was found affine, but the form
    // that runs keeps the per-point metrics)
    p.extra_names = p.fold_faces ? ",affine_metrics,two_wave,folded_faces" : p.two_wave ? ",affine_metrics,two_wave" : p.affine ? ",affine_metrics" : ",affine_block";
  return p;
}

int split_stage_plan(const hfx_eles *e, hfx_inters *const *faces, int nfb, int requested_variant, SplitPlan *pl)
{
  *pl = split_plan(e, faces, nfb, requested_variant);
  HFX_CHECK(!e->over_int_ready || pl->variant == 3,
            "the split variant that keeps the gradients (fused 2, which LES without the in-kernel closure selects) has no over-integration");
  return 0;
}

// what the element kernels of both variants take alike: geometry, state, the RK coefficients of this stage
template <class Args>
static void stage_args(Args &a, const hfx_eles *e, int in_step, bool write_div)
{
  const hfx_params &p = e->ctx->params;
  a.n_eles = e->n_eles;
  a.o1m_dim = e->fused->o1m_dim;
  a.detjac_upts = e->detjac_upts; a.JGinv_upts = e->JGinv_upts;
  a.detjac_fpts = e->detjac_fpts; a.JGinv_fpts = e->JGinv_fpts;
  a.u0 = e->arr[HFX_DISU_UPTS0]; a.u1 = e->arr[HFX_DISU_UPTS1];
  a.delta = e->arr[HFX_DELTA_DISU_FPTS]; a.tconf = e->arr[HFX_NORM_TCONF_FPTS];
  a.disu_next = e->fused->disu_alt;
  a.src = e->src_nonzero ? e->arr[HFX_SRC_UPTS] : nullptr;
  a.dt_local = e->arr[HFX_DT_LOCAL];
  a.nan_flag = e->nan_flag;
  a.P = e->ctx->phys();
  a.adv_type = p.adv_type; a.in_step = in_step; a.dt_local_on = p.dt_type == 2; a.dt = p.dt;
  a.rk_a = (p.adv_type >= 3) ? p.RK_a[in_step] : 0.0;
  a.rk_b = (p.adv_type >= 3) ? p.RK_b[in_step] : 0.0;
  // (low-storage schemes: a stage whose RK_a is 0.0 -- the first of a step -- takes 0.0 for the register instead of reading it)
  a.need_u1 = (p.adv_type >= 3 && a.rk_a != 0.0) || (p.adv_type == 1 && in_step == 3) || (p.adv_type == 2 && in_step == 2);
  a.write_div = write_div ? 1 : 0;
}

// the pairs of one interior-face block for a pairwise kernel; false: none
static bool face_pairs(FacePairArgs &a, const hfx_inters *f)
{
  a.npairs = (long)f->n_inters * f->n_fpts_per_inter;
  a.L = f->L; a.R = f->R;
  return a.npairs > 0;
}

// Over-integration folded into the divergence (src/solver.cpp:82-91): the sum-factorised kernel hands the loader-wave flux kernel
// sum_l Dc[l] tdisf_l -- the de-aliased flux's whole contribution to (div_tdisf - opp_3 norm_tdisf), n_fields values per solution
// point (tensor_ops.hip).  Dc[d] = D - c3[d][0] (L1 Lf)[d][0]^T - c3[d][1] (L1 Lf)[d][1]^T, as the flux kernel's prologue forms
// it (split3_kernels.hpp), from the host copy of the tensor-product tables
template <int ND, int N>
static std::vector<double> over_int_fold_matrices(const std::vector<double> &c)
{
  using T = TGeo<ND, N>;
  std::vector<double> Dc((size_t)ND * N * N);
  for (int d = 0; d < ND; d++)
    for (int mp = 0; mp < N; mp++)
      for (int m = 0; m < N; m++)
      {
        const double ta = c[T::C_3 + (d * 2 + 0) * N + mp] * (c[T::C_L1 + (d * 2 + 0) * N] * c[T::C_LF + (d * 2 + 0) * N + m]);
        const double tb = c[T::C_3 + (d * 2 + 1) * N + mp] * (c[T::C_L1 + (d * 2 + 1) * N] * c[T::C_LF + (d * 2 + 1) * N + m]);
        Dc[((size_t)d * N + mp) * N + m] = c[T::C_D + mp * N + m] - ta - tb;
      }
  return Dc;
}

// SplitStage for one element size: the arguments and the launches
template <int ND, int N>
struct SplitStageT final : SplitStage
{
  static constexpr int TB = SGeo<ND, N>::TB;
  // variant 3's element kernels exist for the sizes they fit only (split3_fits); split_plan sends the others to variant 2
  static constexpr bool V3 = split3_fits<ND, N>();
  FusedData *const F = e->fused.get();
  const hipStream_t st = e->ctx->stream;
  const Phys P = e->ctx->phys();
  // persistent grids: split_grid_per_cu workgroups per CU, 0 = as many as are resident (element_grid)
  const int per_cu = e->ctx->opt.split_grid_per_cu;
  const int flux_per_cu = e->ctx->opt.flux_grid_per_cu > 0 ? e->ctx->opt.flux_grid_per_cu : per_cu;
  Split2Args e2{};      // variant 3
  SplitEleArgs ea{};    // variant 2
  FacePairArgs fa{};    // the pairwise kernels: the block's arrays on both sides, all but a face block's pairs (face_pairs)
  SplitStageT(hfx_eles *e_, hfx_inters *const *faces_, int nfb_, const SplitPlan &pl_) : SplitStage(e_, faces_, nfb_, pl_) {}

  int init(int in_step, bool write_div) override
  {
    HFX_CHECK(V3 || pl.variant == 2, "split variant 3 does not fit %d-D elements with %d points per direction: run variant 2", ND, N);
    const long plane_f = (long)e->n_fpts * e->n_eles;
    FaceSide s{};
    s.plane = plane_f;
    s.disu = e->arr[HFX_DISU_FPTS]; s.grad = e->arr[HFX_GRAD_DISU_FPTS]; s.tdA = e->tdA_fpts;
    s.delta = e->arr[HFX_DELTA_DISU_FPTS]; s.tconf = e->arr[HFX_NORM_TCONF_FPTS];
    // (variant 2: the SGS flux at the flux points arrives in reference space)
    s.sgsf = (e->les_ready && pl.variant == 2) ? e->arr[HFX_SGSF_FPTS] : nullptr;
    s.jac = e->Jacobian_fpts; s.detjac = e->detjac_fpts;
    fa.meta = F->meta; fa.norm = e->norm_fpts;
    fa.l = fa.r = s;
    if (pl.variant == 2)
    {
      stage_args(ea, e, in_step, write_div);
      ea.grad_upts = e->arr[HFX_GRAD_DISU_UPTS]; ea.grad_fpts = e->arr[HFX_GRAD_DISU_FPTS];
      ea.div_out = e->arr[HFX_DIV_TCONF_UPTS];
      ea.sgsf_upts = e->les_ready ? e->arr[HFX_SGSF_UPTS].get() : nullptr;
      return 0;
    }
    const hfx_ctx::Options &opt = e->ctx->opt;
    if (opt.flux_stamps && F->stamps.ensure_zeroed(16 * 16)) return 1; // (a row of 16 per wave: room for every workgroup size)
    if (F->fn_fpts.ensure((size_t)plane_f * e->n_fields)) return 1;
    if (pl.les && les_len2_build(e)) return 1;
    if (pl.oi_fold && !tensor_over_int_folded(e) && tensor_over_int_set_fold(e, over_int_fold_matrices<ND, N>(F->h_coef).data())) return 1;
    stage_args(e2, e, in_step, write_div);
    e2.xcd_order = opt.xcd_order ? 1 : 0;
    e2.pk_g = F->pk_g; e2.pk_r = F->pk_r; e2.tab_g = F->tab_g; e2.tab_r = F->tab_r;
    e2.norm_fpts = e->norm_fpts;
    e2.fn_fpts = F->fn_fpts; e2.ntd_fpts = e->arr[HFX_NORM_TDISF_FPTS]; e2.div = e->arr[HFX_DIV_TCONF_UPTS];
    e2.folded = pl.flux != FluxForm::dictionary_rows ? 1 : 0;
    e2.grad_upts = nullptr;
    e2.grad_fpts = pl.bdy_grad ? e->arr[HFX_GRAD_DISU_FPTS] : nullptr; // boundary points only
    // polynomial de-aliasing: tdisf_upts = over_int_filter . F(opp_over_int_cubpts . u), or its folded form (over_int)
    e2.tdisf_in = e->over_int_ready ? e->arr[HFX_TDISF_UPTS] : nullptr;
    e2.meta = F->meta;
    e2.stamps = F->stamps;
    e2.stamp_it = std::max(2, opt.flux_stamps);
    e2.simd_roles = opt.simd_roles ? 1 : 0;
    e2.light_short = opt.light_wave_short ? 1 : 0;
    e2.o3v = e->opp_3.ell_val; e2.o3i = e->opp_3.ell_idx; e2.o3w = std::max(e->opp_3.nnz_max, 1);
    e2.o0v = e->opp_0.ell_val; e2.o0i = e->opp_0.ell_idx; e2.o0w = std::max(e->opp_0.nnz_max, 1);
    e2.les = e->les; e2.tdA_fpts = e->tdA_fpts;
    e2.les_len2 = F->les_len2;
    e2.nbr = pl.gather ? F->nbr.get() : nullptr;
    e2.disu = e->arr[HFX_DISU_FPTS];
    e2.aff_rec = pl.affine ? F->aff_rec.get() : nullptr;
    fa.l.fn = fa.r.fn = F->fn_fpts;
    return 0;
  }

  int ldg() override
  {
    if (!P.viscous) return 0;
    for (int b = 0; b < nfb; b++)
    {
      if (faces[b]->is_bdy)
      {
        // ghost state -> inviscid common flux and LDG common solution of the boundary points
        if (hfx_bdy_launch_internal(faces[b], 0, 1)) return 1;
        continue;
      }
      if (!pl.face_delta) continue; // (the flux kernel reads the partner's flux-point solution itself)
      if (!face_pairs(fa, faces[b])) continue;
      hipLaunchKernelGGL((face_delta_kernel<ND>), dim3((unsigned)((fa.npairs + 255) / 256)), dim3(256), 0, st, fa, P);
    }
    HFX_HIP(hipGetLastError());
    return 0;
  }

  // grid of the element kernel KERNEL on all elements, or on the list the step was given (the workgroups past its end find no work)
  template <auto KERNEL>
  int flux_grid() const
  {
    return persistent_grid(e, SLOT_ELEMENT, e2.ele_list != nullptr ? e2.n_list : (long)e->n_eles, element_grid<KERNEL>(e, TB, per_cu));
  }

  // the loader-wave form with the plan's flags (instantiated only for the sizes it fits)
  template <bool OI, bool LES>
  void loader_wave()
  {
    constexpr bool fits = loader_wave_fits<ND, N>();
    static_assert(!fits || loader_wave_fits<ND, N, true>(), "the affine form fits wherever the loader wave does");
    if (pl.two_wave)
    {
      long need[6];
      if constexpr (!OI && !LES)
      {
        const int face = two_wave_face(F, P.ldg_beta, need, e->ctx->opt.flux_two_wave_face);
        using Launch = TwoWaveLaunch<ND, N, TwoWave<ND, N>::fits>;
        pl.fold_faces ? Launch::go_fold(e, flux_per_cu, st, e2, F->t_coef, F->t_idx, face) : Launch::go(e, flux_per_cu, st, e2, F->t_coef, F->t_idx, face);
      }
    }
    else if (pl.affine)
    {
      if constexpr (!OI && !LES) LoaderWaveLaunch<ND, N, false, true, false, fits, true>::go(e, flux_per_cu, st, e2, F->t_coef, F->t_idx);
    }
    else if (pl.gather)
      LoaderWaveLaunch<ND, N, OI, true, LES, fits>::go(e, flux_per_cu, st, e2, F->t_coef, F->t_idx);
    else
      LoaderWaveLaunch<ND, N, OI, false, LES, fits>::go(e, flux_per_cu, st, e2, F->t_coef, F->t_idx);
  }
  template <int WV, bool BUF, bool OI>
  void register_pipeline()
  {
    hipLaunchKernelGGL((split_flux_tensor_kernel<ND, N, WV, BUF, OI, false>), dim3(flux_grid<split_flux_tensor_kernel<ND, N, WV, BUF, OI, false>>()),
                       dim3(TB), 0, st, e2, F->t_coef, F->t_idx);
  }

  // (partitioned blocks: the solution exchange runs beside the launch on interior_1, the exchange of the projected fluxes
  // beside the one on interior_2)
  int flux_kernel(EleList list) override
  {
    HFX_CHECK(pl.variant == 3, "split stage: the flux kernel is a step of variant 3");
    if constexpr (V3)
    {
      const bool listed = elements(list, e2.ele_list, e2.n_list);
      if (listed && e2.n_list == 0) return 0;
      HFX_CHECK(!listed || (e2.ele_list != nullptr && !e->over_int_ready), "split flux kernel on element lists: no lists, or over-integration (which runs on all elements first)");
      HFX_CHECK(!pl.oi_fold || pl.flux == FluxForm::loader_wave, "over-integration: the folded form needs the loader-wave flux kernel");
      HFX_CHECK(!pl.affine || (e2.aff_rec != nullptr && pl.flux == FluxForm::loader_wave && pl.gather && !pl.oi && !pl.les),
                "split stage: the affine-metric form needs the block's metric records and the default loader-wave flux kernel");
      HFX_CHECK(!pl.les || (pl.flux == FluxForm::loader_wave && !pl.oi && P.viscous),
                "split variant 3 with an LES closure needs the loader-wave flux kernel (SplitPlan::les_in_flux): run variant 2");
      switch (pl.flux)
      {
      case FluxForm::loader_wave:
        if (pl.les)
          loader_wave<false, true>();
        else if (pl.oi)
          loader_wave<true, false>();
        else
          loader_wave<false, false>();
        break;
      case FluxForm::register_pipeline:
        if (pl.wv == 3)
          register_pipeline<3, true, false>();
        else if (pl.buf && pl.oi)
          register_pipeline<2, true, true>();
        else if (pl.oi)
          register_pipeline<2, false, true>();
        else if (pl.buf)
          register_pipeline<2, true, false>();
        else
          register_pipeline<2, false, false>();
        break;
      case FluxForm::dictionary_rows:
        hipLaunchKernelGGL((split_flux_kernel<ND, N>), dim3(flux_grid<split_flux_kernel<ND, N>>()), dim3(TB), 0, st, e2);
        break;
      }
      HFX_HIP(hipGetLastError());
    }
    return 0;
  }

  int gradient_kernel() override
  {
    HFX_CHECK(pl.variant == 2, "split stage: the gradient kernel is a step of variant 2");
    if (!P.viscous) return 0;
    ea.pk = F->pk_g;
    ea.tab = F->tab_g;
    hipLaunchKernelGGL((split_gradient_kernel<ND, N>), dim3(persistent_grid(e, SLOT_ELEMENT, e->n_eles, element_grid<split_gradient_kernel<ND, N>>(e, TB, per_cu))), dim3(TB), 0, st, ea);
    HFX_HIP(hipGetLastError());
    return 0;
  }

  int common_fluxes() override
  {
    // boundary faces on the side stream, beside the pairwise interior-face kernel: both need the flux kernel's results and
    // write norm_tconf at disjoint points
    bool any_bdy_faces = false;
    for (int b = 0; b < nfb; b++) any_bdy_faces = any_bdy_faces || (faces[b]->is_bdy && faces[b]->n_inters > 0);
    const bool beside = any_bdy_faces && e->ctx->opt.bdy_beside;
    if (beside && side_stream_fork(e->ctx)) return 1;
    for (int b = 0; b < nfb; b++)
      if (faces[b]->is_bdy && hfx_bdy_launch_internal(faces[b], P.viscous ? 1 : 0, 1)) return 1;
    if (beside && side_stream_join(e->ctx)) return 1;
    for (int b = 0; b < nfb; b++)
    {
      if (faces[b]->is_bdy || !face_pairs(fa, faces[b])) continue;
      if (pl.fold_faces) continue; // (the two-wave flux kernel has written the interior pairs' norm_tconf)
      const dim3 nb((unsigned)((fa.npairs + 255) / 256));
      if (pl.variant == 3)
        with_riemann_solver(P.riemann, [&](auto RS) { hipLaunchKernelGGL((face_flux2_kernel<ND, decltype(RS)::value>), nb, dim3(256), 0, st, FaceBlockArgs(fa), P); });
      else
        with_riemann_solver(P.riemann, [&](auto RS) { hipLaunchKernelGGL((face_flux_kernel<ND, decltype(RS)::value>), nb, dim3(256), 0, st, fa, P); });
    }
    if (beside && side_stream_wait(e->ctx)) return 1;
    HFX_HIP(hipGetLastError());
    return 0;
  }

  template <bool BUF>
  void update_launch(long n_work)
  {
    // (the streaming update kernel is fastest at three workgroups per CU: element_grid)
    const int g = persistent_grid(e, SLOT_UPDATE, n_work, std::min<long>(n_work, element_grid<split_update_kernel<ND, N, BUF>>(e, TB, per_cu, 3)));
    hipLaunchKernelGGL((split_update_kernel<ND, N, BUF>), dim3(g), dim3(TB), 0, st, e2);
  }

  // The buffers of disu_fpts change places behind the first update launch of a stage (all | partition): `interior`, which
  // follows `partition` (whose flux-point solution leaves for the neighbours meanwhile), writes the buffer that is disu_fpts by then
  int update(EleList list) override
  {
    if (pl.variant == 2)
    {
      ea.pk = F->pk_r;
      ea.tab = F->tab_r;
      hipLaunchKernelGGL((split_residual_kernel<ND, N>), dim3(persistent_grid(e, SLOT_UPDATE, e->n_eles, element_grid<split_residual_kernel<ND, N>>(e, TB, per_cu))), dim3(TB), 0, st, ea);
    }
    else if constexpr (V3)
    {
      const bool listed = elements(list, e2.ele_list, e2.n_list);
      HFX_CHECK(!listed || e2.ele_list != nullptr || e2.n_list == 0, "split update: no element lists (the block was not built as a partitioned one)");
      const long n_work = listed ? e2.n_list : (long)e->n_eles;
      if (n_work > 0) pl.update_buf ? update_launch<true>(n_work) : update_launch<false>(n_work);
    }
    HFX_HIP(hipGetLastError());
    if (list == EleList::all || list == EleList::partition) std::swap(e->arr[HFX_DISU_FPTS], F->disu_alt);
    return 0;
  }
};

std::unique_ptr<SplitStage> SplitStage::make(hfx_eles *e, hfx_inters *const *faces, int nfb, int in_step, bool write_div, const SplitPlan &pl)
{
  const int N = tensor_n(e); // (one of the sizes: the block has fused tables)
  std::unique_ptr<SplitStage> s;
#define HFX_X(ND_, N_) \
  if (e->n_dims == ND_ && N == N_) s = std::make_unique<SplitStageT<ND_, N_>>(e, faces, nfb, pl);
  HFX_SPLIT_SIZES(HFX_X)
#undef HFX_X
  if (!s || s->init(in_step, write_div)) s.reset();
  return s;
}

bool SplitStage::elements(EleList list, const int *&ele_list, long &n_list) const
{
  const FusedData *F = e->fused.get();
  switch (list)
  {
  case EleList::all: ele_list = nullptr; n_list = 0; break;
  case EleList::interior_1: ele_list = F->upd_list_i; n_list = F->n_list_i1; break;
  case EleList::partition: ele_list = F->upd_list_b; n_list = F->n_list_b; break;
  case EleList::interior_2: ele_list = F->upd_list_i ? F->upd_list_i + F->n_list_i1 : nullptr; n_list = F->n_list_i - F->n_list_i1; break;
  case EleList::interior: ele_list = F->upd_list_i; n_list = F->n_list_i; break;
  }
  return list != EleList::all;
}

int SplitStage::over_int()
{
  HFX_CHECK(pl.variant == 3, "split stage: over-integration is a step of variant 3");
  if (!e->over_int_ready) return 0;
  return pl.oi_fold ? tensor_over_int_launch(e, true) : hfx_eles_evaluate_invFlux_over_int(e);
}

int SplitStage::sgs_kernels()
{
  // LES (eddy-viscosity closures): SGS flux at the solution points from the corrected gradient, its extrapolation to
  // the flux points (src/solver.cpp:162-167); the face kernel adds it to each side, the residual kernel to the total
  // (the back-transform of the extrapolated flux happens in the face kernel)
  HFX_CHECK(pl.variant == 2, "split stage: the SGS kernels are a step of variant 2");
  if (!e->ctx->params.viscous || !e->les_ready) return 0;
  return hfx_les_sgsf_upts_internal(e) || hfx_les_extrapolate_reference_internal(e);
}

// shock capturing inside a split-path stage: disu_fpts must follow the filtered state.  The sum-factorised kernel
// rewrites the flux points of the elements it filters; the dense form is followed by a full extrapolate_solution.
static int shock_capture_keep_fpts(hfx_eles *e)
{
  if (tensor_shock_available(e) && e->ctx->contract_mode != HFX_CONTRACT_DENSE) return tensor_shock_launch(e, true);
  if (hfx_eles_shock_capture(e)) return 1;
  return hfx_eles_extrapolate_solution(e);
}

int ensure_fused_tables(hfx_eles *e, hfx_inters *const *faces, int nfb, bool partitioned)
{
  HFX_CHECK(e->n_eles > 0, "fused path: empty element block");
  if (e->fused && e->fused->built) return 0;
  return fused_build(e, faces, nfb, partitioned);
}

int split_deferred_stage(hfx_eles *e, hfx_inters *const *faces, int nfb, int in_step, bool write_div, bool shock)
{
  SplitPlan pl;
  if (ensure_fused_tables(e, faces, nfb, false) || split_stage_plan(e, faces, nfb, e->ctx->fused_mode, &pl)) return 1;
  const auto stage = SplitStage::make(e, faces, nfb, in_step, write_div, pl);
  if (!stage || stage->run()) return 1;
  // the filter changes disu_upts(0) after the stage: redo the flux-point solution of the new state
  return shock ? shock_capture_keep_fpts(e) : 0;
}

int split_run_steps(hfx_eles *e, hfx_inters *const *faces, int nfb, int n_steps, int variant)
{
  // (an LES closure that variant 3 cannot evaluate in its flux kernel, and element sizes it does not fit, run variant 2)
  SplitPlan pl;
  if (ensure_fused_tables(e, faces, nfb, false) || split_stage_plan(e, faces, nfb, variant, &pl)) return 1;
  if (n_steps <= 0) return 0; // (a call without steps prepares the tables and the plan, and leaves the state alone)
  const int nst = n_rk_stages(e->ctx->params);
  if (hfx_eles_extrapolate_solution(e)) return 1;
  StepLoop loop{&e, 1, faces, nfb, [&](int rk) {
                  const auto stage = SplitStage::make(e, faces, nfb, rk, rk == nst - 1, pl);
                  if (!stage || stage->run()) return 1;
                  // the filter changes disu_upts(0) after the stage: redo the flux-point solution of the new state
                  return e->shock_ready ? shock_capture_keep_fpts(e) : 0;
                }};
  loop.closure = ClosureFilter::filtering_refresh_svv;
  // on a plan that keeps the gradient on chip the last stage of a step a gradient-reading monitor samples runs call by call
  loop.by_calls = pl.variant == 3 && monitor_reads_gradient(&e, 1);
  bool by_calls = false;
  if (run_step_loop(loop, n_steps, &by_calls)) return 1;
  note_gradients(e, pl.variant != 3 || by_calls);
  return 0;
}

int split_time_kernels(hfx_eles *e, hfx_inters *const *faces, int nfb, int reps, double *ms, char *names, int names_len,
                       int variant)
{
  if (ensure_fused_tables(e, faces, nfb, false)) return 1;
  const SplitPlan pl = split_plan(e, faces, nfb, variant);
  const int nst = n_rk_stages(e->ctx->params);
  hipStream_t st = e->ctx->stream;
  // The steps of a stage in launch order, each with its slot of `ms`; the element kernels in two pieces when the block
  // de-aliases (variant 3: the over-integration kernel, then the flux kernel) or carries an LES closure (variant 2: the gradient
  // kernel, then the SGS kernels) -- the second kernel's time goes to slot 4
  struct Timed { int slot; int (*step)(SplitStage &); };
  const bool oi = pl.over_int != OverInt::none, sgs = pl.variant == 2 && e->les_ready && e->ctx->params.viscous;
  std::vector<Timed> steps = {{0, [](SplitStage &s) { return s.ldg(); }}};
  if (oi)
  {
    steps.push_back({4, [](SplitStage &s) { return s.over_int(); }});
    steps.push_back({1, [](SplitStage &s) { return s.flux_kernel(); }});
  }
  else if (sgs)
  {
    steps.push_back({1, [](SplitStage &s) { return s.gradient_kernel(); }});
    steps.push_back({4, [](SplitStage &s) { return s.sgs_kernels(); }});
  }
  else
    steps.push_back({1, [](SplitStage &s) { return s.element_kernels(); }});
  steps.push_back({2, [](SplitStage &s) { return s.common_fluxes(); }});
  steps.push_back({3, [](SplitStage &s) { return s.update(); }});
  const int np = (int)steps.size();
  // one set of events per repetition and ONE synchronisation at the end: a host synchronisation per stage let the queue
  // run dry, and the first kernel after it (the flux kernel) then measured 10 % slower than in the running pipeline
  std::vector<hipEvent_t> ev((size_t)reps * (np + 1));
  for (auto &x : ev) HFX_HIP(hipEventCreate(&x));
  if (hfx_eles_extrapolate_solution(e)) return 1;
  for (int r = 0; r < reps; r++)
  {
    const int rk = r % nst;
    const auto stage = SplitStage::make(e, faces, nfb, rk, rk == nst - 1, pl);
    if (!stage) return 1;
    for (int q = 0; q < np; q++)
    {
      HFX_HIP(hipEventRecord(ev[(np + 1) * r + q], st));
      if (steps[q].step(*stage)) return 1;
    }
    HFX_HIP(hipEventRecord(ev[(np + 1) * r + np], st));
  }
  HFX_HIP(hipStreamSynchronize(st));
  double acc[8] = {};
  for (int r = 0; r < reps; r++)
    for (int q = 0; q < np; q++)
    {
      float t = 0;
      HFX_HIP(hipEventElapsedTime(&t, ev[(np + 1) * r + q], ev[(np + 1) * r + q + 1]));
      acc[steps[q].slot] += t;
    }
  for (auto &x : ev) (void)hipEventDestroy(x);
  for (int i = 0; i < 8; i++) ms[i] = acc[i] / reps;
  // (folded faces without a boundary face: the common-flux step launched nothing -- the events still lie a few microseconds apart)
  {
    bool any_bdy_faces = false;
    for (int b = 0; b < nfb; b++) any_bdy_faces = any_bdy_faces || (faces[b]->is_bdy && faces[b]->n_inters > 0);
    if (pl.fold_faces && !any_bdy_faces) ms[2] = 0.0;
  }
  if (e->fused->stamps)
  {
    long long h[64];
    HFX_HIP(hipMemcpy(h, e->fused->stamps, sizeof h, hipMemcpyDeviceToHost));
    for (int w = 0; w < 3; w++)
    {
      fprintf(stderr, "flux kernel wave %d cycles: ", w);
      for (int q = 1; q <= 9; q++) fprintf(stderr, "%s%lld", q > 1 ? " " : "", h[w * 16 + q] - h[w * 16 + q - 1]);
      fprintf(stderr, "   (fill | bar1 | A | bar2 | B | bar3 | C | bar4 | D)  total %lld;  C: reads landed after %lld\n", h[w * 16 + 9] - h[w * 16], h[w * 16 + 10] - h[w * 16 + 6]);
      if (h[w * 16 + 11])
        fprintf(stderr, "   A0 cycles: corrections written after %lld, next requests issued %lld, barrier 1b %lld\n", h[w * 16 + 11] - h[w * 16 + 2],
                h[w * 16 + 12] - h[w * 16 + 11], h[w * 16 + 13] - h[w * 16 + 12]);
    }
    fprintf(stderr, "loader wave cycles: ");
    for (int q = 1; q <= 7; q++) fprintf(stderr, "%s%lld", q > 1 ? " " : "", h[3 * 16 + q] - h[3 * 16 + q - 1]);
    fprintf(stderr, "   (wait state | bar1 | issue state, wait metrics | bar2 | bar3 | issue metrics | bar4)  total %lld\n", h[3 * 16 + 7] - h[3 * 16]);
  }
  snprintf(names, names_len, "%s%s", pl.names, pl.extra_names);
  note_gradients(e, pl.variant != 3);
  return 0;
}

int split_two_wave_face(hfx_eles *e, hfx_inters *const *faces, int nfb, int variant, int *face, long need[6])
{
  if (ensure_fused_tables(e, faces, nfb, false)) return 1;
  const SplitPlan pl = split_plan(e, faces, nfb, variant);
  for (int f = 0; f < 6; f++) need[f] = 0;
  *face = pl.two_wave ? two_wave_face(e->fused.get(), e->ctx->params.ldg_beta, need, e->ctx->opt.flux_two_wave_face) : -1;
  return 0;
}

void split_kernel_bytes(const hfx_eles *e, double *bytes, int variant)
{
  // (the plan without the face blocks: their boundary faces change only which arrays must be below 4 GiB)
  const SplitPlan pl = split_plan(e, nullptr, 0, variant);
  // ALGORITHMIC HBM bytes per launch (doubles listed per element)
  const double nu = e->n_upts, nfp = e->n_fpts, nf = e->n_fields, nd = e->n_dims, ne = e->n_eles;
  for (int i = 0; i < 8; i++) bytes[i] = 0.0;
  bytes[0] = ne * (8.0 * (2 * nfp * nf) + 4.0 * nfp + nfp * 0.5);                                   // disu r, delta w, index + meta
  bytes[1] = ne * 8.0 * (nu * nf + nfp * nf + nu * (nd * nd + 1) + nfp * (nd * nd + 1) + nfp * nf * nd); // + grad_fpts w
  bytes[2] = ne * (8.0 * (nfp * nf + nfp * nf * nd + 0.5 * nfp * nd + nfp + nfp * nf) + 4.0 * nfp);   // disu, grad, normal(left), tdA r; tconf w
  bytes[3] = ne * 8.0 * (nu * nf + nu * (nd * nd + 1) + nfp * nf + 3 * nu * nf + nfp * nf);           // u, metrics, tconf, u1 r; u0,u1,disu w
  if (pl.variant == 2 && e->les_ready)
    // SGS flux at the solution points (u, corrected gradient, metrics r; sgsf_upts w) and its extrapolation (sgsf_upts r, sgsf_fpts w)
    bytes[4] = ne * 8.0 * (nu * nf + nu * nf * nd + nu * (nd * nd + 1) + 2 * nu * nf * nd + nfp * nf * nd);
  if (pl.variant == 3)
  {
    // u, delta, volume + flux-point metrics, own normals r ; div, norm_tdisf, Fn w
    // (norm_tdisf: the dictionary-row form only; the sum-factorised kernel folds opp_3 . norm_tdisf into div)
    const double ntd = pl.flux != FluxForm::dictionary_rows ? 0.0 : nfp * nf;
    bytes[1] = ne * 8.0 * (nu * nf + nfp * nf + nu * (nd * nd + 1) + nfp * (nd * nd + 1) + nfp * nd + nu * nf + nfp * nf + ntd);
    bytes[2] = ne * (8.0 * (nfp * nf + nfp * nf + 0.5 * nfp * nd + nfp + nfp * nf) + 4.0 * nfp); // disu, Fn, normal(left), tdA r; tconf w
    bytes[3] = ne * 8.0 * (3 * nu * nf + nu + nfp * nf + ntd + 2 * nu * nf + nfp * nf);          // u0,u1,div,detjac,tconf(,ntd) r; u0,u1,disu w
    if (e->les_ready)
    {
      // the closure in the flux kernel: tdA at the flux points, the squared length scale, the Leonard terms of the similarity models
      const int m = e->les.sgs_model;
      bytes[1] += ne * 8.0 * (nfp + nu + ((m == 2 || m == 4) ? nu * (nd == 3 ? 9.0 : 5.0) : 0.0)); // tdA, length scale, Leonard terms
    }
    if (e->over_int_ready)
    {
      // the flux kernel reads the de-aliased flux too; the over-integration kernel: u, the metric tensors at the cubature points r, tdisf w
      // (folded: its contribution to the divergence, n_fields values per solution point)
      const double tdisf = pl.oi_fold ? nu * nf : nu * nf * nd;
      bytes[1] += ne * 8.0 * tdisf;
      bytes[4] = ne * 8.0 * (nu * nf + nd * nd * e->n_cubpts + tdisf);
    }
    if (pl.gather)
    {
      // the flux kernel reads the partners' flux-point solution (as many doubles as the corrections it no longer reads) and
      // a partner word per point; the pairwise LDG kernel is not launched
      bytes[0] = 0.0;
      bytes[1] += ne * 4.0 * nfp;
    }
    if (e->fused && e->fused->built)
    {
      // One-sided LDG (|ldg_beta| = 1/2): of every interior pair one side's Fn enters the common flux.  The face kernel reads that
      // side alone, and the flux kernel that knows its points' partners (gather) writes that side alone.  bytes[5]: the flux points
      // whose Fn is needed -- one per pair, every boundary and partition-face point; every point with another beta, without
      // viscosity, or in 2-D, where the stage is as it was --, bytes[6]: the bytes per stage that are not moved for the others: the face
      // kernel's reads, and the flux kernel's writes in its affine form.  (bytes[1] and bytes[2] keep the count of every point: they
      // price the two kernels as if all were needed.)
      const Phys P = e->ctx->phys();
      const bool one_sided = P.viscous && nd == 3 && ((0.5 + P.ldg_beta) == 0.0 || (0.5 - P.ldg_beta) == 0.0);
      const double idle = one_sided ? 0.5 * (double)e->fused->n_interior_fpts : 0.0;
      bytes[5] = nfp * ne - idle;
      bytes[6] = 8.0 * nf * idle * (pl.affine ? 2.0 : 1.0);
    }
    if (pl.affine)
    {
      // the element's metric record in place of the per-point metrics: the flux kernel reads its 34 doubles and JGinv at the
      // solution points (which transforms the total flux) instead of JGinv / detjac at both point sets and the own normals; the
      // update kernel the record's detjac.  The face kernel keeps the per-point normal and tdA (they multiply the pressure).
      bytes[1] += ne * 8.0 * (AffRec::SIZE + nu * nd * nd - (nu * (nd * nd + 1) + nfp * (nd * nd + 1) + nfp * nd));
      bytes[3] += ne * 8.0 * (1.0 - nu);
    }
    if (pl.fold_faces && e->fused && e->fused->built)
    {
      // The two-wave flux kernel forms the interior pairs' common flux: per pair the stage no longer moves the face kernel's reads
      // (both disu, the needed Fn, the left normal, both tdA, the two point indices) and writes (both norm_tconf) nor the flux
      // kernel's Fn; the flux kernel takes on the partner's disu (a re-read, expected in L2), the normal, both tdA and both
      // norm_tconf.  bytes[7]: the difference per stage.  (bytes[1] and bytes[2] stay as they are: the roofline of the flux
      // kernel is priced without the pairs' traffic, that of the face kernel as if it ran.)
      const double pairs = 0.5 * (double)e->fused->n_interior_fpts;
      bytes[7] = pairs * (8.0 * 3 * nf + 8.0);
    }
  }
}


#include "split_partitioned.hpp"

} // namespace hfx
