// wall_force.hip -- the force on the walls on the device: output::CalcForces (src/output.cpp:1915-2014) and
// eles::compute_wall_forces (src/eles.cpp:5704-5990): Fx, Fy(, Fz), CL, CD of history.plt and Cp, Cf at every wall cubature
// point.  gfx950 only.
//
// One fused kernel per call, in the shape of error_norm_kernel (error_norm.hip).  A workgroup of 256 threads walks passes of `fpp`
// consecutive faces of the SORTED face list in a persistent grid-stride loop; the lanes of a pass own its (face, cubature point)
// pairs.  Per pass the workgroup stages ONE slab at a time in LDS -- the n_upts x n_fields state of the faces' elements first,
// then (a viscous context only) the gradient with respect to each dimension in turn -- and every lane forms its n_fields dot
// products over n_upts from it: the lanes of one face read the same LDS word (a broadcast), the operator of its local face
// comes through L2, consecutive lanes reading consecutive cubature points of one column.  The faces are sorted once, at
// registration, by (local face, element): the lanes of a wave then mostly read one operator and a pass mostly stages
// neighbouring elements.  Everything is runtime-sized; the kernel knows no element class.
//
// Reproducible: the lanes' sums are combined by a butterfly of cross-lane shuffles, the waves' sums by one lane in wave order,
// every workgroup stores one partial per quantity with an ordinary store, and the host adds the partials in workgroup order.
// No floating-point atomics; the result is a function of the state, the registered arrays and the grid.
#include "hfx_internal.hpp"

#include <cmath>
#include <numeric>

namespace hfx
{

// by value in the kernel's argument segment
struct WallArgs
{
  const double *disu_upts;      // (n_upts, n_eles, n_fields): disu_upts(0)
  const double *grad_disu_upts; // (n_upts, n_eles, n_fields, n_dims); read when n_slabs > 1 only
  const int *ele, *inter, *dual; // (n_faces), sorted order
  const long *first;             // (n_faces), sorted order
  const int *n_cubpts;           // (n_inters)
  const long *opp_first, *weight_first; // (n_inters)
  const double *opp, *weight;
  const double *detjac, *norm;
  double *cp_cf;                // (n_points, 2)
  double *partial;              // (n_groups, 2 n_dims + 2): [group + n_groups * quantity]
  long n_eles, n_points;
  int n_faces, n_upts, max_cubpts, fpp; // fpp: faces per pass
  int n_slabs;                  // 1: the state alone; 1 + n_dims: the gradient too
  double gamma, rt_inf, mu_inf, c_sth, fix_vis;
  double factor, p_c_ic, area_ref, sin_aoa, cos_aoa, cos_aos;
};

constexpr int WF_THREADS = 256;
constexpr int WF_LDS_PASS = 32768; // bytes of LDS a pass of several faces may take (one slab)
constexpr int WF_LDS_MOST = 61440; // and one face alone (the static array of the wave sums shares the 64 KB)
constexpr int WF_GROUPS_PER_CU = 4;

template <int ND>
__global__ __launch_bounds__(WF_THREADS) void wall_force_kernel(const WallArgs A)
{
  constexpr int NF = ND + 2, NQ = 2 * ND + 2;
  extern __shared__ double slab[];                    // (n_upts, fpp, NF)
  __shared__ double wave_sum[(WF_THREADS / 64) * NQ];
  const int tid = threadIdx.x;
  const int fl = tid / A.max_cubpts, j = tid - fl * A.max_cubpts; // the lane's face of the pass and its cubature point
  const long P = (long)A.n_upts * A.n_eles;
  const int plane = A.fpp * A.n_upts;
  double acc[NQ]; // Finv (ND), Fvis (ND), cl, cd
#pragma unroll
  for (int q = 0; q < NQ; q++) acc[q] = 0.0;

  for (long s0 = (long)blockIdx.x * A.fpp; s0 < A.n_faces; s0 += (long)gridDim.x * A.fpp)
  {
    const int cnt = (int)min((long)A.fpp, (long)A.n_faces - s0);
    int l = 0, nc = 0;
    if (fl < cnt)
    {
      l = A.inter[s0 + fl];
      nc = A.n_cubpts[l];
    }
    const bool active = fl < cnt && j < nc;
    const double *row = A.opp + (active ? A.opp_first[l] + j : 0);

    double u[NF], g[NF][ND];
#pragma unroll
    for (int f = 0; f < NF; f++)
    {
      u[f] = 0.0;
#pragma unroll
      for (int n = 0; n < ND; n++) g[f][n] = 0.0;
    }
    for (int s = 0; s < A.n_slabs; s++)
    {
      __syncthreads(); // (the slab before this one has been read)
      const double *src = (s == 0 ? A.disu_upts : A.grad_disu_upts + P * NF * (s - 1));
      for (int idx = tid; idx < cnt * A.n_upts; idx += WF_THREADS)
      {
        const int q = idx / A.n_upts, k = idx - q * A.n_upts;
        const double *from = src + (long)A.ele[s0 + q] * A.n_upts + k;
#pragma unroll
        for (int f = 0; f < NF; f++) slab[f * plane + idx] = from[f * P];
      }
      __syncthreads();
      if (!active) continue; // (no barrier below in this iteration)
      double v[NF];
#pragma unroll
      for (int f = 0; f < NF; f++) v[f] = 0.0;
      const double *us = slab + fl * A.n_upts;
      for (int k = 0; k < A.n_upts; k++)
      {
        const double c = row[(long)nc * k];
#pragma unroll
        for (int f = 0; f < NF; f++) v[f] += c * us[f * plane + k];
      }
#pragma unroll
      for (int f = 0; f < NF; f++)
      {
        if (s == 0) u[f] = v[f];
#pragma unroll
        for (int n = 0; n < ND; n++)
          if (s == n + 1) g[f][n] = v[f];
      }
    }
    if (!active) continue; // (every barrier of this pass is behind)

    // src/eles.cpp:5775-5986 for the lane's point
    const long pt = A.first[s0 + fl] + j;
    const double detjac = A.detjac[pt], wgt = A.weight[A.weight_first[l] + j];
    double norm[ND];
    {
      const double *np = A.norm + (A.first[s0 + fl] * ND + j);
#pragma unroll
      for (int m = 0; m < ND; m++) norm[m] = np[(long)nc * m];
    }
    if (A.dual[s0 + fl])
    {
      double vn = 0.;
#pragma unroll
      for (int m = 0; m < ND; m++) vn += u[m + 1] * norm[m];
      vn /= u[0];
#pragma unroll
      for (int m = 0; m < ND; m++) u[m + 1] = u[m + 1] - vn * norm[m];
    }
    double v_sq = 0.;
#pragma unroll
    for (int m = 0; m < ND; m++) v_sq += u[m + 1] * u[m + 1];
    const double p = (A.gamma - 1.0) * (u[ND + 1] - 0.5 * v_sq / u[0]);
    const double cp = (p - A.p_c_ic) * A.factor;
    double Finv[ND], Fvis[ND];
#pragma unroll
    for (int m = 0; m < ND; m++)
    {
      Finv[m] = wgt * (p - A.p_c_ic) * norm[m] * detjac * A.factor / A.area_ref;
      Fvis[m] = 0.0;
    }
    double cl = -Finv[0] * A.sin_aoa + Finv[1] * A.cos_aoa, cd;
    if (ND == 2)
      cd = Finv[0] * A.cos_aoa + Finv[1] * A.sin_aoa;
    else
      cd = Finv[0] * A.cos_aoa * A.cos_aos + Finv[1] * A.sin_aoa + Finv[ND - 1] * A.sin_aoa * A.cos_aos;
    double cf = 0.0;
    if (A.n_slabs > 1)
    {
      double dv[ND][ND];
#pragma unroll
      for (int m = 0; m < ND; m++)
#pragma unroll
        for (int n = 0; n < ND; n++) dv[n][m] = (g[n + 1][m] - g[0][m] * u[n + 1] / u[0]) / u[0];
      double diag = 0.;
#pragma unroll
      for (int m = 0; m < ND; m++) diag += dv[m][m];
      diag /= 3.0;
      double inte = u[ND + 1] / u[0];
#pragma unroll
      for (int m = 0; m < ND; m++) inte -= 0.5 * u[m + 1] * u[m + 1] / u[0] / u[0];
      const double rt_ratio = (A.gamma - 1.0) * inte / A.rt_inf;
      double mu = A.mu_inf * pow(rt_ratio, 1.5) * (1 + A.c_sth) / (rt_ratio + A.c_sth);
      mu = mu + A.fix_vis * (A.mu_inf - mu);
      double taun[ND];
#pragma unroll
      for (int m = 0; m < ND; m++)
      {
        double t = 0.0;
#pragma unroll
        for (int n = 0; n < ND; n++)
        {
          double S = 0.5 * (dv[m][n] + dv[n][m]);
          if (m == n) S -= diag;
          t += 2. * mu * S * norm[n];
        }
        taun[m] = t;
      }
      double taundotn = 0.;
#pragma unroll
      for (int m = 0; m < ND; m++) taundotn += taun[m] * norm[m];
      double tauw = 0.;
#pragma unroll
      for (int m = 0; m < ND; m++)
      {
        const double tt = taun[m] - taundotn * norm[m];
        tauw += tt * tt;
      }
      tauw = sqrt(tauw);
      cf = tauw * A.factor;
#pragma unroll
      for (int m = 0; m < ND; m++) Fvis[m] = -wgt * taun[m] * detjac * A.factor / A.area_ref;
      cl += -Fvis[0] * A.sin_aoa + Fvis[1] * A.cos_aoa;
      if (ND == 2)
        cd += Fvis[0] * A.cos_aoa + Fvis[1] * A.sin_aoa;
      else
        cd += Fvis[0] * A.cos_aoa * A.cos_aos + Fvis[1] * A.sin_aoa + Fvis[ND - 1] * A.sin_aoa * A.cos_aos;
    }
    A.cp_cf[pt] = cp;
    A.cp_cf[A.n_points + pt] = cf;
#pragma unroll
    for (int m = 0; m < ND; m++)
    {
      acc[m] += Finv[m];
      acc[ND + m] += Fvis[m];
    }
    acc[2 * ND] += cl;
    acc[2 * ND + 1] += cd;
  }

  // lane l += lane l ^ 32, ^ 16, ... ^ 1, then the waves in their order
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int q = 0; q < NQ; q++)
  {
    double a = acc[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
    if (lane == 0) wave_sum[wave * NQ + q] = a;
  }
  __syncthreads();
  if (tid < NQ)
  {
    double s = 0.0;
    for (int wv = 0; wv < WF_THREADS / 64; wv++) s += wave_sum[wv * NQ + tid];
    A.partial[blockIdx.x + (size_t)gridDim.x * tid] = s;
  }
}

// what a call launches for the block as it stands: faces per pass, workgroups, bytes of LDS
struct WallLaunch
{
  int fpp = 0, groups = 0;
  size_t lds = 0;
};
static int plan_launch(const hfx_eles *e, WallLaunch &L)
{
  HFX_CHECK(e->wall_forces, "compute_wall_forces: no wall faces registered (hfx_eles_set_wall_faces)");
  const WallForces &W = *e->wall_forces;
  const size_t per_face = sizeof(double) * (size_t)e->n_upts * e->n_fields; // one slab of one face's element
  HFX_CHECK(per_face <= (size_t)WF_LDS_MOST, "compute_wall_forces: %d solution points of %d fields do not fit the kernel's %d bytes of LDS",
            e->n_upts, e->n_fields, WF_LDS_MOST);
  const int nc = std::max(1, W.max_cubpts);
  L.fpp = std::max<int>(1, std::min<size_t>((size_t)(WF_THREADS / nc), (size_t)WF_LDS_PASS / per_face));
  L.lds = per_face * L.fpp;
  const long passes = std::max<long>(1, ((long)W.n_faces + L.fpp - 1) / L.fpp);
  long groups = std::min<long>(passes, (long)WF_GROUPS_PER_CU * e->ctx->n_cu);
  const int cap = e->ctx->opt.persistent_grid_cap;
  if (cap > 0) groups = std::min<long>(groups, cap);
  L.groups = (int)groups;
  return 0;
}

// everything that refuses a call, in the order the header states, before anything is launched (a recorded stage included)
static int check_call(const hfx_eles *e, const char *who)
{
  const hfx_ctx *ctx = e->ctx;
  HFX_CHECK(e->wall_forces, "%s: no wall faces registered (hfx_eles_set_wall_faces)", who);
  HFX_CHECK(ctx->have_force_ref, "%s: no force reference (hfx_ctx_set_force_reference)", who);
  HFX_CHECK(ctx->have_params, "parameters not set");
  HFX_CHECK(e->n_fields == e->n_dims + 2 && (e->n_dims == 2 || e->n_dims == 3), "%s: a block of %d fields in %d dimensions", who,
            e->n_fields, e->n_dims);
  return 0;
}

static int launch_wall_forces(hfx_eles *e, const WallLaunch &L, bool grad)
{
  hfx_ctx *ctx = e->ctx;
  WallForces &W = *e->wall_forces;
  WallArgs A{};
  A.disu_upts = e->arr[HFX_DISU_UPTS0];
  A.grad_disu_upts = grad ? e->arr[HFX_GRAD_DISU_UPTS].get() : nullptr;
  A.ele = W.ele;
  A.inter = W.inter;
  A.dual = W.dual;
  A.first = W.first;
  A.n_cubpts = W.n_cubpts;
  A.opp_first = W.opp_first;
  A.weight_first = W.weight_first;
  A.opp = W.opp;
  A.weight = W.weight;
  A.detjac = W.detjac;
  A.norm = W.norm;
  A.cp_cf = W.cp_cf;
  A.partial = W.partial;
  A.n_eles = e->n_eles;
  A.n_points = W.n_points;
  A.n_faces = W.n_faces;
  A.n_upts = e->n_upts;
  A.max_cubpts = W.max_cubpts;
  A.fpp = L.fpp;
  A.n_slabs = grad ? 1 + e->n_dims : 1;
  A.gamma = ctx->params.gamma;
  A.rt_inf = ctx->params.rt_inf;
  A.mu_inf = ctx->params.mu_inf;
  A.c_sth = ctx->params.c_sth;
  A.fix_vis = ctx->params.fix_vis;
  A.factor = ctx->force_factor;
  A.p_c_ic = ctx->force_ref.p_c_ic;
  A.area_ref = ctx->force_ref.area_ref;
  A.sin_aoa = std::sin(ctx->force_aoa);
  A.cos_aoa = std::cos(ctx->force_aoa);
  A.cos_aos = std::cos(ctx->force_aos);
  if (e->n_dims == 3)
    hipLaunchKernelGGL(wall_force_kernel<3>, dim3(L.groups), dim3(WF_THREADS), L.lds, ctx->stream, A);
  else
    hipLaunchKernelGGL(wall_force_kernel<2>, dim3(L.groups), dim3(WF_THREADS), L.lds, ctx->stream, A);
  HFX_HIP(hipGetLastError());
  return 0;
}

// the arrays a launch needs beside the registration: the state, the gradient (checked current), the partials of this grid
static int prepare_launch(hfx_eles *e, const WallLaunch &L, bool grad, const char *who)
{
  HFX_CHECK(e->arr[HFX_DISU_UPTS0], "%s: the solution was never uploaded", who);
  if (grad)
  {
    HFX_CHECK(e->arr[HFX_GRAD_DISU_UPTS], "%s: no gradient has been computed yet", who);
    HFX_CHECK_CURRENT(e, HFX_GRAD_DISU_UPTS, who);
  }
  WallForces &W = *e->wall_forces;
  const size_t n_partial = (size_t)L.groups * (2 * e->n_dims + 2);
  if (W.partial.size() < n_partial && W.partial.alloc(n_partial)) return 1;
  return 0;
}

// for the rows of the history monitor (history.hip), on a block with wall faces: the call's checks and arrays ...
int wall_force_partials_prepare(hfx_eles *e, const char *who)
{
  if (check_call(e, who)) return 1;
  WallLaunch L;
  if (plan_launch(e, L)) return 1;
  return prepare_launch(e, L, e->ctx->params.viscous != 0, who);
}

// ... and its kernel: the partials of n_groups workgroups are left in wall_forces->partial
int wall_force_partials_launch(hfx_eles *e, int *n_groups)
{
  WallLaunch L;
  if (plan_launch(e, L)) return 1;
  if (launch_wall_forces(e, L, e->ctx->params.viscous != 0)) return 1;
  *n_groups = L.groups;
  return 0;
}

} // namespace hfx

using namespace hfx;

extern "C" {

int hfx_ctx_set_force_reference(hfx_ctx *ctx, const hfx_force_ref *ref)
{
  HFX_CHECK(ctx && ref, "hfx_ctx_set_force_reference: NULL argument");
  const double q = ref->u_c_ic * ref->u_c_ic + ref->v_c_ic * ref->v_c_ic + ref->w_c_ic * ref->w_c_ic;
  HFX_CHECK(q > 0.0 && ref->rho_c_ic != 0.0 && ref->rho_c_ic == ref->rho_c_ic,
            "hfx_ctx_set_force_reference: rho_c_ic %g, |u_c_ic|^2 %g: no dynamic pressure to refer the forces to", ref->rho_c_ic, q);
  HFX_CHECK(ref->area_ref > 0.0, "hfx_ctx_set_force_reference: area_ref %g", ref->area_ref);
  ctx->force_ref = *ref;
  ctx->force_factor = 1.0 / (0.5 * ref->rho_c_ic * q);   /* src/eles.cpp:5743 */
  ctx->force_aoa = std::atan2(ref->v_c_ic, ref->u_c_ic); /* :5734 */
  ctx->force_aos = std::atan2(ref->w_c_ic, ref->u_c_ic); /* :5739 */
  ctx->have_force_ref = true;
  return 0;
}

int hfx_eles_set_wall_faces(hfx_eles *e, int n_faces, const int *face_ele, const int *face_inter, const int *face_flag,
                            int n_inters_per_ele, const int *n_cubpts_per_inter, const double *const *opp_inters_cubpts,
                            const double *const *weight_inters_cubpts, const double *inter_detjac_inters_cubpts,
                            const double *norm_inters_cubpts)
{
  HFX_CHECK(e, "hfx_eles_set_wall_faces: NULL eles");
  HFX_CHECK(n_faces >= 0, "hfx_eles_set_wall_faces: %d faces", n_faces);
  HFX_CHECK(n_faces == 0 || (face_ele && face_inter && face_flag && n_cubpts_per_inter && opp_inters_cubpts &&
                             weight_inters_cubpts && inter_detjac_inters_cubpts && norm_inters_cubpts),
            "hfx_eles_set_wall_faces: NULL argument");
  HFX_CHECK(n_faces == 0 || n_inters_per_ele > 0, "hfx_eles_set_wall_faces: %d local faces per element", n_inters_per_ele);
  HFX_CHECK(e->n_dims == 2 || e->n_dims == 3, "hfx_eles_set_wall_faces: a block in %d dimensions", e->n_dims);
  int max_cub = 0;
  for (int f = 0; f < n_faces; f++)
  {
    HFX_CHECK(face_ele[f] >= 0 && face_ele[f] < e->n_eles, "hfx_eles_set_wall_faces: face %d names element %d of %d", f, face_ele[f], e->n_eles);
    HFX_CHECK(face_inter[f] >= 0 && face_inter[f] < n_inters_per_ele, "hfx_eles_set_wall_faces: face %d names local face %d of %d", f,
              face_inter[f], n_inters_per_ele);
    const int fg = face_flag[f];
    HFX_CHECK(fg == HFX_BC_SLIP_WALL || fg == HFX_BC_ISOTHERM_WALL || fg == HFX_BC_ADIABAT_WALL || fg == HFX_BC_SLIP_WALL_DUAL,
              "hfx_eles_set_wall_faces: face %d has bc flag %d, which is no wall", f, fg);
    const int l = face_inter[f];
    HFX_CHECK(n_cubpts_per_inter[l] > 0 && opp_inters_cubpts[l] && weight_inters_cubpts[l],
              "hfx_eles_set_wall_faces: local face %d has no surface cubature", l);
    HFX_CHECK(n_cubpts_per_inter[l] <= WF_THREADS, "hfx_eles_set_wall_faces: %d cubature points on local face %d (at most %d)",
              n_cubpts_per_inter[l], l, WF_THREADS);
    max_cub = std::max(max_cub, n_cubpts_per_inter[l]);
  }
  HFX_IMMEDIATE(e->ctx, 0);
  e->wall_forces.reset();

  auto W = std::make_unique<WallForces>();
  W->n_faces = n_faces;
  W->n_inters = n_faces ? n_inters_per_ele : 0;
  W->max_cubpts = max_cub;
  // the caller's packing: face f's points begin at first_of[f]
  std::vector<long> first_of((size_t)n_faces);
  long np = 0;
  for (int f = 0; f < n_faces; f++)
  {
    first_of[f] = np;
    np += n_cubpts_per_inter[face_inter[f]];
  }
  W->n_points = np;
  // sorted by (local face, element); equal keys keep the caller's order
  std::vector<int> order((size_t)n_faces);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    if (face_inter[a] != face_inter[b]) return face_inter[a] < face_inter[b];
    return face_ele[a] < face_ele[b];
  });
  std::vector<int> s_ele((size_t)n_faces), s_inter((size_t)n_faces), s_dual((size_t)n_faces);
  std::vector<long> s_first((size_t)n_faces);
  for (int s = 0; s < n_faces; s++)
  {
    const int f = order[s];
    s_ele[s] = face_ele[f];
    s_inter[s] = face_inter[f];
    s_dual[s] = face_flag[f] == HFX_BC_SLIP_WALL_DUAL;
    s_first[s] = first_of[f];
  }
  // the operators and weights of the local faces that are named, one behind the other
  std::vector<char> used((size_t)W->n_inters, 0);
  for (int f = 0; f < n_faces; f++) used[face_inter[f]] = 1;
  std::vector<int> ncub((size_t)W->n_inters, 0);
  std::vector<long> opp_first((size_t)W->n_inters, 0), weight_first((size_t)W->n_inters, 0);
  std::vector<double> opp, weight;
  for (int l = 0; l < W->n_inters; l++)
  {
    if (!used[l]) continue;
    ncub[l] = n_cubpts_per_inter[l];
    opp_first[l] = (long)opp.size();
    weight_first[l] = (long)weight.size();
    opp.insert(opp.end(), opp_inters_cubpts[l], opp_inters_cubpts[l] + (size_t)ncub[l] * e->n_upts);
    weight.insert(weight.end(), weight_inters_cubpts[l], weight_inters_cubpts[l] + ncub[l]);
  }
  if (W->ele.upload(s_ele) || W->inter.upload(s_inter) || W->dual.upload(s_dual) || W->first.upload(s_first)) return 1;
  if (W->n_cubpts.upload(ncub) || W->opp_first.upload(opp_first) || W->weight_first.upload(weight_first)) return 1;
  if (W->opp.upload(opp) || W->weight.upload(weight)) return 1;
  if (W->detjac.upload(inter_detjac_inters_cubpts, (size_t)np)) return 1;
  if (W->norm.upload(norm_inters_cubpts, (size_t)np * e->n_dims)) return 1;
  if (W->cp_cf.alloc_zeroed(2 * (size_t)np)) return 1;
  e->wall_forces = std::move(W);
  return 0;
}

int hfx_eles_clear_wall_faces(hfx_eles *e)
{
  HFX_CHECK(e, "hfx_eles_clear_wall_faces: NULL eles");
  HFX_IMMEDIATE(e->ctx, 0);
  e->wall_forces.reset();
  return 0;
}

int hfx_eles_wall_force_launch(hfx_eles *e, int *n_groups, int *faces_per_pass)
{
  HFX_CHECK(e, "NULL eles");
  WallLaunch L;
  if (plan_launch(e, L)) return 1;
  if (n_groups) *n_groups = L.groups;
  if (faces_per_pass) *faces_per_pass = L.fpp;
  return 0;
}

int hfx_eles_compute_wall_forces(hfx_eles *e, double *inv_force, double *vis_force, double *cl, double *cd, double *cp, double *cf)
{
  HFX_CHECK(e && inv_force && vis_force && cl && cd, "hfx_eles_compute_wall_forces: NULL argument");
  hfx_ctx *ctx = e->ctx;
  if (check_call(e, "hfx_eles_compute_wall_forces")) return 1;
  WallLaunch L;
  if (plan_launch(e, L)) return 1;
  // an inviscid context never touches the gradient and asks a recorded stage for nothing
  const bool grad = ctx->params.viscous != 0;
  HFX_IMMEDIATE(ctx, grad ? (1u << HFX_DISU_UPTS0) | (1u << HFX_GRAD_DISU_UPTS) : 0u);
  const int nd = e->n_dims, nq = 2 * nd + 2;
  WallForces &W = *e->wall_forces;
  // (a refused call leaves the caller's arrays as they were)
  if (W.n_faces != 0 && prepare_launch(e, L, grad, "hfx_eles_compute_wall_forces")) return 1;
  for (int m = 0; m < nd; m++) inv_force[m] = vis_force[m] = 0.0;
  *cl = *cd = 0.0;
  if (W.n_faces == 0) return 0;
  if (launch_wall_forces(e, L, grad)) return 1;
  hipStream_t st = ctx->stream;
  const size_t n_partial = (size_t)L.groups * nq;
  std::vector<double> part(n_partial), pts;
  HFX_HIP(hipMemcpyAsync(part.data(), W.partial, sizeof(double) * n_partial, hipMemcpyDeviceToHost, st));
  if (cp || cf)
  {
    pts.resize(2 * (size_t)W.n_points);
    HFX_HIP(hipMemcpyAsync(pts.data(), W.cp_cf, sizeof(double) * pts.size(), hipMemcpyDeviceToHost, st));
  }
  HFX_HIP(hipStreamSynchronize(st));
  double sum[8];
  for (int q = 0; q < nq; q++)
  {
    double s = 0.0;
    for (int b = 0; b < L.groups; b++) s += part[b + (size_t)L.groups * q];
    sum[q] = s;
  }
  for (int m = 0; m < nd; m++)
  {
    inv_force[m] = sum[m];
    vis_force[m] = sum[nd + m];
  }
  *cl = sum[2 * nd];
  *cd = sum[2 * nd + 1];
  if (cp) std::copy(pts.begin(), pts.begin() + W.n_points, cp);
  if (cf) std::copy(pts.begin() + W.n_points, pts.end(), cf);
  return 0;
}

int hfx_time_wall_forces(hfx_eles *e, int reps, double *ms)
{
  HFX_CHECK(e && ms && reps > 0, "hfx_time_wall_forces: bad argument");
  if (check_call(e, "hfx_time_wall_forces")) return 1;
  WallLaunch L;
  if (plan_launch(e, L)) return 1;
  const bool grad = e->ctx->params.viscous != 0;
  HFX_IMMEDIATE(e->ctx, grad ? (1u << HFX_DISU_UPTS0) | (1u << HFX_GRAD_DISU_UPTS) : 0u);
  HFX_CHECK(e->wall_forces->n_faces > 0, "hfx_time_wall_forces: the block has no wall faces");
  if (prepare_launch(e, L, grad, "hfx_time_wall_forces")) return 1;
  hipStream_t st = e->ctx->stream;
  hipEvent_t t0, t1;
  HFX_HIP(hipEventCreate(&t0));
  HFX_HIP(hipEventCreate(&t1));
  int rc = launch_wall_forces(e, L, grad); // (warm)
  HFX_HIP(hipEventRecord(t0, st));
  for (int r = 0; r < reps && !rc; r++) rc = launch_wall_forces(e, L, grad);
  HFX_HIP(hipEventRecord(t1, st));
  HFX_HIP(hipEventSynchronize(t1));
  float t = 0.f;
  HFX_HIP(hipEventElapsedTime(&t, t0, t1));
  (void)hipEventDestroy(t0);
  (void)hipEventDestroy(t1);
  *ms = t / reps;
  return rc;
}

} // extern "C"
