// error_norm.hip -- exact-solution error norms on the device: eles::compute_error / eles::get_pointwise_error
// (src/eles.cpp:5076-5277) with the exact solutions eval_isentropic_vortex (src/funcs.cpp:1724-1739) and eval_couette_flow
// (src/funcs.cpp:1830-1922), the monitor the reference ends a verification run with (src/HiFiLES.cpp:324-325).  gfx950 only.
//
// One fused kernel per call.  A workgroup walks passes of `epp` consecutive elements in a persistent grid-stride loop; the lanes
// of a pass own its (element, cubature point) pairs.  Per pass the workgroup stages ONE slab at a time in LDS -- the n_upts x
// n_fields state of its elements first, then (Couette flow on a viscous context only) the gradient with respect to each
// dimension in turn -- and every lane forms its n_fields dot products over n_upts from it: the lanes of one element read the
// same LDS word (a broadcast), and the operator is the registered dense (n_cubpts, n_upts) column-major matrix, so consecutive
// lanes read consecutive cubature points of one column.  The lane then takes the difference to the exact solution it evaluated
// at its point and adds error x weight x detjac to its own sums.  Nothing of size n_cubpts x n_eles is ever written: what
// hfx_eles_CalcIntegralQuantities keeps in two scratch arrays lives here in registers.
//
// Reproducible: the lanes' sums are combined by a butterfly of cross-lane shuffles, the waves' sums by one lane in wave order,
// every workgroup stores one partial per quantity with an ordinary store, and the host adds the partials in workgroup order.
// No floating-point atomics; the result is a function of the state, the registered arrays and the grid.
//
// Left for later: every pass reads its operator columns again from L2 (n_cubpts x n_upts doubles per pass and slab; 2 GB per call on
// the 32^3 P4 mesh, 8 GB with the gradient), and that, not HBM, bounds the kernel.  Several elements per lane for
// one operator value, or operator tiles staged in the LDS the slab leaves free, would cut it several times; a monitor that runs once
// per simulation has not earned the second kernel shape yet.
#include "hfx_internal.hpp"

namespace hfx
{

// by value in the kernel's argument segment
struct ErrorArgs
{
  const double *disu_upts;     // (n_upts, n_eles, n_fields): disu_upts(0)
  const double *grad_disu_upts; // (n_upts, n_eles, n_fields, n_dims); read when n_slabs > 1 only
  const double *opp;           // (n_cubpts, n_upts) column-major
  const double *weight;        // (n_cubpts)
  const double *detjac;        // (n_cubpts, n_eles)
  const double *pos;           // (n_cubpts, n_eles, n_dims)
  double *partial;             // (n_groups, 2 n_fields): [group + n_groups * (row + 2 field)]
  long n_eles;
  int n_upts, n_cubpts, epp;   // epp: elements per pass
  int n_slabs;                 // 1: the state alone; 1 + n_dims: the gradient too
  int norm_type, test_case;
  double time, gamma, prandtl;
  hfx_exact x;
};

constexpr int ERR_MAX_THREADS = 1024;
constexpr int ERR_LDS_PASS = 32768;  // bytes of LDS a pass of several elements may take (one slab)
constexpr int ERR_LDS_MOST = 61440;  // and one element alone (the static array of the wave sums shares the 64 KB)
constexpr int ERR_GROUPS_PER_CU = 4;

template <int ND>
__global__ __launch_bounds__(ERR_MAX_THREADS) void error_norm_kernel(const ErrorArgs A)
{
  constexpr int NF = ND + 2;
  extern __shared__ double slab[];                         // (n_upts, epp, NF)
  __shared__ double wave_sum[(ERR_MAX_THREADS / 64) * 2 * NF];
  const int tid = threadIdx.x;
  const int el = tid / A.n_cubpts, j = tid - el * A.n_cubpts; // the lane's element of the pass and its cubature point
  const long P = (long)A.n_upts * A.n_eles;
  const int plane = A.epp * A.n_upts;
  double acc0[NF], acc1[NF];
#pragma unroll
  for (int f = 0; f < NF; f++) acc0[f] = acc1[f] = 0.0;

  for (long i0 = (long)blockIdx.x * A.epp; i0 < A.n_eles; i0 += (long)gridDim.x * A.epp)
  {
    const int cnt = (int)min((long)A.epp, A.n_eles - i0);
    const bool active = el < cnt;
    // the exact solution at the lane's point: ex[f], and the only exact gradients that are not zero, d/dy of rho, rho u and E
    double ex[NF], gy_rho = 0.0, gy_mx = 0.0, gy_E = 0.0, w = 0.0, dj = 0.0;
#pragma unroll
    for (int f = 0; f < NF; f++) ex[f] = 0.0;
    if (active)
    {
      const long pt = j + (long)A.n_cubpts * (i0 + el), pc = (long)A.n_cubpts * A.n_eles;
      w = A.weight[j];
      dj = A.detjac[pt];
      const double px = A.pos[pt], py = A.pos[pt + pc];
      if (A.test_case == 1)
      {
        // eval_isentropic_vortex: eps = 5, the centre at (t, t); vz = 0
        const double eps = 5.0, g = A.gamma, pi = 3.14159265358979323846;
        const double x = px - A.time, y = py - A.time;
        const double fe = 1.0 - (x * x + y * y);
        const double rho = pow(1.0 - eps * eps * (g - 1.0) / (8.0 * g * pi * pi) * exp(fe), 1.0 / (g - 1.0));
        const double vx = 1. - eps * y / (2.0 * pi) * exp(fe / 2.0);
        const double vy = 1. + eps * x / (2.0 * pi) * exp(fe / 2.0);
        const double p = pow(rho, g);
        ex[0] = rho;
        ex[1] = rho * vx;
        ex[2] = rho * vy;
        ex[NF - 1] = p / (g - 1) + 0.5 * rho * (vx * vx + vy * vy);
      }
      else
      {
        // eval_couette_flow: channel height 1, the moving wall at y = 1; every exact gradient but d/dy of rho, rho u and E is
        // left at zero there (src/funcs.cpp:1898-1921), and so it is here
        const double g = A.gamma, R = A.x.R_ref, uw = A.x.u_wall;
        const double y = py;
        const double cp = (g * R) / (g - 1.0);
        const double vx = uw * y;
        const double ka = 1.0 / A.x.T_ref;
        const double kb = 0.5 * (A.prandtl / cp) * (uw * uw) * ka;
        const double ps = A.x.p_bound;
        const double Ts = A.x.T_wall + y * ka + kb * y * (1.0 - y);
        const double rho = ps / (R * Ts);
        const double mx = rho * vx;
        ex[0] = rho;
        ex[1] = mx;
        ex[NF - 1] = (ps / (g - 1.0)) + 0.5 * rho * (vx * vx);
        gy_rho = -(ps / R) * (ka - kb * y + kb * (1.0 - y)) / (Ts * Ts);
        gy_mx = gy_rho * vx + rho * uw;
        gy_E = 0.5 * gy_rho * (vx * vx) + mx * uw;
      }
    }

    double e0[NF], e1[NF];
#pragma unroll
    for (int f = 0; f < NF; f++) e0[f] = e1[f] = 0.0;
    for (int s = 0; s < A.n_slabs; s++)
    {
      __syncthreads(); // (the slab before this one has been read)
      const double *src = (s == 0 ? A.disu_upts : A.grad_disu_upts + P * NF * (s - 1)) + i0 * A.n_upts;
      for (int f = 0; f < NF; f++)
        for (int idx = tid; idx < cnt * A.n_upts; idx += blockDim.x) slab[f * plane + idx] = src[f * P + idx];
      __syncthreads();
      if (!active) continue; // (no barrier below in this iteration)
      double v[NF];
#pragma unroll
      for (int f = 0; f < NF; f++) v[f] = 0.0;
      const double *us = slab + el * A.n_upts;
      const double *row = A.opp + j;
      for (int k = 0; k < A.n_upts; k++)
      {
        const double c = row[(long)A.n_cubpts * k];
#pragma unroll
        for (int f = 0; f < NF; f++) v[f] += c * us[f * plane + k];
      }
#pragma unroll
      for (int f = 0; f < NF; f++)
      {
        double d;
        if (s == 0)
          d = v[f] - ex[f];
        else
          d = v[f] - (s != 2 ? 0.0 : f == 0 ? gy_rho : f == 1 ? gy_mx : f == NF - 1 ? gy_E : 0.0);
        const double t = (A.norm_type == 1) ? fabs(d) : d * d;
        if (s == 0) e0[f] = t;
        else e1[f] += t;
      }
    }
#pragma unroll
    for (int f = 0; f < NF; f++)
    {
      acc0[f] += e0[f] * w * dj;
      acc1[f] += e1[f] * w * dj;
    }
  }

  // lane l += lane l ^ 32, ^ 16, ... ^ 1, then the waves in their order
  const int lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
#pragma unroll
  for (int f = 0; f < NF; f++)
  {
    double a = acc0[f], b = acc1[f];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
    {
      a += __shfl_xor(a, off, 64);
      b += __shfl_xor(b, off, 64);
    }
    if (lane == 0)
    {
      wave_sum[wave * 2 * NF + 2 * f] = a;
      wave_sum[wave * 2 * NF + 2 * f + 1] = b;
    }
  }
  __syncthreads();
  if (tid < 2 * NF)
  {
    double s = 0.0;
    for (int wv = 0; wv < n_waves; wv++) s += wave_sum[wv * 2 * NF + tid];
    A.partial[blockIdx.x + (size_t)gridDim.x * tid] = s;
  }
}

// what a call launches for the block as it stands: threads per workgroup, elements per pass, workgroups, bytes of LDS
struct ErrorLaunch
{
  int threads = 0, epp = 0, groups = 0;
  size_t lds = 0;
};
static int plan_launch(const hfx_eles *e, ErrorLaunch &L)
{
  const int nc = e->n_vol_cubpts;
  HFX_CHECK(nc > 0 && e->opp_volume_cubpts.dense, "compute_error: hfx_eles_set_volume_cubpts was not called");
  HFX_CHECK(nc <= ERR_MAX_THREADS, "compute_error: %d cubature points per element (at most %d)", nc, ERR_MAX_THREADS);
  const size_t per_ele = sizeof(double) * (size_t)e->n_upts * e->n_fields; // one slab of one element
  HFX_CHECK(per_ele <= (size_t)ERR_LDS_MOST, "compute_error: %d solution points of %d fields do not fit the kernel's %d bytes of LDS",
            e->n_upts, e->n_fields, ERR_LDS_MOST);
  L.threads = nc <= 256 ? 256 : 64 * ((nc + 63) / 64);
  L.epp = std::max<int>(1, std::min<size_t>((size_t)(L.threads / nc), (size_t)ERR_LDS_PASS / per_ele));
  L.lds = per_ele * L.epp;
  const long passes = std::max<long>(1, (e->n_eles + L.epp - 1) / L.epp);
  long groups = std::min<long>(passes, (long)ERR_GROUPS_PER_CU * e->ctx->n_cu);
  const int cap = e->ctx->opt.persistent_grid_cap;
  if (cap > 0) groups = std::min<long>(groups, cap);
  L.groups = (int)groups;
  return 0;
}

} // namespace hfx

using namespace hfx;

extern "C" {

int hfx_ctx_set_exact_solution(hfx_ctx *ctx, const hfx_exact *x)
{
  HFX_CHECK(ctx, "hfx_ctx_set_exact_solution: NULL context");
  ctx->have_exact = x != nullptr;
  if (x) ctx->exact = *x;
  return 0;
}

int hfx_eles_set_error_points(hfx_eles *e, const double *pos_volume_cubpts)
{
  HFX_CHECK(e && pos_volume_cubpts, "hfx_eles_set_error_points: NULL argument");
  HFX_CHECK(e->n_vol_cubpts > 0 && e->opp_volume_cubpts.dense, "hfx_eles_set_error_points: hfx_eles_set_volume_cubpts was not called");
  HFX_IMMEDIATE(e->ctx, 0);
  e->n_err_cubpts = 0;
  if (e->pos_volume_cubpts.upload(pos_volume_cubpts, (size_t)e->n_vol_cubpts * e->n_eles * e->n_dims)) return 1;
  e->n_err_cubpts = e->n_vol_cubpts;
  return 0;
}

int hfx_eles_error_launch(hfx_eles *e, int *n_groups, int *eles_per_pass)
{
  HFX_CHECK(e, "NULL eles");
  ErrorLaunch L;
  if (plan_launch(e, L)) return 1;
  if (n_groups) *n_groups = L.groups;
  if (eles_per_pass) *eles_per_pass = L.epp;
  return 0;
}

int hfx_eles_compute_error(hfx_eles *e, int norm_type, double time, double *error)
{
  HFX_CHECK(e && error, "hfx_eles_compute_error: NULL argument");
  hfx_ctx *ctx = e->ctx;
  // everything that refuses the call comes before anything is launched, a recorded stage included
  HFX_CHECK(norm_type == 1 || norm_type == 2, "Error norm not supported!"); /* src/output.cpp:2082 */
  HFX_CHECK(ctx->have_exact, "hfx_eles_compute_error: no exact solution (hfx_ctx_set_exact_solution)");
  const int tc = ctx->exact.test_case;
  HFX_CHECK(!(tc >= 2 && tc <= 4), "hfx_eles_compute_error: test case %d is an exact solution of the advection-diffusion equation, "
                                   "which this library does not solve (equation != 0)", tc);
  HFX_CHECK(tc == 1 || tc == 5, "Test case not recognized in compute error, exiting"); /* src/eles.cpp:5247 */
  HFX_CHECK(ctx->have_params, "parameters not set");
  HFX_CHECK(e->n_fields == e->n_dims + 2 && (e->n_dims == 2 || e->n_dims == 3), "compute_error: a block of %d fields in %d dimensions",
            e->n_fields, e->n_dims);
  ErrorLaunch L;
  if (plan_launch(e, L)) return 1;
  HFX_CHECK(e->pos_volume_cubpts && e->n_err_cubpts > 0, "compute_error: hfx_eles_set_error_points was not called");
  // the gradient error exists for Couette flow on a viscous context alone (src/eles.cpp:5110); the vortex never reads the array
  const bool grad = tc == 5 && ctx->params.viscous;
  HFX_IMMEDIATE(ctx, grad ? (1u << HFX_DISU_UPTS0) | (1u << HFX_GRAD_DISU_UPTS) : 0u);
  for (int q = 0; q < 2 * e->n_fields; q++) error[q] = 0.0;
  if (e->n_eles == 0) return 0;
  HFX_CHECK(e->arr[HFX_DISU_UPTS0], "compute_error: the solution was never uploaded");
  if (grad)
  {
    HFX_CHECK(e->arr[HFX_GRAD_DISU_UPTS], "compute_error: no gradient has been computed yet");
    HFX_CHECK_CURRENT(e, HFX_GRAD_DISU_UPTS, "hfx_eles_compute_error");
  }
  const size_t n_partial = (size_t)L.groups * 2 * e->n_fields;
  if (e->err_partial.size() < n_partial && e->err_partial.alloc(n_partial)) return 1;
  ErrorArgs A{};
  A.disu_upts = e->arr[HFX_DISU_UPTS0];
  A.grad_disu_upts = grad ? e->arr[HFX_GRAD_DISU_UPTS].get() : nullptr;
  A.opp = e->opp_volume_cubpts.dense;
  A.weight = e->weight_volume_cubpts;
  A.detjac = e->vol_detjac_vol_cubpts;
  A.pos = e->pos_volume_cubpts;
  A.partial = e->err_partial;
  A.n_eles = e->n_eles;
  A.n_upts = e->n_upts;
  A.n_cubpts = e->n_vol_cubpts;
  A.epp = L.epp;
  A.n_slabs = grad ? 1 + e->n_dims : 1;
  A.norm_type = norm_type;
  A.test_case = tc;
  A.time = time;
  A.gamma = ctx->params.gamma;
  A.prandtl = ctx->params.prandtl;
  A.x = ctx->exact;
  hipStream_t st = ctx->stream;
  if (e->n_dims == 3)
    hipLaunchKernelGGL(error_norm_kernel<3>, dim3(L.groups), dim3(L.threads), L.lds, st, A);
  else
    hipLaunchKernelGGL(error_norm_kernel<2>, dim3(L.groups), dim3(L.threads), L.lds, st, A);
  HFX_HIP(hipGetLastError());
  std::vector<double> part(n_partial);
  HFX_HIP(hipMemcpyAsync(part.data(), e->err_partial, sizeof(double) * n_partial, hipMemcpyDeviceToHost, st));
  HFX_HIP(hipStreamSynchronize(st));
  for (int q = 0; q < 2 * e->n_fields; q++)
  {
    double s = 0.0;
    for (int b = 0; b < L.groups; b++) s += part[b + (size_t)L.groups * q];
    error[q] = s;
  }
  return 0;
}

} // extern "C"
