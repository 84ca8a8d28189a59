// averages.hip -- time-averaged fields on the device: run_input.average_fields (src/input.cpp:115-133), the array
// disu_average_upts (src/eles.cpp:124-127), eles::CalcTimeAverageQuantities (src/eles.cpp:5630-5702) and the clock the
// reference's main loop keeps around it (src/HiFiLES.cpp:221-245).  gfx950 only.
//
// The update is one streaming kernel per block and time step: it reads the density and every momentum / energy plane of
// disu_upts(0) a registered field needs ONCE, serves all registered fields from them, and reads and writes every plane of
// disu_average_upts once -- 15 doubles per solution point with the reference's five fields.
//
// Not built: the reference stops with "NaN in average value" (src/eles.cpp:5698).  An average is a * average + b * current of
// a zero-initialised array, so a NaN average means a NaN state, and the residual's scan already reports that
// (hfx_eles_check_nan); the kernel stays free of a flag and of the atomic that sets it.
#include "step_loop.hpp"

namespace hfx
{

// by value in the kernel's argument segment
struct AverageArgs
{
  const double *disu_upts; // (n_upts, n_eles, n_fields): disu_upts(0)
  double *average;         // (n_upts, n_eles, n)
  const double *dt_local;  // (n_eles): dt_type 2, a and b per element; nullptr: the a and b below
  long P;                  // n_upts * n_eles, the length of one field plane
  int n_upts, n;
  // plane of disu_upts each registered field is made of: 0 the density itself, f > 0 field f divided by the density
  unsigned char plane[HFX_MAX_AVERAGE_FIELDS];
  unsigned need; // bit f: plane f (1..4) is read
  double a, b;   // dt_type 0 / 1
  double t;      // time - spinup_time; t == 0 exactly when time == spinup_time (a = 0, b = 1)
};

// W consecutive solution points of one plane as one access: 16 bytes for W = 2 (P even: every plane, P doubles after the
// last, is then 16-byte aligned), 8 bytes for W = 1
template <int W> struct Points { double v[W]; };
template <int W> __device__ inline Points<W> load_points(const double *p);
template <> __device__ inline Points<1> load_points<1>(const double *p) { return {{p[0]}}; }
template <> __device__ inline Points<2> load_points<2>(const double *p)
{
  const double2 t = *reinterpret_cast<const double2 *>(p);
  return {{t.x, t.y}};
}
__device__ inline void store_points(double *p, const Points<1> &x) { p[0] = x.v[0]; }
__device__ inline void store_points(double *p, const Points<2> &x) { *reinterpret_cast<double2 *>(p) = make_double2(x.v[0], x.v[1]); }

// the reference's weights (src/eles.cpp:5684-5694), in its order of operations; t = time - spinup_time
__host__ __device__ inline void average_weights(double t, double dt, double &a, double &b)
{
  if (t == 0.0)
  {
    a = 0.0;
    b = 1.0;
  }
  else
  {
    a = (t - dt) / t;
    b = dt / t;
  }
}

// One thread: W consecutive solution points, grid-stride over the P / W items of a plane.  The quotients are IEEE
// divisions (the build has no fast-math) and a * average + b * current is evaluated as written, contracted to an FMA at most.
template <int W>
__global__ __launch_bounds__(256) void time_average_kernel(const AverageArgs A)
{
  const long n_items = A.P / W;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < n_items; it += stride)
  {
    const long p = it * W;
    const Points<W> rho = load_points<W>(A.disu_upts + p);
    Points<W> q[5] = {};
#pragma unroll
    for (int f = 1; f < 5; f++)
      if (A.need & (1u << f))
      {
        const Points<W> m = load_points<W>(A.disu_upts + f * A.P + p);
#pragma unroll
        for (int w = 0; w < W; w++) q[f].v[w] = m.v[w] / rho.v[w];
      }
    double a[W], b[W];
#pragma unroll
    for (int w = 0; w < W; w++)
    {
      a[w] = A.a;
      b[w] = A.b;
      if (A.dt_local) average_weights(A.t, A.dt_local[(p + w) / A.n_upts], a[w], b[w]);
    }
    for (int i = 0; i < A.n; i++)
    {
      const int pl = A.plane[i];
      double *dst = A.average + i * A.P + p;
      Points<W> avg = load_points<W>(dst);
#pragma unroll
      for (int w = 0; w < W; w++)
      {
        // (selects between registers: no indexing by pl)
        const double cur = pl == 0 ? rho.v[w] : pl == 1 ? q[1].v[w] : pl == 2 ? q[2].v[w] : pl == 3 ? q[3].v[w] : q[4].v[w];
        avg.v[w] = a[w] * avg.v[w] + b[w] * cur;
      }
      store_points(dst, avg);
    }
  }
}

// one update of e's averages on the compute stream
int launch_time_average(hfx_eles *e, double time, double spinup_time)
{
  hfx_ctx *ctx = e->ctx;
  if (e->n_average_fields == 0 || e->n_eles == 0) return 0;
  HFX_CHECK(ctx->have_params, "parameters not set");
  AverageArgs A{};
  A.disu_upts = e->arr[HFX_DISU_UPTS0];
  A.average = e->disu_average_upts;
  A.P = (long)e->n_upts * e->n_eles;
  A.n_upts = e->n_upts;
  A.n = e->n_average_fields;
  for (int i = 0; i < A.n; i++)
  {
    const int c = e->average_codes[i];
    const int pl = c == HFX_AVG_RHO ? 0 : c == HFX_AVG_E ? e->n_dims + 1 : c; /* src/eles.cpp:5646-5674 */
    A.plane[i] = (unsigned char)pl;
    if (pl > 0) A.need |= 1u << pl;
  }
  A.t = time - spinup_time;
  if (ctx->params.dt_type == 2)
  {
    HFX_CHECK(e->arr[HFX_DT_LOCAL], "CalcTimeAverageQuantities: dt_type 2 averages with the elements' own time steps, and dt_local "
                                    "has not been computed (hfx_eles_calc_dt_local) or uploaded");
    A.dt_local = e->arr[HFX_DT_LOCAL];
  }
  else
    average_weights(A.t, ctx->params.dt, A.a, A.b);
  const int W = (A.P % 2 == 0) ? 2 : 1;
  const long blocks = (A.P / W + 255) / 256;
  const dim3 grid((unsigned)std::min<long>(blocks, 2048)), block(256);
  if (W == 2)
    hipLaunchKernelGGL(time_average_kernel<2>, grid, block, 0, ctx->stream, A);
  else
    hipLaunchKernelGGL(time_average_kernel<1>, grid, block, 0, ctx->stream, A);
  HFX_HIP(hipGetLastError());
  return 0;
}

} // namespace hfx

using namespace hfx;

extern "C" {

int hfx_ctx_set_clock(hfx_ctx *ctx, double time, int i_steps)
{
  HFX_CHECK(ctx, "hfx_ctx_set_clock: NULL ctx");
  HFX_CHECK(i_steps >= 0, "hfx_ctx_set_clock: i_steps %d", i_steps);
  ctx->time = time;
  ctx->i_steps = i_steps;
  ctx->have_clock = true;
  return 0;
}

int hfx_flush_for_samples(hfx_eles *const *eles, int n_ele_blocks, int which)
{
  HFX_CHECK(eles && n_ele_blocks > 0 && eles[0], "hfx_flush_for_samples: no element blocks");
  HFX_CHECK(which >= 0 && which < 8, "hfx_flush_for_samples: which %d (the sum of 1 integrals, 2 history, 4 plot)", which);
  unsigned need = 0;
  for (int i = 0; i < n_ele_blocks; i++)
  {
    HFX_CHECK(eles[i] && eles[i]->ctx == eles[0]->ctx, "hfx_flush_for_samples: the blocks belong to several contexts");
    if (which & 1) need |= integral_sample_need(eles[i]);
    if (which & 2) need |= history_sample_need(eles[i]);
    if (which & 4) need |= plot_sample_need(eles[i]);
  }
  return defer_flush(eles[0]->ctx, need);
}

int hfx_ctx_set_spinup_time(hfx_ctx *ctx, double spinup_time)
{
  HFX_CHECK(ctx, "hfx_ctx_set_spinup_time: NULL ctx");
  ctx->spinup_time = spinup_time;
  return 0;
}

int hfx_ctx_get_clock(hfx_ctx *ctx, double *time, int *i_steps, double *spinup_time)
{
  HFX_CHECK(ctx, "hfx_ctx_get_clock: NULL ctx");
  if (time) *time = ctx->time;
  if (i_steps) *i_steps = ctx->i_steps;
  if (spinup_time) *spinup_time = ctx->spinup_time;
  return 0;
}

int hfx_eles_set_average_fields(hfx_eles *e, int n, const int *codes)
{
  HFX_CHECK(e && (n == 0 || codes), "hfx_eles_set_average_fields: NULL argument");
  HFX_CHECK(n >= 0 && n <= HFX_MAX_AVERAGE_FIELDS, "hfx_eles_set_average_fields: %d fields (at most %d)", n, HFX_MAX_AVERAGE_FIELDS);
  for (int i = 0; i < n; i++)
  {
    HFX_CHECK(codes[i] >= HFX_AVG_RHO && codes[i] <= HFX_AVG_E, "hfx_eles_set_average_fields: unknown average field %d", codes[i]);
    HFX_CHECK(codes[i] != HFX_AVG_W || e->n_dims == 3, "hfx_eles_set_average_fields: w_average on a two-dimensional block");
  }
  HFX_IMMEDIATE(e->ctx, 0);
  HFX_HIP(hipStreamSynchronize(e->ctx->stream)); // (an update of the array that goes may still be running)
  e->n_average_fields = 0;
  e->disu_average_upts.reset();
  e->disu_average_ppts.reset();
  if (n == 0) return 0;
  if (e->disu_average_upts.alloc_zeroed((size_t)e->n_upts * e->n_eles * n)) return 1;
  std::copy(codes, codes + n, e->average_codes);
  e->n_average_fields = n;
  return 0;
}

int hfx_eles_upload_average(hfx_eles *e, const double *host)
{
  HFX_CHECK(e && host, "hfx_eles_upload_average: NULL argument");
  HFX_CHECK(e->n_average_fields > 0, "hfx_eles_upload_average: no average fields (hfx_eles_set_average_fields)");
  HFX_IMMEDIATE(e->ctx, 0);
  HFX_HIP(hipStreamSynchronize(e->ctx->stream));
  HFX_HIP(hipMemcpy(e->disu_average_upts, host, sizeof(double) * (size_t)e->n_upts * e->n_eles * e->n_average_fields,
                    hipMemcpyHostToDevice));
  return 0;
}

int hfx_eles_download_average(hfx_eles *e, double *host)
{
  HFX_CHECK(e && host, "hfx_eles_download_average: NULL argument");
  HFX_CHECK(e->n_average_fields > 0, "hfx_eles_download_average: no average fields (hfx_eles_set_average_fields)");
  HFX_IMMEDIATE(e->ctx, 0);
  HFX_HIP(hipStreamSynchronize(e->ctx->stream));
  HFX_HIP(hipMemcpy(host, e->disu_average_upts, sizeof(double) * (size_t)e->n_upts * e->n_eles * e->n_average_fields,
                    hipMemcpyDeviceToHost));
  return 0;
}

int hfx_eles_CalcTimeAverageQuantities(hfx_eles *e, double time, double spinup_time)
{
  HFX_CHECK(e, "NULL eles");
  // (the stage that has been recorded leaves disu_upts(0) of the new state whichever way it runs)
  HFX_IMMEDIATE(e->ctx, 0);
  return launch_time_average(e, time, spinup_time);
}

} // extern "C"
