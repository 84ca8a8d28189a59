// integrals.hip -- the integral quantities of history.plt sampled on the device: the Diagnostics[...] columns the reference fills
// every monitor_res_freq steps and at step 1 (src/HiFiLES.cpp:247-266; output::CalcIntegralQuantities, src/output.cpp:2017;
// eles::CalcIntegralQuantities, src/eles.cpp:5485-5627).  gfx950 only.
//
// One fused kernel per block and sample, in the shape of error_norm.hip: a workgroup walks passes of `epp` consecutive elements in
// a persistent grid-stride loop and stages ONE slab at a time in LDS -- the state, then (an id 1-4 selected) the gradient with
// respect to each dimension in turn, without the energy's, which no quantity reads.  What error_norm.hip left for later is done
// here: a lane keeps its cubature point for E consecutive elements of the pass, so an operator value, read once from L2, serves E
// elements; the slab lies element-fastest in LDS and a lane reads its E values of one (field, solution point) as 16-byte words.
// The interpolated state (n_fields doubles) and the velocity gradient (n_dims^2 doubles, formed slab by slab) of the E elements stay
// in registers; the lane evaluates the selected quantities (integral_point.hpp) and adds diagnostic x weight x detjac to its sums.
// Nothing of size n_cubpts x n_eles is written.
//
// Reproducible: lanes are combined by a butterfly of cross-lane shuffles, waves by one lane in wave order, and a second launch of
// one workgroup adds the workgroups' partials in workgroup order into the slot's n_quantities doubles.  Ordinary stores only, no
// floating-point atomics: a sample is a function of the state, the registered arrays and the grid, whatever its slot.
//
// Which gradient: grad_disu_upts as it stands, like the reference and like the wall forces.  Behind a step that is what the last
// stage's correct_gradient left -- the gradient of that stage's INPUT state, paired with the state after the step.  The step loops
// see to it that the array holds exactly that when they sample (stage_call_by_call); the monitor forms no gradient of its own.
#include "step_loop.hpp"
#include "integral_point.hpp"

namespace hfx
{

// by value in the kernel's argument segment
struct IntegralArgs
{
  const double *disu_upts;      // (n_upts, n_eles, n_fields): disu_upts(0)
  const double *grad_disu_upts; // (n_upts, n_eles, n_fields, n_dims); read when need_grad only
  const double *opp;            // (n_cubpts, n_upts) column-major
  const double *weight;         // (n_cubpts)
  const double *detjac;         // (n_cubpts, n_eles)
  double *partial;              // (n_groups, n_q): [group + n_groups * quantity]
  long n_eles;
  int n_upts, n_cubpts;
  int lane_groups;              // groups of n_cubpts lanes that work; a pass is lane_groups * E elements
  int n_q, need_grad;
  int ids[IQ_MAX];
  double gamma;
};

constexpr int IQ_LDS_PASS = 49152;  // bytes of LDS a pass of several elements may take (one slab)
constexpr int IQ_LDS_MOST = 61440;  // and one element alone (the static array of the wave sums shares the 64 KB)
constexpr int IQ_GROUPS_PER_CU = 3; // workgroups per CU of the grid: what is resident at E = 4 (2: 1.27 ms, 3: 1.06 ms, 4: 1.39 ms for all five quantities on 32^3 P4)

// v[e][f] += sum_k opp(j, k) slab(f, k, element e of the lane), f < NFL; us: the lane's first element in the slab
template <int E, int NFL, int NF>
__device__ inline void iq_contract(const double *row, int n_cubpts, int n_upts, const double *us, int epp, double (&v)[E][NF])
{
  for (int k = 0; k < n_upts; k++)
  {
    const double c = row[(long)n_cubpts * k];
#pragma unroll
    for (int f = 0; f < NFL; f++)
    {
      const double *p = us + (size_t)(f * n_upts + k) * epp;
      if constexpr (E % 2 == 0)
      {
        // (epp is a multiple of E and the lane's first element one of E: 16-byte aligned)
        const double2 *p2 = reinterpret_cast<const double2 *>(p);
#pragma unroll
        for (int h = 0; h < E / 2; h++)
        {
          const double2 t = p2[h];
          v[2 * h][f] += c * t.x;
          v[2 * h + 1][f] += c * t.y;
        }
      }
      else
      {
#pragma unroll
        for (int e = 0; e < E; e++) v[e][f] += c * p[e];
      }
    }
  }
}

// T: the most threads a launch has (the register budget); E: elements per lane and pass
template <int ND, int E, int T>
__global__ __launch_bounds__(T) void integral_history_kernel(const IntegralArgs A)
{
  constexpr int NF = ND + 2;
  extern __shared__ __align__(16) double slab[];           // (epp, n_upts, NF), the element index fastest
  __shared__ double wave_sum[(T / 64) * IQ_MAX];
  const int tid = threadIdx.x;
  const int g = tid / A.n_cubpts, j = tid - g * A.n_cubpts; // the lane's group of elements in the pass and its cubature point
  const bool lane_on = g < A.lane_groups;
  const int epp = A.lane_groups * E;
  const long P = (long)A.n_upts * A.n_eles;
  const double w = lane_on ? A.weight[j] : 0.0;
  double acc[IQ_MAX];
#pragma unroll
  for (int m = 0; m < IQ_MAX; m++) acc[m] = 0.0;

  for (long i0 = (long)blockIdx.x * epp; i0 < A.n_eles; i0 += (long)gridDim.x * epp)
  {
    const int cnt = (int)min((long)epp, A.n_eles - i0);
    double u[E][NF], dv[E][ND][ND];
#pragma unroll
    for (int e = 0; e < E; e++)
    {
#pragma unroll
      for (int f = 0; f < NF; f++) u[e][f] = 0.0;
#pragma unroll
      for (int a = 0; a < ND; a++)
#pragma unroll
        for (int b = 0; b < ND; b++) dv[e][a][b] = 0.0;
    }
#pragma unroll
    for (int s = 0; s <= ND; s++)
    {
      if (s > 0 && !A.need_grad) continue; // (uniform over the workgroup)
      const int nfl = s == 0 ? NF : NF - 1; // no quantity reads the energy's gradient
      __syncthreads();                      // (the slab before this one has been read)
      const double *src = (s == 0 ? A.disu_upts : A.grad_disu_upts + P * NF * (s - 1)) + i0 * A.n_upts;
      for (int f = 0; f < nfl; f++)
        for (int idx = tid; idx < cnt * A.n_upts; idx += blockDim.x)
        {
          const int el = idx / A.n_upts, k = idx - el * A.n_upts;
          slab[(size_t)(f * A.n_upts + k) * epp + el] = src[f * P + idx];
        }
      __syncthreads();
      if (!lane_on) continue; // (no barrier below in this iteration)
      double v[E][NF];
#pragma unroll
      for (int e = 0; e < E; e++)
#pragma unroll
        for (int f = 0; f < NF; f++) v[e][f] = 0.0;
      if (s == 0)
      {
        iq_contract<E, NF, NF>(A.opp + j, A.n_cubpts, A.n_upts, slab + g * E, epp, v);
#pragma unroll
        for (int e = 0; e < E; e++)
#pragma unroll
          for (int f = 0; f < NF; f++) u[e][f] = v[e][f];
      }
      else
      {
        iq_contract<E, NF - 1, NF>(A.opp + j, A.n_cubpts, A.n_upts, slab + g * E, epp, v);
#pragma unroll
        for (int e = 0; e < E; e++) iq_velocity_gradient<ND>(u[e], 1. / u[e][0], v[e], s - 1, dv[e]);
      }
    }
    if (lane_on)
    {
#pragma unroll
      for (int e = 0; e < E; e++)
      {
        // (an element past the end of the pass: its slab entries are whatever the pass before left, and nothing is added)
        const bool valid = g * E + e < cnt;
        const double wd = valid ? w * A.detjac[j + (long)A.n_cubpts * (i0 + g * E + e)] : 0.0;
        const double irho = 1. / u[e][0];
        const double tke = iq_tke<ND>(u[e]);
#pragma unroll
        for (int m = 0; m < IQ_MAX; m++)
          if (m < A.n_q)
          {
            const double diagnostic = iq_diagnostic<ND>(A.ids[m], u[e], irho, tke, dv[e], A.gamma);
            if (valid) acc[m] += diagnostic * wd;
          }
      }
    }
  }

  // lane l += lane l ^ 32, ^ 16, ... ^ 1, then the waves in their order
  const int lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
#pragma unroll
  for (int m = 0; m < IQ_MAX; m++)
  {
    double a = acc[m];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
    if (lane == 0) wave_sum[wave * IQ_MAX + m] = a;
  }
  __syncthreads();
  if (tid < A.n_q)
  {
    double s = 0.0;
    for (int wv = 0; wv < n_waves; wv++) s += wave_sum[wv * IQ_MAX + tid];
    A.partial[blockIdx.x + (size_t)gridDim.x * tid] = s;
  }
}

// one workgroup: out[m] = the partials of quantity m in workgroup order
__global__ __launch_bounds__(64) void integral_finish_kernel(const double *partial, int n_groups, int n_q, double *out)
{
  const int m = threadIdx.x;
  if (m >= n_q) return;
  double s = 0.0;
  for (int b = 0; b < n_groups; b++) s += partial[b + (size_t)n_groups * m];
  out[m] = s;
}

// what a sample launches for the block as it stands
struct IntegralLaunch
{
  int threads = 0, most = 0, E = 0, lane_groups = 0, epp = 0, groups = 0;
  size_t lds = 0;
};
static int plan_launch(const hfx_eles *e, IntegralLaunch &L)
{
  const int nc = e->n_vol_cubpts;
  HFX_CHECK(nc > 0 && e->opp_volume_cubpts.dense, "integral quantities: hfx_eles_set_volume_cubpts was not called");
  HFX_CHECK(nc <= 1024, "integral quantities: %d cubature points per element (at most 1024)", nc);
  const size_t per_ele = sizeof(double) * (size_t)e->n_upts * e->n_fields; // one slab of one element
  HFX_CHECK(per_ele <= (size_t)IQ_LDS_MOST, "integral quantities: %d solution points of %d fields do not fit the kernel's %d bytes of LDS",
            e->n_upts, e->n_fields, IQ_LDS_MOST);
  L.threads = nc <= 256 ? 256 : 64 * ((nc + 63) / 64);
  L.most = L.threads <= 512 ? 512 : 1024;
  // E = 4 where four elements' slab fits and the register budget is that of 512 threads, else 2 or 1
  L.E = L.most == 1024 ? 1 : 4 * per_ele <= (size_t)IQ_LDS_PASS ? 4 : 2 * per_ele <= (size_t)IQ_LDS_PASS ? 2 : 1;
  L.lane_groups = (int)std::max<size_t>(1, std::min<size_t>((size_t)(L.threads / nc), (size_t)IQ_LDS_PASS / (per_ele * L.E)));
  L.epp = L.lane_groups * L.E;
  L.lds = per_ele * L.epp;
  const long passes = std::max<long>(1, (e->n_eles + L.epp - 1) / L.epp);
  long groups = std::min<long>(passes, (long)IQ_GROUPS_PER_CU * e->ctx->n_cu);
  const int cap = e->ctx->opt.persistent_grid_cap;
  if (cap > 0) groups = std::min<long>(groups, cap);
  L.groups = (int)groups;
  return 0;
}

// the block's history as the context's monitor wants it: made anew, empty, when the monitor has changed since
static int prepare_history(hfx_eles *e)
{
  hfx_ctx *ctx = e->ctx;
  IntegralHistory &H = e->integrals;
  if (H.history && H.epoch == ctx->iq_epoch) return 0;
  HFX_HIP(hipStreamSynchronize(ctx->stream)); // (a sample into the history that goes may still be running)
  H.times.clear();
  H.steps.clear();
  H.history.reset();
  H.n_quantities = H.capacity = 0;
  H.epoch = ctx->iq_epoch;
  if (ctx->n_iq == 0) return 0;
  if (H.history.alloc((size_t)ctx->n_iq * ((size_t)ctx->iq_capacity + 1))) return 1;
  H.n_quantities = ctx->n_iq;
  H.capacity = ctx->iq_capacity;
  return 0;
}

template <int ND>
static void launch_kernel(const IntegralLaunch &L, hipStream_t st, const IntegralArgs &A)
{
  const dim3 grid(L.groups), block(L.threads);
  if (L.most == 1024)
    hipLaunchKernelGGL((integral_history_kernel<ND, 1, 1024>), grid, block, L.lds, st, A);
  else if (L.E == 4)
    hipLaunchKernelGGL((integral_history_kernel<ND, 4, 512>), grid, block, L.lds, st, A);
  else if (L.E == 2)
    hipLaunchKernelGGL((integral_history_kernel<ND, 2, 512>), grid, block, L.lds, st, A);
  else
    hipLaunchKernelGGL((integral_history_kernel<ND, 1, 512>), grid, block, L.lds, st, A);
}

// the two launches of one sample into slot `slot` (prepare_history has run)
static int launch_sample(hfx_eles *e, int slot)
{
  hfx_ctx *ctx = e->ctx;
  IntegralHistory &H = e->integrals;
  HFX_CHECK(ctx->have_params, "parameters not set");
  HFX_CHECK(e->n_fields == e->n_dims + 2 && (e->n_dims == 2 || e->n_dims == 3), "integral quantities: a block of %d fields in %d dimensions",
            e->n_fields, e->n_dims);
  IntegralLaunch L;
  if (plan_launch(e, L)) return 1;
  const bool grad = integral_monitor_reads_gradient(ctx);
  HFX_CHECK(e->n_eles == 0 || e->arr[HFX_DISU_UPTS0], "integral quantities: the solution was never uploaded");
  HFX_CHECK(e->n_eles == 0 || !grad || e->arr[HFX_GRAD_DISU_UPTS], "integral quantities: no gradient has been computed yet");
  const size_t n_partial = (size_t)L.groups * H.n_quantities;
  if (H.partial.size() < n_partial && H.partial.alloc(n_partial)) return 1;
  hipStream_t st = ctx->stream;
  const int n_groups = e->n_eles > 0 ? L.groups : 0;
  if (n_groups > 0)
  {
    IntegralArgs A{};
    A.disu_upts = e->arr[HFX_DISU_UPTS0];
    A.grad_disu_upts = grad ? e->arr[HFX_GRAD_DISU_UPTS].get() : nullptr;
    A.opp = e->opp_volume_cubpts.dense;
    A.weight = e->weight_volume_cubpts;
    A.detjac = e->vol_detjac_vol_cubpts;
    A.partial = H.partial;
    A.n_eles = e->n_eles;
    A.n_upts = e->n_upts;
    A.n_cubpts = e->n_vol_cubpts;
    A.lane_groups = L.lane_groups;
    A.n_q = H.n_quantities;
    A.need_grad = grad;
    for (int m = 0; m < H.n_quantities; m++) A.ids[m] = ctx->iq_ids[m];
    A.gamma = ctx->params.gamma;
    if (e->n_dims == 3)
      launch_kernel<3>(L, st, A);
    else
      launch_kernel<2>(L, st, A);
    HFX_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(integral_finish_kernel, dim3(1), dim3(64), 0, st, H.partial.get(), n_groups, H.n_quantities,
                     H.history + (size_t)slot * H.n_quantities);
  HFX_HIP(hipGetLastError());
  return 0;
}

unsigned integral_sample_need(const hfx_eles *e)
{
  if (e->ctx->n_iq <= 0 || e->n_vol_cubpts <= 0) return 0;
  return integral_monitor_reads_gradient(e->ctx) ? (1u << HFX_DISU_UPTS0) | (1u << HFX_GRAD_DISU_UPTS) : (1u << HFX_DISU_UPTS0);
}

bool integral_monitor_reads_gradient(const hfx_ctx *ctx)
{
  for (int m = 0; m < ctx->n_iq; m++)
    if (ctx->iq_ids[m] != 0) return true;
  return false;
}

int sample_integrals(hfx_eles *e, double time, int step)
{
  hfx_ctx *ctx = e->ctx;
  if (ctx->n_iq == 0 || e->n_vol_cubpts == 0) return 0;
  if (prepare_history(e)) return 1;
  IntegralHistory &H = e->integrals;
  HFX_CHECK((int)H.times.size() < H.capacity, "hfx_eles_sample_integral_quantities: the history is full (%d samples); read it "
                                              "(hfx_eles_read_integral_history) before the next sample", H.capacity);
  if (launch_sample(e, (int)H.times.size())) return 1;
  H.times.push_back(time);
  H.steps.push_back(step);
  return 0;
}

int integrals_check_capacity(hfx_eles *const *eles, int neb, int n_steps)
{
  hfx_ctx *ctx = eles[0]->ctx;
  if (!ctx->have_clock || ctx->n_iq == 0 || n_steps <= 0) return 0;
  const long n_new = integral_samples_in(ctx->i_steps, n_steps, ctx->iq_freq);
  for (int i = 0; i < neb; i++)
  {
    if (eles[i]->n_vol_cubpts == 0) continue;
    if (prepare_history(eles[i])) return 1;
    IntegralHistory &H = eles[i]->integrals;
    HFX_CHECK((long)H.times.size() + n_new <= H.capacity,
              "integral monitor: %d steps from step %d take %ld samples (monitor_res_freq %d), the history of %d holds %d already; "
              "read it (hfx_eles_read_integral_history) or take fewer steps per call",
              n_steps, ctx->i_steps, n_new, ctx->iq_freq, H.capacity, (int)H.times.size());
  }
  return 0;
}

} // namespace hfx

using namespace hfx;

extern "C" {

int hfx_ctx_set_integral_monitor(hfx_ctx *ctx, int n_quantities, const int *quantity_ids, int monitor_res_freq, int capacity)
{
  HFX_CHECK(ctx && (n_quantities == 0 || quantity_ids), "hfx_ctx_set_integral_monitor: NULL argument");
  HFX_CHECK(n_quantities >= 0 && n_quantities <= IQ_MAX, "hfx_ctx_set_integral_monitor: %d quantities (at most %d)", n_quantities, IQ_MAX);
  bool grad = false;
  for (int m = 0; m < n_quantities; m++)
  {
    HFX_CHECK(quantity_ids[m] >= 0 && quantity_ids[m] <= 4, "integral diagnostic quantity not recognized"); /* src/eles.cpp:5618 */
    grad = grad || quantity_ids[m] != 0;
  }
  if (n_quantities > 0)
  {
    HFX_CHECK(monitor_res_freq >= 1, "hfx_ctx_set_integral_monitor: monitor_res_freq %d (at least 1)", monitor_res_freq);
    HFX_CHECK(capacity >= 1, "hfx_ctx_set_integral_monitor: a history of %d samples (at least 1)", capacity);
    HFX_CHECK(ctx->have_params, "hfx_ctx_set_integral_monitor: parameters not set");
    // (the reference has one monitor_res_freq for the whole row: history.hip)
    HFX_CHECK(!ctx->hist_on || ctx->hist_freq == monitor_res_freq,
              "hfx_ctx_set_integral_monitor: monitor_res_freq %d, and the history monitor is registered with %d: a row of history.plt has one",
              monitor_res_freq, ctx->hist_freq);
    // the reference has no grad_disu_upts on an inviscid run (src/eles.cpp:5517 reads it unconditionally)
    HFX_CHECK(!grad || ctx->params.viscous, "hfx_ctx_set_integral_monitor: a quantity that reads the gradient (ids 1-4) on an inviscid "
                                            "context, which has no grad_disu_upts; kinetic energy (id 0) alone works there");
  }
  HFX_IMMEDIATE(ctx, 0);
  ctx->n_iq = n_quantities;
  if (n_quantities > 0)
  {
    std::copy(quantity_ids, quantity_ids + n_quantities, ctx->iq_ids);
    ctx->iq_freq = monitor_res_freq;
    ctx->iq_capacity = capacity;
  }
  ctx->iq_epoch++; // (every block makes its history anew, empty, when it is next asked for)
  return 0;
}

int hfx_eles_sample_integral_quantities(hfx_eles *e, double time, int step)
{
  HFX_CHECK(e, "NULL eles");
  hfx_ctx *ctx = e->ctx;
  HFX_CHECK(ctx->n_iq > 0, "hfx_eles_sample_integral_quantities: no quantities (hfx_ctx_set_integral_monitor)");
  HFX_CHECK(e->n_vol_cubpts > 0 && e->opp_volume_cubpts.dense, "hfx_eles_sample_integral_quantities: hfx_eles_set_volume_cubpts was not called");
  const bool grad = integral_monitor_reads_gradient(ctx);
  // (a pending stage runs so that it leaves the gradient when a quantity reads it; with kinetic energy alone fused as it would have)
  HFX_IMMEDIATE(ctx, integral_sample_need(e));
  if (grad) HFX_CHECK_CURRENT(e, HFX_GRAD_DISU_UPTS, "hfx_eles_sample_integral_quantities");
  return sample_integrals(e, time, step);
}

int hfx_eles_integral_count(hfx_eles *e, int *n_samples)
{
  HFX_CHECK(e && n_samples, "hfx_eles_integral_count: NULL argument");
  *n_samples = e->integrals.epoch == e->ctx->iq_epoch ? (int)e->integrals.times.size() : 0;
  return 0;
}

int hfx_eles_read_integral_history(hfx_eles *e, int max_samples, double *times, int *steps, double *values, int *n_samples)
{
  HFX_CHECK(e && n_samples, "hfx_eles_read_integral_history: NULL argument");
  HFX_IMMEDIATE(e->ctx, 0);
  if (prepare_history(e)) return 1;
  IntegralHistory &H = e->integrals;
  const int n = (int)H.times.size();
  HFX_CHECK(n <= max_samples, "hfx_eles_read_integral_history: %d samples are stored, the caller's arrays hold %d", n, max_samples);
  HFX_CHECK(n == 0 || (times && steps && values), "hfx_eles_read_integral_history: NULL argument");
  HFX_HIP(hipStreamSynchronize(e->ctx->stream));
  if (n > 0) HFX_HIP(hipMemcpy(values, H.history, sizeof(double) * (size_t)H.n_quantities * n, hipMemcpyDeviceToHost));
  std::copy(H.times.begin(), H.times.end(), times);
  std::copy(H.steps.begin(), H.steps.end(), steps);
  *n_samples = n;
  H.times.clear();
  H.steps.clear();
  return 0;
}

int hfx_eles_integral_launch(hfx_eles *e, int *n_groups, int *eles_per_pass)
{
  HFX_CHECK(e, "NULL eles");
  IntegralLaunch L;
  if (plan_launch(e, L)) return 1;
  if (n_groups) *n_groups = L.groups;
  if (eles_per_pass) *eles_per_pass = L.epp;
  return 0;
}

int hfx_integral_monitor_samples(int i_steps, int n_steps, int monitor_res_freq, int *n_samples)
{
  HFX_CHECK(n_samples && i_steps >= 0 && monitor_res_freq >= 1, "hfx_integral_monitor_samples: bad argument");
  *n_samples = (int)integral_samples_in(i_steps, n_steps, monitor_res_freq);
  return 0;
}

int hfx_time_integral_quantities(hfx_eles *e, int reps, double *ms)
{
  HFX_CHECK(e && ms && reps > 0, "hfx_time_integral_quantities: bad argument");
  hfx_ctx *ctx = e->ctx;
  HFX_CHECK(ctx->n_iq > 0, "hfx_time_integral_quantities: no quantities (hfx_ctx_set_integral_monitor)");
  HFX_CHECK(e->n_vol_cubpts > 0 && e->opp_volume_cubpts.dense, "hfx_time_integral_quantities: hfx_eles_set_volume_cubpts was not called");
  // (a timing entry point: it reads grad_disu_upts whatever stage wrote it last)
  HFX_IMMEDIATE(ctx, 0);
  if (prepare_history(e)) return 1;
  hipStream_t st = ctx->stream;
  hipEvent_t t0, t1;
  HFX_HIP(hipEventCreate(&t0));
  HFX_HIP(hipEventCreate(&t1));
  int rc = launch_sample(e, e->integrals.capacity); // (warm)
  HFX_HIP(hipEventRecord(t0, st));
  for (int r = 0; r < reps && !rc; r++) rc = launch_sample(e, e->integrals.capacity);
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
