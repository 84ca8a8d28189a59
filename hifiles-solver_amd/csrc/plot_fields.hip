// plot_fields.hip -- the rows of the plot file sampled on the device: per plot point the conserved fields (eles::calc_disu_ppts,
// src/eles.cpp:3757), the time averages (calc_time_average_ppts, :3820) and run_input.diagnostic_fields (calc_grad_disu_ppts :3781,
// calc_sensor_ppts :3848, calc_diagnostic_fields_ppts :3858-4006), which output::write_tec / write_vtu print every plot_freq steps
// (src/HiFiLES.cpp:273-285).  gfx950 only.
//
// One fused kernel per block and snapshot, in the shape of integrals.hip: a workgroup walks passes of `epp` consecutive elements in a
// persistent grid-stride loop and stages ONE slab at a time in LDS -- the state, then (vorticity or a Q criterion selected) the
// conservative gradient with respect to each dimension in turn, without the energy's, which no field reads, then the average fields
// in groups of n_fields.  The slab lies element-fastest: the lanes of one element read one address (a broadcast), those of
// neighbouring elements neighbouring doubles, so no read of the contraction has a bank conflict.  A lane owns one plot point of one
// element of the pass; where an element has more plot points than the workgroup lanes, the lanes take them in several passes, each of
// which stages the slabs again (they come from L2 then).  The lane's dot products against the dense (n_ppts, n_upts) operator run over
// the columns in ascending order, as the reference's dgemm does (src/funcs.cpp:49-123).  The interpolated state (n_fields doubles) and
// the velocity gradient (n_dims^2 doubles, formed slab by slab) stay in registers; nothing of the size n_ppts x n_eles x n_fields x
// n_dims is written.  Ordinary stores, no atomics: a snapshot is a function of the state, the registered arrays and nothing else.
//
// Which gradient: grad_disu_upts as it stands, like the reference and like the integral monitor.  Behind a step that is what the last
// stage's correct_gradient left -- the gradient of that stage's INPUT state, paired with the state after the step.  The step loops see
// to it that the array holds exactly that when they sample (stage_call_by_call); the monitor forms no gradient of its own.
#include "step_loop.hpp"
#include "plot_point.hpp"

namespace hfx
{

constexpr int PF_THREADS = 256;    // lanes of a workgroup
constexpr int PF_LDS_PASS = 32768; // bytes of LDS a pass of several elements may take (one slab)
constexpr int PF_LDS_MOST = 65536; // and one element alone
constexpr int PF_GROUPS_PER_CU = 4;

// by value in the kernel's argument segment
struct PlotArgs
{
  const double *disu_upts;      // (n_upts, n_eles, n_fields): disu_upts(0)
  const double *grad_disu_upts; // (n_upts, n_eles, n_fields, n_dims); read when need_grad only
  const double *average;        // (n_upts, n_eles, n_average): disu_average_upts; read when n_average > 0 only
  const double *sensor;         // (n_eles); read when need_sensor only
  const double *opp;            // (n_ppts, n_upts) column-major
  double *out;                  // (n_ppts, n_eles, n_fields + n_average + n_diag) of this snapshot
  long n_eles;
  int n_upts, n_ppts;
  int epp;                      // elements of a pass: epp * min(n_ppts, PF_THREADS) <= PF_THREADS
  int n_average, n_diag, need_grad, need_sensor;
  int codes[PF_MAX_DIAG];
  double gamma;
};

// the slab of `nfl` field planes of the pass's `cnt` elements from i0 on: slab[(f * n_upts + k) * epp + element]
__device__ inline void pf_stage(double *slab, const double *src, long P, int nfl, int n_upts, int epp, int cnt)
{
  __syncthreads(); // (the slab before this one has been read)
  for (int f = 0; f < nfl; f++)
    for (int idx = threadIdx.x; idx < cnt * n_upts; idx += PF_THREADS)
    {
      const int el = idx / n_upts, k = idx - el * n_upts;
      slab[(size_t)(f * n_upts + k) * epp + el] = src[f * P + idx];
    }
  __syncthreads();
}

// v[f] = sum_k opp(j, k) slab(f, k, the lane's element), f < NFL, k ascending
template <int NFL, int NF>
__device__ inline void pf_contract(const double *row, int n_ppts, int n_upts, const double *us, int epp, double (&v)[NF])
{
#pragma unroll
  for (int f = 0; f < NF; f++) v[f] = 0.0;
  for (int k = 0; k < n_upts; k++)
  {
    const double c = row[(long)n_ppts * k];
#pragma unroll
    for (int f = 0; f < NFL; f++) v[f] += c * us[(size_t)(f * n_upts + k) * epp];
  }
}

template <int ND>
__global__ __launch_bounds__(PF_THREADS) void plot_fields_kernel(const PlotArgs A)
{
  constexpr int NF = ND + 2;
  extern __shared__ __align__(16) double slab[]; // (NF, n_upts, epp), the element index fastest
  const int tid = threadIdx.x;
  const int epp = A.epp;
  const long P = (long)A.n_upts * A.n_eles;  // a field plane of the solution-point arrays
  const long PP = (long)A.n_ppts * A.n_eles; // and of the plot-point output
  const bool several = A.n_ppts > PF_THREADS; // (then epp is 1 and the lanes take the element's points in passes)

  for (long i0 = (long)blockIdx.x * epp; i0 < A.n_eles; i0 += (long)gridDim.x * epp)
  {
    const int cnt = (int)min((long)epp, A.n_eles - i0);
    for (int p0 = 0; p0 < (several ? A.n_ppts : 1); p0 += PF_THREADS)
    {
      // the lane's element of the pass and its plot point
      const int g = several ? 0 : tid / A.n_ppts;
      const int j = several ? p0 + tid : tid - g * A.n_ppts;
      const bool lane_on = g < cnt && j < A.n_ppts;
      const double *row = A.opp + j, *us = slab + g;
      double *dst = A.out + (i0 + g) * A.n_ppts + j;
      double u[NF], dv[ND][ND], v[NF];
#pragma unroll
      for (int a = 0; a < ND; a++)
#pragma unroll
        for (int b = 0; b < ND; b++) dv[a][b] = 0.0;

      pf_stage(slab, A.disu_upts + i0 * A.n_upts, P, NF, A.n_upts, epp, cnt);
      if (lane_on)
      {
        pf_contract<NF, NF>(row, A.n_ppts, A.n_upts, us, epp, u);
#pragma unroll
        for (int f = 0; f < NF; f++) dst[PP * f] = u[f];
      }
      if (A.need_grad) // (uniform over the workgroup)
      {
#pragma unroll
        for (int d = 0; d < ND; d++)
        {
          pf_stage(slab, A.grad_disu_upts + P * NF * d + i0 * A.n_upts, P, NF - 1, A.n_upts, epp, cnt);
          if (lane_on)
          {
            pf_contract<NF - 1, NF>(row, A.n_ppts, A.n_upts, us, epp, v);
            pf_velocity_gradient<ND>(u, v, d, dv);
          }
        }
      }
      for (int c0 = 0; c0 < A.n_average; c0 += NF)
      {
        const int nfl = min(NF, A.n_average - c0);
        pf_stage(slab, A.average + P * c0 + i0 * A.n_upts, P, nfl, A.n_upts, epp, cnt);
        if (lane_on)
        {
          // (planes past nfl hold what an earlier slab left: they are contracted and not stored)
          pf_contract<NF, NF>(row, A.n_ppts, A.n_upts, us, epp, v);
#pragma unroll
          for (int f = 0; f < NF; f++)
            if (f < nfl) dst[PP * (NF + c0 + f)] = v[f];
        }
      }
      if (lane_on)
      {
        const double sensor = A.need_sensor ? A.sensor[i0 + g] : 0.0;
        for (int m = 0; m < A.n_diag; m++) dst[PP * (NF + A.n_average + m)] = pf_diagnostic<ND>(A.codes[m], u, dv, A.gamma, sensor);
      }
    }
  }
}

// what a snapshot launches for the block as it stands
struct PlotLaunch
{
  int epp = 0, groups = 0, ppts_per_pass = 0;
  size_t lds = 0;
};
static int plan_launch(const hfx_eles *e, PlotLaunch &L)
{
  const int np = e->n_ppts;
  HFX_CHECK(np > 0 && e->opp_p.dense, "plot monitor: hfx_eles_set_opp_p was not called");
  const size_t per_ele = sizeof(double) * (size_t)e->n_upts * e->n_fields; // one slab of one element
  HFX_CHECK(per_ele <= (size_t)PF_LDS_MOST, "plot monitor: %d solution points of %d fields do not fit the kernel's %d bytes of LDS", e->n_upts,
            e->n_fields, PF_LDS_MOST);
  L.ppts_per_pass = std::min(np, PF_THREADS);
  L.epp = np > PF_THREADS ? 1 : (int)std::max<size_t>(1, std::min<size_t>((size_t)(PF_THREADS / np), (size_t)PF_LDS_PASS / per_ele));
  L.lds = per_ele * L.epp;
  const long passes = std::max<long>(1, (e->n_eles + L.epp - 1) / L.epp);
  long groups = std::min<long>(passes, (long)PF_GROUPS_PER_CU * e->ctx->n_cu);
  const int cap = e->ctx->opt.persistent_grid_cap;
  if (cap > 0) groups = std::min<long>(groups, cap);
  L.groups = (int)groups;
  return 0;
}

static bool monitor_reads(const hfx_ctx *ctx, bool (*what)(int))
{
  for (int m = 0; m < ctx->n_plot_diag; m++)
    if (what(ctx->plot_codes[m])) return true;
  return false;
}
static bool reads_sensor(int code) { return code == PF_SENSOR; }

bool plot_monitor_reads_gradient(const hfx_eles *e)
{
  const hfx_ctx *ctx = e->ctx;
  return ctx->plot_on && ctx->params.viscous && e->n_ppts > 0 && monitor_reads(ctx, pf_reads_gradient);
}

// everything that refuses a snapshot of this block whatever its state, with the reference's messages (src/eles.cpp:3933, :3988): asked
// by the loops before their first launch and by every entry point
static int check_block(const hfx_eles *e, const char *who)
{
  const hfx_ctx *ctx = e->ctx;
  HFX_CHECK(ctx->have_params, "parameters not set");
  HFX_CHECK(e->n_fields == e->n_dims + 2 && (e->n_dims == 2 || e->n_dims == 3), "%s: a block of %d fields in %d dimensions", who, e->n_fields,
            e->n_dims);
  for (int m = 0; m < ctx->n_plot_diag; m++)
  {
    const int c = ctx->plot_codes[m];
    HFX_CHECK(e->n_dims == 3 || (c != PF_Q_CRITERION && c != PF_SCALED_Q_CRITERION), "%s: Q criterion Not implemented in 2D", who);
    HFX_CHECK(c != PF_SENSOR || e->shock_ready, "%s: Sensor unavailable (the block has no shock capturing, hfx_eles_set_shock_capture)", who);
  }
  PlotLaunch L;
  return plan_launch(e, L);
}

// the block's history as the context's monitor and the block's registrations want it: made anew, empty, when either has changed
static int prepare_history(hfx_eles *e)
{
  hfx_ctx *ctx = e->ctx;
  PlotHistory &H = e->plot;
  const int n_out = ctx->plot_on ? e->n_fields + e->n_average_fields + ctx->n_plot_diag : 0;
  const bool same = H.epoch == ctx->plot_epoch && H.n_ppts == e->n_ppts && H.n_average == e->n_average_fields && H.n_out == n_out;
  if (same && (H.history || !ctx->plot_on)) return 0;
  HFX_HIP(hipStreamSynchronize(ctx->stream)); // (a snapshot into the history that goes may still be running)
  H.times.clear();
  H.steps.clear();
  H.history.reset();
  H.scratch.reset();
  H.n_ppts = e->n_ppts;
  H.n_average = e->n_average_fields;
  H.n_out = n_out;
  H.capacity = 0;
  H.epoch = ctx->plot_epoch;
  if (!ctx->plot_on || e->n_ppts == 0) return 0;
  if (H.history.alloc((size_t)e->n_ppts * e->n_eles * n_out * ctx->plot_capacity)) return 1;
  H.capacity = ctx->plot_capacity;
  return 0;
}

// the launch of one snapshot into `out` (check_block and prepare_history have run)
static int launch_snapshot(hfx_eles *e, double *out)
{
  hfx_ctx *ctx = e->ctx;
  if (e->n_eles == 0) return 0;
  PlotLaunch L;
  if (plan_launch(e, L)) return 1;
  const bool grad = plot_monitor_reads_gradient(e), sensor = monitor_reads(ctx, reads_sensor);
  HFX_CHECK(e->arr[HFX_DISU_UPTS0], "plot monitor: the solution was never uploaded");
  HFX_CHECK(!grad || e->arr[HFX_GRAD_DISU_UPTS], "plot monitor: no gradient has been computed yet");
  HFX_CHECK(!sensor || e->arr[HFX_SENSOR], "plot monitor: no sensor has been computed yet (hfx_eles_shock_capture)");
  PlotArgs A{};
  A.disu_upts = e->arr[HFX_DISU_UPTS0];
  A.grad_disu_upts = grad ? e->arr[HFX_GRAD_DISU_UPTS].get() : nullptr;
  A.average = e->n_average_fields > 0 ? e->disu_average_upts.get() : nullptr;
  A.sensor = sensor ? e->arr[HFX_SENSOR].get() : nullptr;
  A.opp = e->opp_p.dense;
  A.out = out;
  A.n_eles = e->n_eles;
  A.n_upts = e->n_upts;
  A.n_ppts = e->n_ppts;
  A.epp = L.epp;
  A.n_average = e->n_average_fields;
  A.n_diag = ctx->n_plot_diag;
  A.need_grad = grad;
  A.need_sensor = sensor;
  for (int m = 0; m < ctx->n_plot_diag; m++) A.codes[m] = ctx->plot_codes[m];
  A.gamma = ctx->params.gamma;
  const dim3 grid(L.groups), block(PF_THREADS);
  if (e->n_dims == 3)
    hipLaunchKernelGGL(plot_fields_kernel<3>, grid, block, L.lds, ctx->stream, A);
  else
    hipLaunchKernelGGL(plot_fields_kernel<2>, grid, block, L.lds, ctx->stream, A);
  HFX_HIP(hipGetLastError());
  return 0;
}

static size_t snapshot_size(const hfx_eles *e) { return (size_t)e->n_ppts * e->n_eles * e->plot.n_out; }

int sample_plot(hfx_eles *e, double time, int step)
{
  hfx_ctx *ctx = e->ctx;
  if (!ctx->plot_on || e->n_ppts == 0) return 0;
  if (check_block(e, "hfx_eles_sample_plot") || prepare_history(e)) return 1;
  PlotHistory &H = e->plot;
  HFX_CHECK((int)H.times.size() < H.capacity, "hfx_eles_sample_plot: the history is full (%d snapshots); read it "
                                              "(hfx_eles_read_plot_snapshots) before the next sample", H.capacity);
  if (launch_snapshot(e, H.history + snapshot_size(e) * H.times.size())) return 1;
  H.times.push_back(time);
  H.steps.push_back(step);
  return 0;
}

int plot_check_capacity(hfx_eles *const *eles, int neb, int n_steps)
{
  hfx_ctx *ctx = eles[0]->ctx;
  if (!ctx->have_clock || !ctx->plot_on || n_steps <= 0) return 0;
  const long n_new = plot_samples_in(ctx->i_steps, n_steps, ctx->plot_freq);
  for (int i = 0; i < neb; i++)
  {
    if (eles[i]->n_ppts == 0) continue;
    if (check_block(eles[i], "plot monitor") || prepare_history(eles[i])) return 1;
    PlotHistory &H = eles[i]->plot;
    HFX_CHECK((long)H.times.size() + n_new <= H.capacity,
              "plot monitor: %d steps from step %d take %ld snapshots (plot_freq %d), the history of %d holds %d already; "
              "read it (hfx_eles_read_plot_snapshots) or take fewer steps per call",
              n_steps, ctx->i_steps, n_new, ctx->plot_freq, H.capacity, (int)H.times.size());
  }
  return 0;
}

// what a direct entry point asks of a pending deferred stage: the state, and what the selected fields read beside it
static unsigned need_mask(const hfx_eles *e)
{
  unsigned need = 1u << HFX_DISU_UPTS0;
  if (plot_monitor_reads_gradient(e)) need |= 1u << HFX_GRAD_DISU_UPTS;
  if (monitor_reads(e->ctx, reads_sensor)) need |= 1u << HFX_SENSOR;
  return need;
}

unsigned plot_sample_need(const hfx_eles *e) { return e->ctx->plot_on && e->n_ppts > 0 ? need_mask(e) : 0; }

} // namespace hfx

using namespace hfx;

extern "C" {

int hfx_ctx_set_plot_monitor(hfx_ctx *ctx, int n_diag, const int *codes, int plot_freq, int capacity)
{
  HFX_CHECK(ctx && (n_diag == 0 || codes), "hfx_ctx_set_plot_monitor: NULL argument");
  HFX_CHECK(n_diag >= 0 && n_diag <= PF_MAX_DIAG, "hfx_ctx_set_plot_monitor: %d diagnostic fields (at most %d)", n_diag, PF_MAX_DIAG);
  if (capacity != 0)
  {
    HFX_CHECK(capacity >= 1, "hfx_ctx_set_plot_monitor: a history of %d snapshots (at least 1, or 0 for no monitor)", capacity);
    HFX_CHECK(plot_freq >= 1, "hfx_ctx_set_plot_monitor: plot_freq %d (at least 1)", plot_freq);
    HFX_CHECK(ctx->have_params, "hfx_ctx_set_plot_monitor: parameters not set");
    for (int m = 0; m < n_diag; m++)
    {
      HFX_CHECK(codes[m] >= 0 && codes[m] < PF_N_FIELDS, "hfx_ctx_set_plot_monitor: plot_quantity %d: plot_quantity not recognized", codes[m]); /* src/eles.cpp:3994 */
      HFX_CHECK(!pf_reads_gradient(codes[m]) || ctx->params.viscous,
                "hfx_ctx_set_plot_monitor: Trying to calculate diagnostic field only supported by viscous simualtion"); /* src/eles.cpp:3916 */
    }
  }
  HFX_IMMEDIATE(ctx, 0);
  ctx->plot_on = capacity != 0;
  ctx->n_plot_diag = 0;
  if (ctx->plot_on)
  {
    ctx->n_plot_diag = n_diag;
    std::copy(codes, codes + n_diag, ctx->plot_codes);
    ctx->plot_freq = plot_freq;
    ctx->plot_capacity = capacity;
  }
  ctx->plot_epoch++; // (every block makes its history anew, empty, when it is next asked for)
  return 0;
}

int hfx_eles_sample_plot(hfx_eles *e, double time, int step)
{
  HFX_CHECK(e, "NULL eles");
  hfx_ctx *ctx = e->ctx;
  HFX_CHECK(ctx->plot_on, "hfx_eles_sample_plot: no monitor (hfx_ctx_set_plot_monitor)");
  HFX_CHECK(e->n_ppts > 0, "hfx_eles_sample_plot: hfx_eles_set_opp_p was not called");
  if (check_block(e, "hfx_eles_sample_plot")) return 1;
  // (a pending stage runs so that it leaves the gradient when a field reads it; with gradient-free fields fused as it would have)
  HFX_IMMEDIATE(ctx, need_mask(e));
  if (plot_monitor_reads_gradient(e)) HFX_CHECK_CURRENT(e, HFX_GRAD_DISU_UPTS, "hfx_eles_sample_plot");
  return sample_plot(e, time, step);
}

int hfx_eles_plot_count(hfx_eles *e, int *n_snapshots)
{
  HFX_CHECK(e && n_snapshots, "hfx_eles_plot_count: NULL argument");
  *n_snapshots = e->plot.epoch == e->ctx->plot_epoch ? (int)e->plot.times.size() : 0;
  return 0;
}

int hfx_eles_plot_width(hfx_eles *e, int *n_out)
{
  HFX_CHECK(e && n_out, "hfx_eles_plot_width: NULL argument");
  *n_out = e->ctx->plot_on ? e->n_fields + e->n_average_fields + e->ctx->n_plot_diag : 0;
  return 0;
}

int hfx_eles_read_plot_snapshots(hfx_eles *e, int max_snapshots, double *times, int *steps, double *values, int *n_snapshots)
{
  HFX_CHECK(e && n_snapshots, "hfx_eles_read_plot_snapshots: NULL argument");
  HFX_IMMEDIATE(e->ctx, 0);
  if (prepare_history(e)) return 1;
  PlotHistory &H = e->plot;
  const int n = (int)H.times.size();
  HFX_CHECK(n <= max_snapshots, "hfx_eles_read_plot_snapshots: %d snapshots are stored, the caller's arrays hold %d", n, max_snapshots);
  HFX_CHECK(n == 0 || (times && steps && values), "hfx_eles_read_plot_snapshots: NULL argument");
  HFX_HIP(hipStreamSynchronize(e->ctx->stream));
  if (n > 0 && snapshot_size(e) > 0) HFX_HIP(hipMemcpy(values, H.history, sizeof(double) * snapshot_size(e) * n, hipMemcpyDeviceToHost));
  std::copy(H.times.begin(), H.times.end(), times);
  std::copy(H.steps.begin(), H.steps.end(), steps);
  *n_snapshots = n;
  H.times.clear();
  H.steps.clear();
  return 0;
}

// the scratch snapshot of the entry points that leave the history alone
static int ensure_scratch(hfx_eles *e)
{
  if (prepare_history(e)) return 1;
  const size_t n = snapshot_size(e);
  return e->plot.scratch.size() == std::max<size_t>(n, 1) ? 0 : e->plot.scratch.alloc(n);
}

int hfx_eles_calc_plot_fields(hfx_eles *e, double *host)
{
  HFX_CHECK(e && host, "hfx_eles_calc_plot_fields: NULL argument");
  hfx_ctx *ctx = e->ctx;
  HFX_CHECK(ctx->plot_on, "hfx_eles_calc_plot_fields: no monitor (hfx_ctx_set_plot_monitor)");
  HFX_CHECK(e->n_ppts > 0, "hfx_eles_calc_plot_fields: hfx_eles_set_opp_p was not called");
  if (check_block(e, "hfx_eles_calc_plot_fields")) return 1;
  HFX_IMMEDIATE(ctx, need_mask(e));
  if (plot_monitor_reads_gradient(e)) HFX_CHECK_CURRENT(e, HFX_GRAD_DISU_UPTS, "hfx_eles_calc_plot_fields");
  if (e->n_eles == 0) return 0;
  if (ensure_scratch(e) || launch_snapshot(e, e->plot.scratch)) return 1;
  HFX_HIP(hipMemcpyAsync(host, e->plot.scratch, sizeof(double) * snapshot_size(e), hipMemcpyDeviceToHost, ctx->stream));
  HFX_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int hfx_eles_plot_launch(hfx_eles *e, int *n_groups, int *eles_per_pass, int *ppts_per_pass)
{
  HFX_CHECK(e, "NULL eles");
  PlotLaunch L;
  if (plan_launch(e, L)) return 1;
  if (n_groups) *n_groups = L.groups;
  if (eles_per_pass) *eles_per_pass = L.epp;
  if (ppts_per_pass) *ppts_per_pass = L.ppts_per_pass;
  return 0;
}

int hfx_plot_monitor_samples(int i_steps, int n_steps, int plot_freq, int *n_samples)
{
  HFX_CHECK(n_samples && i_steps >= 0 && plot_freq >= 1, "hfx_plot_monitor_samples: bad argument");
  *n_samples = (int)plot_samples_in(i_steps, n_steps, plot_freq);
  return 0;
}

int hfx_plot_point_fields(int n_dims, const double *u, const double *grad, double gamma, double sensor, int n_diag, const int *codes,
                          double *out)
{
  HFX_CHECK(u && out && (n_diag == 0 || codes) && (n_dims == 2 || n_dims == 3), "hfx_plot_point_fields: bad argument");
  bool reads = false;
  for (int m = 0; m < n_diag; m++)
  {
    HFX_CHECK(codes[m] >= 0 && codes[m] < PF_N_FIELDS, "hfx_plot_point_fields: plot_quantity %d: plot_quantity not recognized", codes[m]);
    HFX_CHECK(n_dims == 3 || (codes[m] != PF_Q_CRITERION && codes[m] != PF_SCALED_Q_CRITERION), "hfx_plot_point_fields: Q criterion Not implemented in 2D");
    reads = reads || pf_reads_gradient(codes[m]);
  }
  HFX_CHECK(!reads || grad, "hfx_plot_point_fields: a field reads the gradient, and none was given");
  const int nf = n_dims + 2;
  if (n_dims == 3)
  {
    double dv[3][3] = {};
    if (reads)
      for (int d = 0; d < 3; d++) pf_velocity_gradient<3>(u, grad + nf * d, d, dv);
    for (int m = 0; m < n_diag; m++) out[m] = pf_diagnostic<3>(codes[m], u, dv, gamma, sensor);
  }
  else
  {
    double dv[2][2] = {};
    if (reads)
      for (int d = 0; d < 2; d++) pf_velocity_gradient<2>(u, grad + nf * d, d, dv);
    for (int m = 0; m < n_diag; m++) out[m] = pf_diagnostic<2>(codes[m], u, dv, gamma, sensor);
  }
  return 0;
}

int hfx_time_plot_fields(hfx_eles *e, int reps, double *ms)
{
  HFX_CHECK(e && ms && reps > 0, "hfx_time_plot_fields: bad argument");
  hfx_ctx *ctx = e->ctx;
  HFX_CHECK(ctx->plot_on, "hfx_time_plot_fields: no monitor (hfx_ctx_set_plot_monitor)");
  HFX_CHECK(e->n_ppts > 0, "hfx_time_plot_fields: hfx_eles_set_opp_p was not called");
  if (check_block(e, "hfx_time_plot_fields")) return 1;
  // (a timing entry point: it reads grad_disu_upts whatever stage wrote it last)
  HFX_IMMEDIATE(ctx, 0);
  if (ensure_scratch(e)) return 1;
  hipStream_t st = ctx->stream;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  float t = 0.f;
  // (no early return between the creation of the events and their destruction)
  hipError_t err = hipEventCreate(&t0);
  if (err == hipSuccess) err = hipEventCreate(&t1);
  int rc = err == hipSuccess ? launch_snapshot(e, e->plot.scratch) : 1; // (warm)
  if (err == hipSuccess) err = hipEventRecord(t0, st);
  for (int r = 0; r < reps && !rc && err == hipSuccess; r++) rc = launch_snapshot(e, e->plot.scratch);
  if (err == hipSuccess) err = hipEventRecord(t1, st);
  if (err == hipSuccess) err = hipEventSynchronize(t1);
  if (err == hipSuccess) err = hipEventElapsedTime(&t, t0, t1);
  if (t0) (void)hipEventDestroy(t0);
  if (t1) (void)hipEventDestroy(t1);
  HFX_CHECK(err == hipSuccess, "hfx_time_plot_fields: %s", hipGetErrorString(err));
  *ms = t / reps;
  return rc;
}

} // extern "C"
