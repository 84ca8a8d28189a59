// history.hip -- the residual norms and the wall forces of history.plt sampled on the device: the columns the reference fills
// every monitor_res_freq steps and at step 1 in front of the Diagnostics[...] ones (src/HiFiLES.cpp:247-266; output::CalcNormResidual,
// src/output.cpp:2166-2248; eles::compute_res_upts, src/eles.cpp:5045-5074; output::CalcForces, src/output.cpp:1915-2014).
// gfx950 only.
//
// The residual: one fused kernel per block and sample for ALL fields and the chosen norm, a streaming reduction over the solution
// points of div_tconf_upts(0) / detjac_upts - src_upts.  A lane owns HR_POINTS consecutive points of every plane in a persistent
// grid-stride loop: it reads their detjac once and serves every field from it -- n_fields + 1 (+ n_fields with a source) doubles per
// point.  The lane's first point is a multiple of HR_POINTS, so the detjac is read as 16-byte words; a field's plane begins n_upts x
// n_eles doubles behind the one before, 8 bytes off a 16-byte boundary for every other plane when that product is odd (3^3 P2
// hexahedra): there the lane reads an 8-byte head, a 16-byte middle and an 8-byte tail.  The last item of a plane is read point by
// point.  Nothing is written but one partial per workgroup and field.
//
// The forces: wall_force_kernel as hfx_eles_compute_wall_forces launches it (wall_force.hip), whose per-workgroup partials stay on
// the device.
//
// Reproducible: lanes are combined by a butterfly of cross-lane shuffles, waves by one lane in wave order, and a second launch of
// one workgroup combines the workgroups' partials in workgroup order -- the order of the host loops of hfx_eles_compute_res_upts
// and hfx_eles_compute_wall_forces -- into the slot's row.  Ordinary stores only, no floating-point atomics: a row is a function of
// the arrays and the grid, whatever its slot.  Norm 0 combines by a maximum that keeps a NaN (fmax would drop it): the reference
// stops on a NaN residual whatever the norm (src/output.cpp:2243).
//
// Which gradient the viscous force reads: grad_disu_upts as it stands, as for the integral monitor (integrals.hip).  The step loops
// see to it that it is what the last RK stage left (stage_call_by_call); the monitor forms no gradient of its own.
#include "step_loop.hpp"

#include <cstdint>

namespace hfx
{

// by value in the kernel's argument segment
struct ResidualArgs
{
  const double *div;    // (n_upts, n_eles, n_fields): div_tconf_upts(0)
  const double *detjac; // (n_upts, n_eles)
  const double *src;    // (n_upts, n_eles, n_fields), or nullptr: no source term
  double *partial;      // (n_groups, n_fields): [group + n_groups * field]
  long P;               // n_upts * n_eles, the length of one field plane
  int norm;             // run_input.res_norm_type: 0 max |r|, 1 sum |r|, 2 sum r^2
};

constexpr int HR_THREADS = 256;
constexpr int HR_POINTS = 4;        // consecutive points of a lane per pass
constexpr int HR_GROUPS_PER_CU = 4; // workgroups per CU of the grid

// the larger of two residuals, a NaN before either
__device__ inline double hr_max(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ inline double hr_combine(int norm, double a, double b) { return norm == 0 ? hr_max(a, b) : a + b; }

// cnt <= HR_POINTS consecutive doubles from p (8-byte aligned); a whole item as 16-byte words where the address allows
__device__ inline void hr_load(const double *p, int cnt, double (&v)[HR_POINTS])
{
  if (cnt == HR_POINTS)
  {
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0)
    {
      const double2 a = *reinterpret_cast<const double2 *>(p), b = *reinterpret_cast<const double2 *>(p + 2);
      v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    }
    else
    {
      // (p + 1 is on a 16-byte boundary)
      const double2 m = *reinterpret_cast<const double2 *>(p + 1);
      v[0] = p[0]; v[1] = m.x; v[2] = m.y; v[3] = p[3];
    }
  }
  else
  {
#pragma unroll
    for (int w = 0; w < HR_POINTS; w++) v[w] = w < cnt ? p[w] : 1.0;
  }
}

template <int NF>
__global__ __launch_bounds__(HR_THREADS) void residual_norm_kernel(const ResidualArgs A)
{
  static_assert(HR_POINTS == 4, "hr_load reads items of four points");
  __shared__ double wave_acc[(HR_THREADS / 64) * NF];
  const int tid = threadIdx.x;
  const long n_items = (A.P + HR_POINTS - 1) / HR_POINTS;
  double acc[NF];
#pragma unroll
  for (int f = 0; f < NF; f++) acc[f] = 0.0;

  for (long it = (long)blockIdx.x * HR_THREADS + tid; it < n_items; it += (long)gridDim.x * HR_THREADS)
  {
    const long q = it * HR_POINTS;
    const int cnt = (int)min((long)HR_POINTS, A.P - q);
    double dj[HR_POINTS];
    hr_load(A.detjac + q, cnt, dj);
#pragma unroll
    for (int f = 0; f < NF; f++)
    {
      double d[HR_POINTS], s[HR_POINTS];
      hr_load(A.div + f * A.P + q, cnt, d);
      if (A.src) hr_load(A.src + f * A.P + q, cnt, s); // (uniform over the grid)
#pragma unroll
      for (int w = 0; w < HR_POINTS; w++)
      {
        // (the operations of res_partial_kernel: an IEEE division, then the source)
        const double r = d[w] / dj[w] - (A.src ? s[w] : 0.0);
        const double t = A.norm == 2 ? r * r : fabs(r);
        if (w < cnt) acc[f] = hr_combine(A.norm, acc[f], t);
      }
    }
  }

  // lane l with lane l ^ 32, ^ 16, ... ^ 1, then the waves in their order
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int f = 0; f < NF; f++)
  {
    double a = acc[f];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a = hr_combine(A.norm, a, __shfl_xor(a, off, 64));
    if (lane == 0) wave_acc[wave * NF + f] = a;
  }
  __syncthreads();
  if (tid < NF)
  {
    double s = 0.0;
    for (int wv = 0; wv < HR_THREADS / 64; wv++) s = hr_combine(A.norm, s, wave_acc[wv * NF + tid]);
    A.partial[blockIdx.x + (size_t)gridDim.x * tid] = s;
  }
}

// one workgroup: row[f] = the residual partials of field f combined in workgroup order, row[nf + q] = the wall-force partials of
// quantity q added in workgroup order (zeros without groups: a block without wall faces)
// The partials pass through LDS HF_THREADS workgroups at a time -- every thread fetches one workgroup's value of every quantity, the
// loads coalesced and in flight together -- and thread m walks quantity m's chunk in order, so that no lane waits for a thousand
// dependent loads from memory
constexpr int HF_THREADS = 256;
constexpr int HF_MAX_Q = 5 + 8; // n_fields + 2 n_dims + 2 in three dimensions
__global__ __launch_bounds__(HF_THREADS) void history_finish_kernel(const double *res_partial, int n_res_groups, int nf, int norm,
                                                                    const double *force_partial, int n_force_groups, int nq, double *row)
{
  __shared__ double chunk[HF_MAX_Q][HF_THREADS + 1]; // (+ 1: the lanes that walk the rows read different banks)
  const int tid = threadIdx.x;
  const bool mine = tid < nf + nq, res = tid < nf;
  const int most = max(n_res_groups, n_force_groups);
  double s = 0.0;
  for (int b0 = 0; b0 < most; b0 += HF_THREADS)
  {
    const int b = b0 + tid;
    for (int m = 0; m < nf; m++)
      if (b < n_res_groups) chunk[m][tid] = res_partial[b + (size_t)n_res_groups * m];
    for (int q = 0; q < nq; q++)
      if (b < n_force_groups) chunk[nf + q][tid] = force_partial[b + (size_t)n_force_groups * q];
    __syncthreads();
    if (mine)
    {
      const int n = min(HF_THREADS, (res ? n_res_groups : n_force_groups) - b0); // (may be <= 0: this kind has fewer workgroups)
      // (sixteen LDS reads in flight at a time: one read per dependent add left the lane waiting out the LDS latency a thousand times)
      int k = 0;
      for (; k + 16 <= n; k += 16)
      {
        double v[16];
#pragma unroll
        for (int j = 0; j < 16; j++) v[j] = chunk[tid][k + j];
#pragma unroll
        for (int j = 0; j < 16; j++) s = res ? hr_combine(norm, s, v[j]) : s + v[j];
      }
      for (; k < n; k++) s = res ? hr_combine(norm, s, chunk[tid][k]) : s + chunk[tid][k];
    }
    __syncthreads();
  }
  if (mine) row[tid] = s;
}

// the workgroups of the residual kernel for the block as it stands
static int plan_groups(const hfx_eles *e)
{
  const long P = (long)e->n_upts * e->n_eles;
  const long items = (P + HR_POINTS - 1) / HR_POINTS;
  long groups = std::min<long>(std::max<long>(1, (items + HR_THREADS - 1) / HR_THREADS), (long)HR_GROUPS_PER_CU * e->ctx->n_cu);
  const int cap = e->ctx->opt.persistent_grid_cap;
  if (cap > 0) groups = std::min<long>(groups, cap);
  return (int)groups;
}

static bool block_has_walls(const hfx_eles *e) { return e->wall_forces && e->wall_forces->n_faces > 0; }

// the block's history as the context's monitor wants it: made anew, empty, when the monitor has changed since
static int prepare_history(hfx_eles *e)
{
  hfx_ctx *ctx = e->ctx;
  HistoryRows &H = e->history_rows;
  if (H.rows && H.epoch == ctx->hist_epoch) return 0;
  HFX_HIP(hipStreamSynchronize(ctx->stream)); // (a sample into the history that goes may still be running)
  H.times.clear();
  H.steps.clear();
  H.rows.reset();
  H.n_res = H.n_force = H.capacity = 0;
  H.epoch = ctx->hist_epoch;
  if (!ctx->hist_on) return 0;
  const int n_force = ctx->hist_forces ? 2 * e->n_dims + 2 : 0;
  if (H.rows.alloc_zeroed((size_t)(e->n_fields + n_force) * ((size_t)ctx->hist_capacity + 1))) return 1;
  H.n_res = e->n_fields;
  H.n_force = n_force;
  H.capacity = ctx->hist_capacity;
  return 0;
}

// everything that refuses a sample of the block as it stands, before anything is launched; leaves the wall-force launch prepared
static int check_sample(hfx_eles *e, const char *who)
{
  hfx_ctx *ctx = e->ctx;
  HFX_CHECK(ctx->have_params, "parameters not set");
  HFX_CHECK(e->n_fields == e->n_dims + 2 && (e->n_dims == 2 || e->n_dims == 3), "%s: a block of %d fields in %d dimensions", who,
            e->n_fields, e->n_dims);
  if (e->n_eles == 0) return 0;
  HFX_CHECK(e->arr[HFX_DIV_TCONF_UPTS], "%s: no residual has been computed yet", who);
  HFX_CHECK(!(e->stale & (1u << HFX_DIV_TCONF_UPTS)),
            "compute_res_upts: div_tconf_upts was not stored by the fused stage that ran last (deferred execution stores it at the last "
            "stage of a step, or when asked before the next stage begins)");
  if (ctx->hist_forces && block_has_walls(e) && wall_force_partials_prepare(e, who)) return 1;
  return 0;
}

// the launches of one row into slot `slot` (prepare_history and check_sample have run)
static int launch_sample(hfx_eles *e, int slot)
{
  hfx_ctx *ctx = e->ctx;
  HistoryRows &H = e->history_rows;
  hipStream_t st = ctx->stream;
  const int n_groups = e->n_eles > 0 ? plan_groups(e) : 0;
  if (n_groups > 0)
  {
    const size_t n_partial = (size_t)n_groups * H.n_res;
    // (growing frees the old buffer, which an earlier sample still queued may read: hipFree waits for the device first)
    if (H.partial.size() < n_partial && H.partial.alloc(n_partial)) return 1;
    ResidualArgs A{};
    A.div = e->arr[HFX_DIV_TCONF_UPTS];
    A.detjac = e->detjac_upts;
    A.src = e->src_nonzero ? e->arr[HFX_SRC_UPTS].get() : nullptr;
    A.partial = H.partial;
    A.P = (long)e->n_upts * e->n_eles;
    A.norm = ctx->hist_norm;
    if (e->n_dims == 3)
      hipLaunchKernelGGL(residual_norm_kernel<5>, dim3(n_groups), dim3(HR_THREADS), 0, st, A);
    else
      hipLaunchKernelGGL(residual_norm_kernel<4>, dim3(n_groups), dim3(HR_THREADS), 0, st, A);
    HFX_HIP(hipGetLastError());
  }
  int n_force_groups = 0;
  if (H.n_force > 0 && block_has_walls(e) && wall_force_partials_launch(e, &n_force_groups)) return 1;
  hipLaunchKernelGGL(history_finish_kernel, dim3(1), dim3(HF_THREADS), 0, st, H.partial.get(), n_groups, H.n_res, ctx->hist_norm,
                     n_force_groups > 0 ? e->wall_forces->partial.get() : nullptr, n_force_groups, H.n_force,
                     H.rows + (size_t)slot * (H.n_res + H.n_force));
  HFX_HIP(hipGetLastError());
  return 0;
}

bool history_monitor_reads_gradient(const hfx_eles *e)
{
  const hfx_ctx *ctx = e->ctx;
  return ctx->hist_on && ctx->hist_forces && ctx->params.viscous && block_has_walls(e);
}

unsigned history_sample_need(const hfx_eles *e)
{
  if (!e->ctx->hist_on) return 0;
  unsigned need = 1u << HFX_DIV_TCONF_UPTS;
  if (history_monitor_reads_gradient(e)) need |= (1u << HFX_DISU_UPTS0) | (1u << HFX_GRAD_DISU_UPTS);
  return need;
}

int sample_history(hfx_eles *e, double time, int step)
{
  hfx_ctx *ctx = e->ctx;
  if (!ctx->hist_on) return 0;
  if (prepare_history(e)) return 1;
  HistoryRows &H = e->history_rows;
  HFX_CHECK((int)H.times.size() < H.capacity, "hfx_eles_sample_history: the history is full (%d rows); read it (hfx_eles_read_history) "
                                              "before the next sample", H.capacity);
  if (check_sample(e, "hfx_eles_sample_history")) return 1;
  if (launch_sample(e, (int)H.times.size())) return 1;
  H.times.push_back(time);
  H.steps.push_back(step);
  return 0;
}

int history_check_capacity(hfx_eles *const *eles, int neb, int n_steps)
{
  hfx_ctx *ctx = eles[0]->ctx;
  if (!ctx->have_clock || !ctx->hist_on || n_steps <= 0) return 0;
  const long n_new = integral_samples_in(ctx->i_steps, n_steps, ctx->hist_freq);
  for (int i = 0; i < neb; i++)
  {
    HFX_CHECK(eles[i]->n_fields == eles[i]->n_dims + 2, "history monitor: a block of %d fields in %d dimensions", eles[i]->n_fields,
              eles[i]->n_dims);
    if (prepare_history(eles[i])) return 1;
    HistoryRows &H = eles[i]->history_rows;
    HFX_CHECK((long)H.times.size() + n_new <= H.capacity,
              "history monitor: %d steps from step %d take %ld rows (monitor_res_freq %d), the history of %d holds %d already; "
              "read it (hfx_eles_read_history) or take fewer steps per call",
              n_steps, ctx->i_steps, n_new, ctx->hist_freq, H.capacity, (int)H.times.size());
  }
  return 0;
}

} // namespace hfx

using namespace hfx;

extern "C" {

int hfx_ctx_set_history_monitor(hfx_ctx *ctx, int res_norm_type, int with_forces, int monitor_res_freq, int capacity)
{
  HFX_CHECK(ctx, "hfx_ctx_set_history_monitor: NULL ctx");
  if (capacity != 0)
  {
    HFX_CHECK(res_norm_type >= 0 && res_norm_type <= 2, "norm_type not recognized"); /* src/output.cpp:2241 */
    HFX_CHECK(capacity >= 1, "hfx_ctx_set_history_monitor: a history of %d rows (at least 1, or 0 for no monitor)", capacity);
    HFX_CHECK(monitor_res_freq >= 1, "hfx_ctx_set_history_monitor: monitor_res_freq %d (at least 1)", monitor_res_freq);
    HFX_CHECK(ctx->have_params, "hfx_ctx_set_history_monitor: parameters not set");
    HFX_CHECK(!with_forces || ctx->have_force_ref, "hfx_ctx_set_history_monitor: no force reference (hfx_ctx_set_force_reference)");
    // (the reference has one monitor_res_freq for the whole row)
    HFX_CHECK(ctx->n_iq == 0 || ctx->iq_freq == monitor_res_freq,
              "hfx_ctx_set_history_monitor: monitor_res_freq %d, and the integral monitor is registered with %d: a row of history.plt has one",
              monitor_res_freq, ctx->iq_freq);
  }
  HFX_IMMEDIATE(ctx, 0);
  ctx->hist_on = capacity != 0;
  if (ctx->hist_on)
  {
    ctx->hist_norm = res_norm_type;
    ctx->hist_forces = with_forces != 0;
    ctx->hist_freq = monitor_res_freq;
    ctx->hist_capacity = capacity;
  }
  ctx->hist_epoch++; // (every block makes its history anew, empty, when it is next asked for)
  return 0;
}

int hfx_eles_sample_history(hfx_eles *e, double time, int step)
{
  HFX_CHECK(e, "NULL eles");
  hfx_ctx *ctx = e->ctx;
  HFX_CHECK(ctx->hist_on, "hfx_eles_sample_history: no monitor (hfx_ctx_set_history_monitor)");
  // (a pending stage runs so that it stores div_tconf_upts and, for the viscous force, leaves the gradient: hfx_eles_compute_wall_forces)
  HFX_IMMEDIATE(ctx, history_sample_need(e));
  return sample_history(e, time, step);
}

int hfx_eles_history_count(hfx_eles *e, int *n_rows)
{
  HFX_CHECK(e && n_rows, "hfx_eles_history_count: NULL argument");
  *n_rows = e->history_rows.epoch == e->ctx->hist_epoch ? (int)e->history_rows.times.size() : 0;
  return 0;
}

int hfx_eles_read_history(hfx_eles *e, int max_rows, double *times, int *steps, double *residuals, double *forces, int *n_rows)
{
  HFX_CHECK(e && n_rows, "hfx_eles_read_history: NULL argument");
  HFX_IMMEDIATE(e->ctx, 0);
  if (prepare_history(e)) return 1;
  HistoryRows &H = e->history_rows;
  const int n = (int)H.times.size();
  HFX_CHECK(n <= max_rows, "hfx_eles_read_history: %d rows are stored, the caller's arrays hold %d", n, max_rows);
  HFX_CHECK(n == 0 || (times && steps && residuals && (forces || H.n_force == 0)), "hfx_eles_read_history: NULL argument");
  HFX_HIP(hipStreamSynchronize(e->ctx->stream));
  const int width = H.n_res + H.n_force;
  std::vector<double> rows((size_t)width * n);
  if (n > 0) HFX_HIP(hipMemcpy(rows.data(), H.rows, sizeof(double) * rows.size(), hipMemcpyDeviceToHost));
  for (int r = 0; r < n; r++)
  {
    const double *row = rows.data() + (size_t)width * r;
    std::copy(row, row + H.n_res, residuals + (size_t)H.n_res * r);
    if (H.n_force) std::copy(row + H.n_res, row + width, forces + (size_t)H.n_force * r);
  }
  std::copy(H.times.begin(), H.times.end(), times);
  std::copy(H.steps.begin(), H.steps.end(), steps);
  *n_rows = n;
  H.times.clear();
  H.steps.clear();
  return 0;
}

int hfx_eles_history_launch(hfx_eles *e, int *n_groups, int *points_per_pass)
{
  HFX_CHECK(e, "NULL eles");
  if (n_groups) *n_groups = e->n_eles > 0 ? plan_groups(e) : 0;
  if (points_per_pass) *points_per_pass = HR_THREADS * HR_POINTS;
  return 0;
}

int hfx_time_history(hfx_eles *e, int reps, double *ms)
{
  HFX_CHECK(e && ms && reps > 0, "hfx_time_history: bad argument");
  hfx_ctx *ctx = e->ctx;
  HFX_CHECK(ctx->hist_on, "hfx_time_history: no monitor (hfx_ctx_set_history_monitor)");
  unsigned need = 1u << HFX_DIV_TCONF_UPTS;
  if (history_monitor_reads_gradient(e)) need |= (1u << HFX_DISU_UPTS0) | (1u << HFX_GRAD_DISU_UPTS);
  HFX_IMMEDIATE(ctx, need);
  if (prepare_history(e)) return 1;
  if (check_sample(e, "hfx_time_history")) return 1;
  hipStream_t st = ctx->stream;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  float t = 0.f;
  // (no early return between the creation of the events and their destruction)
  hipError_t err = hipEventCreate(&t0);
  if (err == hipSuccess) err = hipEventCreate(&t1);
  int rc = err == hipSuccess ? launch_sample(e, e->history_rows.capacity) : 1; // (warm)
  if (err == hipSuccess) err = hipEventRecord(t0, st);
  for (int r = 0; r < reps && !rc && err == hipSuccess; r++) rc = launch_sample(e, e->history_rows.capacity);
  if (err == hipSuccess) err = hipEventRecord(t1, st);
  if (err == hipSuccess) err = hipEventSynchronize(t1);
  if (err == hipSuccess) err = hipEventElapsedTime(&t, t0, t1);
  if (t0) (void)hipEventDestroy(t0);
  if (t1) (void)hipEventDestroy(t1);
  HFX_CHECK(err == hipSuccess, "hfx_time_history: %s", hipGetErrorString(err));
  *ms = t / reps;
  return rc;
}

} // extern "C"
