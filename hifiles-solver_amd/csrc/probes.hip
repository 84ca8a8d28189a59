// probes.hip -- point probes sampled on the device: run_input.probe / probe_input (src/probe_input.cpp), the operator row
// eles::set_opp_probe (src/eles.cpp:3625-3631), eles::calc_disu_probepoints and the fields output::write_probe forms from the
// interpolated state (src/output.cpp:1479-1538), at the place and under the condition of the reference's main loop
// (src/HiFiLES.cpp:289-297).  gfx950 only.
//
// A sample is one launch per block: one wave per probe.  The 64 lanes stride over the solution points of the probe's element,
// so every field plane is read in coalesced 512-byte pieces and the operator row once for all planes; each lane adds its points
// in ascending order, the 64 partial sums are combined by a butterfly of cross-lane shuffles whose order is fixed, and lane 0
// forms the registered fields and stores them into the sample's slot of the device history.  No atomics, no order that depends
// on timing: a probe's value is a function of its operator row, its element's state and nothing else -- not of the probes
// registered beside it, nor of its place among them.
#include "step_loop.hpp"

namespace hfx
{

// by value in the kernel's argument segment
struct ProbeArgs
{
  const double *disu_upts; // (n_upts, n_eles, n_fields_state): disu_upts(0)
  const double *opp;       // (n_upts, n_probes), sorted order
  const int *ele, *dest;   // (n_probes) element | index in the caller's order, sorted order
  double *out;             // (n_out, n_probes): the slot of this sample, caller's order
  long P;                  // n_upts * n_eles, the length of one field plane
  int n_upts, n_probes, n_out;
  unsigned char code[HFX_MAX_PROBE_FIELDS];
  double gamma;
};

constexpr int PROBE_WAVES = 4; // waves (probes) per workgroup

// NF = n_dims + 2 state planes
template <int NF>
__global__ __launch_bounds__(64 * PROBE_WAVES) void sample_probes_kernel(const ProbeArgs A)
{
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * PROBE_WAVES + (threadIdx.x >> 6); // (uniform over the wave)
  if (p >= A.n_probes) return;
  const double *row = A.opp + (size_t)p * A.n_upts;
  const double *u = A.disu_upts + (size_t)A.ele[p] * A.n_upts;
  double acc[NF];
#pragma unroll
  for (int f = 0; f < NF; f++) acc[f] = 0.0;
  for (int k = lane; k < A.n_upts; k += 64)
  {
    const double c = row[k];
#pragma unroll
    for (int f = 0; f < NF; f++) acc[f] += c * u[k + f * A.P];
  }
  // lane l += lane l ^ 32, ^ 16, ... ^ 1: every lane ends with the same sum, formed in the same order
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
  {
#pragma unroll
    for (int f = 0; f < NF; f++) acc[f] += __shfl_xor(acc[f], off, 64);
  }
  if (lane != 0) return;
  // src/output.cpp:1479-1538 on the interpolated conservative state
  const double rho = acc[0], E = acc[NF - 1];
  double v_sq = 0.0;
#pragma unroll
  for (int m = 1; m < NF - 1; m++) v_sq += acc[m] * acc[m];
  v_sq /= rho * rho;
  const double pressure = (A.gamma - 1.0) * (E - 0.5 * rho * v_sq);
  double *dst = A.out + (size_t)A.dest[p] * A.n_out;
  for (int i = 0; i < A.n_out; i++)
  {
    const int c = A.code[i];
    // (selects between registers: no indexing by c)
    double v = rho;
    if (c == HFX_PROBE_U) v = acc[1] / rho;
    else if (c == HFX_PROBE_V) v = acc[2] / rho;
    else if (c == HFX_PROBE_W) v = acc[NF - 2] / rho; /* three-dimensional blocks only: field 3 = NF - 2 */
    else if (c == HFX_PROBE_E) v = E / rho;
    else if (c == HFX_PROBE_P) v = pressure;
    dst[i] = v;
  }
}

// the history of e as the context's probe registration wants it: made anew (and empty) when that registration has changed
static int prepare_history(hfx_eles *e)
{
  hfx_ctx *ctx = e->ctx;
  Probes &pr = e->probes;
  if (pr.epoch == ctx->probe_epoch) return 0;
  for (int i = 0; i < ctx->n_probe_fields; i++)
    HFX_CHECK(ctx->probe_codes[i] != HFX_PROBE_W || e->n_dims == 3, "probes: field w on a two-dimensional block");
  pr.history.reset();
  pr.times.clear();
  pr.steps.clear();
  pr.n_fields = ctx->n_probe_fields;
  pr.capacity = ctx->probe_capacity;
  if (pr.n > 0 && pr.n_fields > 0 && pr.history.alloc((size_t)pr.n_fields * pr.n * ((size_t)pr.capacity + 1))) return 1;
  pr.epoch = ctx->probe_epoch;
  return 0;
}

// one sampling launch of e's probes into slot `slot` of its history
static int launch_sample(hfx_eles *e, int slot)
{
  hfx_ctx *ctx = e->ctx;
  const Probes &pr = e->probes;
  HFX_CHECK(ctx->have_params, "parameters not set");
  HFX_CHECK(e->n_fields == e->n_dims + 2, "probes: a block of %d fields in %d dimensions", e->n_fields, e->n_dims);
  ProbeArgs A{};
  A.disu_upts = e->arr[HFX_DISU_UPTS0];
  A.opp = pr.opp;
  A.ele = pr.ele;
  A.dest = pr.dest;
  A.out = pr.history + (size_t)slot * pr.n_fields * pr.n;
  A.P = (long)e->n_upts * e->n_eles;
  A.n_upts = e->n_upts;
  A.n_probes = pr.n;
  A.n_out = pr.n_fields;
  for (int i = 0; i < pr.n_fields; i++) A.code[i] = (unsigned char)ctx->probe_codes[i];
  A.gamma = ctx->params.gamma;
  const dim3 grid((unsigned)((pr.n + PROBE_WAVES - 1) / PROBE_WAVES)), block(64 * PROBE_WAVES);
  if (e->n_dims == 3)
    hipLaunchKernelGGL(sample_probes_kernel<5>, grid, block, 0, ctx->stream, A);
  else
    hipLaunchKernelGGL(sample_probes_kernel<4>, grid, block, 0, ctx->stream, A);
  HFX_HIP(hipGetLastError());
  return 0;
}

int sample_probes(hfx_eles *e, double time, int step)
{
  hfx_ctx *ctx = e->ctx;
  Probes &pr = e->probes;
  if (pr.n == 0 || ctx->n_probe_fields == 0) return 0;
  if (prepare_history(e)) return 1;
  HFX_CHECK((int)pr.times.size() < pr.capacity, "hfx_eles_sample_probes: the history is full (%d samples of %d probes); read it "
                                                "(hfx_eles_read_probes) before the next sample", pr.capacity, pr.n);
  if (launch_sample(e, (int)pr.times.size())) return 1;
  pr.times.push_back(time);
  pr.steps.push_back(step);
  return 0;
}

int probes_check_capacity(hfx_eles *const *eles, int neb, int n_steps)
{
  hfx_ctx *ctx = eles[0]->ctx;
  if (!ctx->have_clock || ctx->n_probe_fields == 0 || n_steps <= 0) return 0;
  // the steps i_steps + 1 .. i_steps + n_steps that are multiples of probe_freq
  const long f = ctx->probe_freq, i0 = ctx->i_steps;
  const long n_new = (i0 + n_steps) / f - i0 / f;
  for (int i = 0; i < neb; i++)
  {
    Probes &pr = eles[i]->probes;
    if (pr.n == 0) continue;
    if (prepare_history(eles[i])) return 1;
    HFX_CHECK((long)pr.times.size() + n_new <= pr.capacity,
              "probes: %d steps from step %d take %ld samples (probe_freq %d), the history of %d holds %d already; read it "
              "(hfx_eles_read_probes) or take fewer steps per call",
              n_steps, ctx->i_steps, n_new, ctx->probe_freq, pr.capacity, (int)pr.times.size());
  }
  return 0;
}

} // namespace hfx

using namespace hfx;

extern "C" {

int hfx_ctx_set_probes(hfx_ctx *ctx, int n_fields, const int *codes, int probe_freq, int capacity)
{
  HFX_CHECK(ctx && (n_fields == 0 || codes), "hfx_ctx_set_probes: NULL argument");
  HFX_CHECK(n_fields >= 0 && n_fields <= HFX_MAX_PROBE_FIELDS, "hfx_ctx_set_probes: %d fields (at most %d)", n_fields, HFX_MAX_PROBE_FIELDS);
  for (int i = 0; i < n_fields; i++)
    HFX_CHECK(codes[i] >= HFX_PROBE_RHO && codes[i] <= HFX_PROBE_P, "hfx_ctx_set_probes: unknown probe field %d", codes[i]);
  if (n_fields > 0)
  {
    HFX_CHECK(probe_freq >= 1, "hfx_ctx_set_probes: probe_freq %d (at least 1)", probe_freq);
    HFX_CHECK(capacity >= 1, "hfx_ctx_set_probes: a history of %d samples (at least 1)", capacity);
  }
  HFX_IMMEDIATE(ctx, 0);
  ctx->n_probe_fields = n_fields;
  if (n_fields > 0)
  {
    std::copy(codes, codes + n_fields, ctx->probe_codes);
    ctx->probe_freq = probe_freq;
    ctx->probe_capacity = capacity;
  }
  ctx->probe_epoch++; // (every block makes its history anew, empty, when it is next asked for)
  return 0;
}

int hfx_eles_set_probes(hfx_eles *e, int n_probes, const int *ele, const double *opp_probe)
{
  HFX_CHECK(e && (n_probes == 0 || (ele && opp_probe)), "hfx_eles_set_probes: NULL argument");
  HFX_CHECK(n_probes >= 0, "hfx_eles_set_probes: %d probes", n_probes);
  for (int i = 0; i < n_probes; i++)
    HFX_CHECK(ele[i] >= 0 && ele[i] < e->n_eles, "hfx_eles_set_probes: probe %d lies in element %d of %d", i, ele[i], e->n_eles);
  hfx_ctx *ctx = e->ctx;
  for (int i = 0; i < (n_probes > 0 ? ctx->n_probe_fields : 0); i++)
    HFX_CHECK(ctx->probe_codes[i] != HFX_PROBE_W || e->n_dims == 3, "hfx_eles_set_probes: field w on a two-dimensional block");
  HFX_IMMEDIATE(ctx, 0);
  HFX_HIP(hipStreamSynchronize(ctx->stream)); // (a sample of the probes that go may still be running)
  // sorted by element, stable: probes of one element read the same cache lines, and a probe's value does not depend on its place
  std::vector<int> order(n_probes);
  for (int i = 0; i < n_probes; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ele[a] < ele[b]; });
  std::vector<int> h_ele(n_probes);
  std::vector<double> h_opp((size_t)n_probes * e->n_upts);
  for (int i = 0; i < n_probes; i++)
  {
    h_ele[i] = ele[order[i]];
    std::copy(opp_probe + (size_t)order[i] * e->n_upts, opp_probe + (size_t)(order[i] + 1) * e->n_upts, h_opp.begin() + (size_t)i * e->n_upts);
  }
  // built beside the registered probes, which stay until everything is there
  Probes nw;
  if (n_probes > 0)
  {
    if (nw.opp.upload(h_opp) || nw.ele.upload(h_ele) || nw.dest.upload(order)) return 1;
    nw.n = n_probes;
    if (ctx->n_probe_fields > 0 &&
        nw.history.alloc((size_t)ctx->n_probe_fields * n_probes * ((size_t)ctx->probe_capacity + 1)))
      return 1;
    nw.n_fields = ctx->n_probe_fields;
    nw.capacity = ctx->probe_capacity;
  }
  nw.epoch = ctx->probe_epoch;
  e->probes = std::move(nw);
  return 0;
}

int hfx_eles_sample_probes(hfx_eles *e, double time, int step)
{
  HFX_CHECK(e, "NULL eles");
  // (the stage that has been recorded leaves disu_upts(0) of the new state whichever way it runs)
  HFX_IMMEDIATE(e->ctx, 0);
  HFX_CHECK(e->ctx->n_probe_fields > 0, "hfx_eles_sample_probes: no probe fields (hfx_ctx_set_probes)");
  return sample_probes(e, time, step);
}

int hfx_eles_probe_count(hfx_eles *e, int *n_samples, int *n_probes)
{
  HFX_CHECK(e, "NULL eles");
  const bool current = e->probes.epoch == e->ctx->probe_epoch;
  if (n_samples) *n_samples = current ? (int)e->probes.times.size() : 0;
  if (n_probes) *n_probes = e->probes.n;
  return 0;
}

int hfx_eles_read_probes(hfx_eles *e, int max_samples, double *times, int *steps, double *values, int *n_samples)
{
  HFX_CHECK(e && n_samples, "hfx_eles_read_probes: NULL argument");
  HFX_IMMEDIATE(e->ctx, 0);
  if (prepare_history(e)) return 1;
  Probes &pr = e->probes;
  const int n = (int)pr.times.size();
  HFX_CHECK(n <= max_samples, "hfx_eles_read_probes: %d samples are stored, the caller's arrays hold %d", n, max_samples);
  HFX_CHECK(n == 0 || (times && steps && values), "hfx_eles_read_probes: NULL argument");
  HFX_HIP(hipStreamSynchronize(e->ctx->stream));
  if (n > 0 && pr.n > 0)
    HFX_HIP(hipMemcpy(values, pr.history, sizeof(double) * (size_t)pr.n_fields * pr.n * n, hipMemcpyDeviceToHost));
  std::copy(pr.times.begin(), pr.times.end(), times);
  std::copy(pr.steps.begin(), pr.steps.end(), steps);
  *n_samples = n;
  pr.times.clear();
  pr.steps.clear();
  return 0;
}

int hfx_time_probes(hfx_eles *e, int reps, double *ms)
{
  HFX_CHECK(e && ms && reps > 0, "hfx_time_probes: bad argument");
  HFX_IMMEDIATE(e->ctx, 0);
  HFX_CHECK(e->probes.n > 0 && e->ctx->n_probe_fields > 0, "hfx_time_probes: no probes (hfx_ctx_set_probes, hfx_eles_set_probes)");
  if (prepare_history(e)) return 1;
  hipStream_t st = e->ctx->stream;
  hipEvent_t t0, t1;
  HFX_HIP(hipEventCreate(&t0));
  HFX_HIP(hipEventCreate(&t1));
  int rc = launch_sample(e, e->probes.capacity); // (warm)
  HFX_HIP(hipEventRecord(t0, st));
  for (int r = 0; r < reps && !rc; r++) rc = launch_sample(e, e->probes.capacity);
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
