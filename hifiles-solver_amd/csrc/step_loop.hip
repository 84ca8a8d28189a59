// step_loop.hip -- the one time-step loop behind every hfx_run_steps* entry point (the reference's main loop, src/HiFiLES.cpp:194-297,
// around the RK stages of src/solver.cpp:45-216) and the pieces it is made of.  The duties themselves -- time averages, probes, the
// integral, history and plot monitors, the body force -- live in their own files; here is the one place that calls them.  gfx950 only.
#include "step_loop.hpp"

namespace hfx
{

int step_loop_check(hfx_eles *const *eles, int neb, hfx_inters *const *faces, int nfb, int n_steps)
{
  if (probes_check_capacity(eles, neb, n_steps)) return 1;
  if (integrals_check_capacity(eles, neb, n_steps)) return 1;
  if (history_check_capacity(eles, neb, n_steps)) return 1;
  if (plot_check_capacity(eles, neb, n_steps)) return 1;
  return wall_model_check_points(faces, nfb);
}

int calc_time_step_blocks(hfx_eles *const *eles, int neb, hfx_comm *comm)
{
  hfx_ctx *ctx = eles[0]->ctx;
  if (ctx->params.dt_type != 1 && ctx->params.dt_type != 2) return 0;
  HFX_CHECK(ctx->have_CFL, "dt_type %d needs run_input.CFL: call hfx_ctx_set_CFL", ctx->params.dt_type);
  double dt_min = 1e12;
  for (int i = 0; i < neb; i++)
  {
    double dt_block = 0.0;
    if (hfx_eles_calc_dt_local(eles[i], ctx->CFL, &dt_block)) return 1;
    dt_min = std::min(dt_min, dt_block);
  }
  if (comm && comm->nranks > 1 && hfx_comm_allreduce(comm, &dt_min, 1, 0)) return 1;
  ctx->params.dt = dt_min;
  return 0;
}

int begin_of_step(hfx_eles *const *eles, int neb, hfx_comm *comm)
{
  for (int i = 0; i < neb; i++)
    if (eles[i]->body_force && evaluate_body_force(eles[i], comm)) return 1;
  return 0;
}

int first_stage_closure_filter(hfx_eles *const *eles, int neb, bool refresh_svv)
{
  for (int i = 0; i < neb; i++)
    if (eles[i]->les_ready && eles[i]->les.sgs_model >= 2 &&
        (hfx_eles_calc_sgs_terms(eles[i]) || (refresh_svv && eles[i]->les.sgs_model == 3 && hfx_eles_extrapolate_solution(eles[i]))))
      return 1;
  return 0;
}

void advance_ramp_counters(hfx_inters *const *faces, int nfb)
{
  for (int b = 0; b < nfb; b++)
    if (faces[b]->is_bdy && faces[b]->any_ramp) faces[b]->ramp_counter++;
}

int end_of_step(hfx_eles *const *eles, int neb)
{
  hfx_ctx *ctx = eles[0]->ctx;
  if (!ctx->have_clock) return 0;
  ctx->time += ctx->params.dt; /* src/HiFiLES.cpp:221-223 */
  ctx->i_steps++;
  if (ctx->i_steps == 1) ctx->spinup_time = ctx->time; /* src/HiFiLES.cpp:242-243 */
  for (int i = 0; i < neb; i++)
    if (launch_time_average(eles[i], ctx->time, ctx->spinup_time)) return 1;
  if (ctx->n_probe_fields > 0 && ctx->i_steps % ctx->probe_freq == 0) /* src/HiFiLES.cpp:289-297 */
    for (int i = 0; i < neb; i++)
      if (sample_probes(eles[i], ctx->time, ctx->i_steps)) return 1;
  if (integral_monitor_samples(ctx, ctx->i_steps)) /* src/HiFiLES.cpp:247-266 */
    for (int i = 0; i < neb; i++)
      if (sample_integrals(eles[i], ctx->time, ctx->i_steps)) return 1;
  if (history_monitor_samples(ctx, ctx->i_steps))
    for (int i = 0; i < neb; i++)
      if (sample_history(eles[i], ctx->time, ctx->i_steps)) return 1;
  if (plot_monitor_samples(ctx, ctx->i_steps)) /* src/HiFiLES.cpp:273-285 */
    for (int i = 0; i < neb; i++)
      if (sample_plot(eles[i], ctx->time, ctx->i_steps)) return 1;
  return 0;
}

bool monitor_reads_gradient(hfx_eles *const *eles, int neb)
{
  const hfx_ctx *ctx = eles[0]->ctx;
  if (!ctx->params.viscous) return false;
  const bool integrals = integral_monitor_reads_gradient(ctx);
  for (int i = 0; i < neb; i++)
    if ((integrals && eles[i]->n_vol_cubpts > 0) || history_monitor_reads_gradient(eles[i]) || plot_monitor_reads_gradient(eles[i])) return true;
  return false;
}

int stage_call_by_call(hfx_eles *const *eles, int neb, hfx_inters *const *faces, int nfb, int rk)
{
  const int adv = eles[0]->ctx->params.adv_type;
  if (hfx_CalcResidual_blocks(eles, neb, faces, nfb)) return 1;
  for (int i = 0; i < neb; i++)
    if (hfx_eles_AdvanceSolution(eles[i], rk, adv)) return 1;
  for (int i = 0; i < neb; i++)
    if (eles[i]->shock_ready && hfx_eles_shock_capture(eles[i])) return 1; /* src/HiFiLES.cpp:214-216 */
  // (the update call by call has cleared fpts_valid, DESIGN.md 3.7: the fused stage behind this one reads disu_fpts of the new state)
  for (int i = 0; i < neb; i++)
    if (hfx_eles_extrapolate_solution(eles[i])) return 1;
  return 0;
}

// The integral monitor inside a partitioned loop: a quantity that reads grad_disu_upts would need the last stage of a sampled step run
// call by call with messages in flight, which is not built
static const char *const MONITOR_PARTITIONED =
    "partitioned step loop: the integral monitor has a quantity that reads grad_disu_upts (ids 1-4), and the stages of this loop keep the "
    "gradient on chip; run it with fused mode 2 (hfx_ctx_set_fused_mode), or monitor the kinetic energy (id 0) alone";
// the same for the history monitor's viscous wall forces (history.hip)
static const char *const HISTORY_PARTITIONED =
    "partitioned step loop: the history monitor samples the viscous wall forces, which read grad_disu_upts, and the stages of this loop "
    "keep the gradient on chip; run it with fused mode 2 (hfx_ctx_set_fused_mode), or monitor the residuals alone (with_forces 0)";
// the same for the plot monitor's vorticity and Q criteria (plot_fields.hip)
static const char *const PLOT_PARTITIONED =
    "partitioned step loop: the plot monitor has a field that reads grad_disu_upts (vorticity, q_criterion, scaled_q_criterion), and the "
    "stages of this loop keep the gradient on chip; run it with fused mode 2 (hfx_ctx_set_fused_mode), or plot gradient-free fields alone";

const char *monitor_gradient_on_chip(hfx_eles *const *eles, int neb)
{
  const hfx_ctx *ctx = eles[0]->ctx;
  if (!ctx->have_clock || !monitor_reads_gradient(eles, neb)) return nullptr;
  for (int i = 0; i < neb; i++)
    if (history_monitor_reads_gradient(eles[i])) return HISTORY_PARTITIONED;
  for (int i = 0; i < neb; i++)
    if (plot_monitor_reads_gradient(eles[i])) return PLOT_PARTITIONED;
  return MONITOR_PARTITIONED;
}

int run_step_loop(const StepLoop &L, int n_steps, bool *last_by_calls)
{
  hfx_ctx *ctx = L.eles[0]->ctx;
  const int nst = n_rk_stages(ctx->params); /* src/HiFiLES.cpp:143-150 */
  bool by_calls = false;
  for (int s = 0; s < n_steps; s++)
  {
    if (calc_time_step_blocks(L.eles, L.neb, L.comm)) return 1; /* src/HiFiLES.cpp:198 */
    if (begin_of_step(L.eles, L.neb, L.comm)) return 1;         /* src/solver.cpp:96-109 */
    // a monitor that reads grad_disu_upts pairs the state behind a step with the gradient of the last stage's input state
    by_calls = L.by_calls && monitor_samples(ctx, (long)ctx->i_steps + 1);
    for (int rk = 0; rk < nst; rk++)
    {
      // (the SVV closure replaces the state, whose flux-point values the previous stage's update kernel has already written)
      if (rk == 0 && L.closure != ClosureFilter::none && /* src/solver.cpp:55-62 */
          first_stage_closure_filter(L.eles, L.neb, L.closure == ClosureFilter::filtering_refresh_svv))
        return 1;
      if (by_calls && rk == nst - 1 ? stage_call_by_call(L.eles, L.neb, L.faces, L.nfb, rk) : L.stage(rk)) return 1;
    }
    advance_ramp_counters(L.faces, L.nfb); /* src/HiFiLES.cpp:224-225 */
    if (end_of_step(L.eles, L.neb)) return 1;      /* src/HiFiLES.cpp:221-297 */
  }
  if (last_by_calls) *last_by_calls = by_calls;
  return 0;
}

} // namespace hfx
