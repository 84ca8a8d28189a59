// step_loop.hpp -- the time-step loop of every hfx_run_steps* entry point and the per-step duties it runs (step_loop.hip):
//   calc_time_step -> begin_of_step -> per RK stage: [closure filter at stage 0] stage -> advance_ramp_counters -> end_of_step
// A new per-step duty is one line in end_of_step (or begin_of_step) and, where it can refuse, one in step_loop_check.
#pragma once
#include "hfx_internal.hpp"
#include <functional>

namespace hfx
{
// RK stages per time step of adv_type (src/HiFiLES.cpp:143-150)
inline int n_rk_stages(int adv_type) { return (adv_type == 0) ? 1 : (adv_type <= 2) ? 4 : (adv_type == 3) ? 5 : 14; }
inline int n_rk_stages(const hfx_params &p) { return n_rk_stages(p.adv_type); }

// ---- the duties, each in its own file ----
// (averages.hip) one update of e's averages on the compute stream; nothing for a block without average fields
int launch_time_average(hfx_eles *e, double time, double spinup_time);
// (forcing.hip) eles::evaluate_body_force for one block that has a body force registered.  comm: a partitioned loop's communicator -- the
// integrals are summed over its ranks (src/eles.cpp:5375-5385) by the path of hfx_comm_allreduce, one host round trip; without one
// nothing leaves the device
int evaluate_body_force(hfx_eles *e, hfx_comm *comm);
// (probes.hip) one sample of e's probes on the compute stream; nothing for a block or a context without probes
int sample_probes(hfx_eles *e, double time, int step);
// what every step loop asks before its first launch: can the histories of these blocks take the samples of the next n_steps steps?
// Nothing to ask without the library's clock or without probes
int probes_check_capacity(hfx_eles *const *eles, int neb, int n_steps);
// ---- the integral monitor (integrals.hip) ----
// does the reference fill the Diagnostics columns after step `step`?  i_steps == 1 || i_steps % monitor_res_freq == 0
// (src/HiFiLES.cpp:247-266)
inline bool integral_sample_step(long step, long freq) { return step == 1 || step % freq == 0; }
// how many of the steps i_steps + 1 .. i_steps + n_steps are such steps
inline long integral_samples_in(long i_steps, long n_steps, long freq)
{
  if (n_steps <= 0) return 0;
  const long last = i_steps + n_steps;
  return last / freq - i_steps / freq + ((freq > 1 && i_steps < 1 && last >= 1) ? 1 : 0);
}
// will the step loops sample behind the step that makes i_steps `step`?
inline bool integral_monitor_samples(const hfx_ctx *ctx, long step)
{
  return ctx->have_clock && ctx->n_iq > 0 && integral_sample_step(step, ctx->iq_freq);
}
// does a sample read grad_disu_upts (an id 1-4)?  The last RK stage of a step that is sampled then has to leave the corrected gradient
// of its input state in memory
bool integral_monitor_reads_gradient(const hfx_ctx *ctx);
// one sample of e on the compute stream; nothing for a context without a monitor or a block without a cubature
int sample_integrals(hfx_eles *e, double time, int step);
// what every step loop asks before its first launch, beside probes_check_capacity
int integrals_check_capacity(hfx_eles *const *eles, int neb, int n_steps);
// ---- the history monitor (history.hip) ----
// will the step loops take a row behind the step that makes i_steps `step`?  The condition of the integral monitor, the reference's one
inline bool history_monitor_samples(const hfx_ctx *ctx, long step)
{
  return ctx->have_clock && ctx->hist_on && integral_sample_step(step, ctx->hist_freq);
}
// does a row of e read grad_disu_upts: the monitor with forces, a viscous context, a block with wall faces
bool history_monitor_reads_gradient(const hfx_eles *e);
// one row of e on the compute stream; nothing for a context without the monitor
int sample_history(hfx_eles *e, double time, int step);
// what every step loop asks before its first launch, beside probes_check_capacity and integrals_check_capacity
int history_check_capacity(hfx_eles *const *eles, int neb, int n_steps);
// ---- the plot monitor (plot_fields.hip) ----
// does a snapshot of e read grad_disu_upts: a monitor with vorticity or a Q criterion, a block with plot points
bool plot_monitor_reads_gradient(const hfx_eles *e);
// will the step loops take a snapshot behind the step that makes i_steps `step`?  i_steps % plot_freq == 0 (src/HiFiLES.cpp:273)
inline bool plot_monitor_samples(const hfx_ctx *ctx, long step) { return ctx->have_clock && ctx->plot_on && step % ctx->plot_freq == 0; }
// how many of the steps i_steps + 1 .. i_steps + n_steps are such steps
inline long plot_samples_in(long i_steps, long n_steps, long freq) { return n_steps <= 0 ? 0 : (i_steps + n_steps) / freq - i_steps / freq; }
// one snapshot of e on the compute stream; nothing for a context without the monitor or a block without plot points
int sample_plot(hfx_eles *e, double time, int step);
// what every step loop asks before its first launch, beside the other three: the capacity, and everything that refuses a block
int plot_check_capacity(hfx_eles *const *eles, int neb, int n_steps);
// what one sample of each monitor asks a pending deferred stage to leave in memory (bit i = hfx_array_id i): the need mask of
// hfx_eles_sample_integral_quantities, hfx_eles_sample_history and hfx_eles_sample_plot; 0 where the context has no such monitor
// or the block is not equipped for it
unsigned integral_sample_need(const hfx_eles *e);
unsigned history_sample_need(const hfx_eles *e);
unsigned plot_sample_need(const hfx_eles *e);

// ---- the one-stage rule of the step loops ----
// does a monitor the loops sample read grad_disu_upts of one of these blocks: the integral monitor with an id 1-4 and a block with a
// cubature, the history monitor's viscous wall forces (history_monitor_reads_gradient), or the plot monitor's vorticity and Q criteria
// on a block with plot points (plot_monitor_reads_gradient)?  The last RK stage of a step that is sampled then has to leave the
// corrected gradient of its input state in memory
bool monitor_reads_gradient(hfx_eles *const *eles, int neb);
// will the loops sample such a monitor behind the step that makes i_steps `step`?  (The plot monitor has a frequency of its own: it
// counts only where it reads the gradient, so that a plot of gradient-free fields never changes what another monitor's steps launch)
inline bool monitor_samples(const hfx_ctx *ctx, long step)
{
  bool plot_gradient = false;
  for (int m = 0; m < ctx->n_plot_diag; m++) plot_gradient = plot_gradient || pf_reads_gradient(ctx->plot_codes[m]);
  return integral_monitor_samples(ctx, step) || history_monitor_samples(ctx, step) || (plot_gradient && plot_monitor_samples(ctx, step));
}
// One RK stage call by call -- CalcResidual, AdvanceSolution, the shock filter where registered -- and the flux-point solution of the new
// state, which the fused stage that follows reads: what a loop whose stages keep the gradient on chip runs as the last stage of a step
// the monitor samples with a gradient quantity
int stage_call_by_call(hfx_eles *const *eles, int neb, hfx_inters *const *faces, int nfb, int rk);
// A monitor inside a loop that cannot fall back to stage_call_by_call (the partitioned ones: messages are in flight).  Asked before the
// first launch.  nullptr: the loop does not sample (the clock is not the library's) or no monitor reads the gradient; else the refusal of
// a loop whose stages keep it on chip
const char *monitor_gradient_on_chip(hfx_eles *const *eles, int neb);

// ---- the pieces of a step ----
// what every step loop asks before its first launch, and before it changes anything: the four capacity checks above, then -- do the
// wall-model faces of a viscous run have their input points (wall_model_check_points)?
int step_loop_check(hfx_eles *const *eles, int neb, hfx_inters *const *faces, int nfb, int n_steps);
// calc_time_step (src/solver.cpp:484-549, src/HiFiLES.cpp:198): dt_type 1 sets params.dt to the minimum CFL step over the blocks
// (src/solver.cpp:498-505) and, with `comm`, over its ranks -- one all-reduce; dt_type 2 refreshes HFX_DT_LOCAL; dt_type 0: nothing.
// It reads disu_upts(0) on the compute stream; a solution message in flight reads the packed flux-point values
int calc_time_step_blocks(hfx_eles *const *eles, int neb, hfx_comm *comm);
// the `forcing == 1` branch at the first RK stage of a step (src/solver.cpp:96-109): evaluate_body_force of every block that has a body
// force registered -- three launches per such block and, without `comm`, nothing else: no copy, no synchronisation.  With `comm` (the
// partitioned loops) the two integrals are summed over its ranks between the first and the second kernel: one host round trip per step.
// Called behind calc_time_step_blocks: the controller takes params.dt of this step.  Nothing, and no launch, for blocks without a body force
int begin_of_step(hfx_eles *const *eles, int neb, hfx_comm *comm);
// first stage of a step (src/solver.cpp:55-62): calc_sgs_terms of every block with a filtering closure.  SVV replaces the state;
// refresh_svv: extrapolate it again at once (the unpartitioned fused loops; deferred does so through fpts_valid, partitioned blocks refuse SVV: false)
int first_stage_closure_filter(hfx_eles *const *eles, int neb, bool refresh_svv);
// run_input.ramp_counter++ after a time step for the boundary blocks with a ramping group (src/HiFiLES.cpp:224-225)
void advance_ramp_counters(hfx_inters *const *faces, int nfb);
// What the reference's main loop does between the last RK stage and the next step (src/HiFiLES.cpp:221-297), for a context whose clock
// is the library's, in this order:
//   1. the clock: time += dt, i_steps++, spinup_time at step 1
//   2. the time averages of every block that has average fields (averages.hip)
//   3. when i_steps % probe_freq == 0: one sample of every block that has probes (probes.hip)
//   4. when i_steps == 1 || i_steps % monitor_res_freq == 0: one sample of the integral monitor for every block with a cubature (integrals.hip)
//   5. under the same condition with its own frequency: one row of the history monitor for every block (history.hip)
//   6. when i_steps % plot_freq == 0: one snapshot of the plot monitor for every block with plot points (plot_fields.hip)
// Nothing for a context without a clock; no launch for a block that a duty has nothing to do for
int end_of_step(hfx_eles *const *eles, int neb);

// ---- the loop ----
enum class ClosureFilter { none, filtering, filtering_refresh_svv }; // first_stage_closure_filter at stage 0: not at all / (.., false) / (.., true)
struct StepLoop
{
  hfx_eles *const *eles;
  int neb;
  hfx_inters *const *faces; // the face blocks whose ramp counters advance (a partitioned loop: its interior and boundary blocks)
  int nfb;
  std::function<int(int rk)> stage; // one RK stage as this loop runs it
  ClosureFilter closure = ClosureFilter::none;
  hfx_comm *comm = nullptr; // a partitioned loop: the MIN of calc_time_step and the body force's sums go over its ranks
  // the stages keep the gradient on chip and a monitor reads it: the last stage of a step it samples is stage_call_by_call on `faces`
  bool by_calls = false;
};
// n_steps time steps.  last_by_calls (optional): did the last step run its last stage call by call (note_gradients of the callers)?
int run_step_loop(const StepLoop &L, int n_steps, bool *last_by_calls = nullptr);
} // namespace hfx
