// fused_hex.hpp -- the split fused stage for tensor-product elements (declarations).
#pragma once
#include "hfx_internal.hpp"

namespace hfx
{
// drop any fused-path tables derived from the block's face registration
void fused_invalidate(hfx_eles *e);
// the split fused stage (variants 2 and 3): pairwise face kernels + per-element kernels, three or four launches per stage;
// n_steps time steps, fails loudly when the block does not qualify
int split_run_steps(hfx_eles *e, hfx_inters *const *faces, int nfb, int n_steps, int variant = 2);
// average duration (ms, HIP events on the context stream) of each kernel of the stage over `reps` stages
int split_time_kernels(hfx_eles *e, hfx_inters *const *faces, int nfb, int reps, double *ms, char *names, int names_len,
                       int variant = 2);
// the local face that holds the left-over flux points of the two-wave flux kernel on this block (-1: the form does not run), and
// per local face the elements that would need the projected viscous flux of a left-over point there
int split_two_wave_face(hfx_eles *e, hfx_inters *const *faces, int nfb, int variant, int *face, long need[6]);
// algorithmic HBM bytes per launch of each kernel, same order
void split_kernel_bytes(const hfx_eles *e, double *bytes, int variant = 2);
// what the split stage runs on a block when `requested_variant` (2 or 3) is asked for (split_common.hpp): its .variant is 2
// (the reference's gradient arrays kept) when asked for, when the block has an LES closure that variant 3 cannot evaluate,
// or when variant 3 does not fit its element size (hexes from P6 on), else 3.  Needs the block's fused tables (fused_build)
struct SplitPlan;
SplitPlan split_plan(const hfx_eles *e, hfx_inters *const *faces, int nfb, int requested_variant);
// the plan of a stage that is about to run: split_plan, and the one refusal of what no variant of the split stage computes
// (over-integration where variant 2 runs).  Non-zero: refused, message in hfx_last_error
int split_stage_plan(const hfx_eles *e, hfx_inters *const *faces, int nfb, int requested_variant, SplitPlan *pl);
// builds the block's fused tables for these face blocks unless they exist; non-zero (message in hfx_last_error) when the
// block does not qualify for the split fused stage.  partitioned: flux points without a registered face are partition-face points
int ensure_fused_tables(hfx_eles *e, hfx_inters *const *faces, int nfb, bool partitioned);
// the one-sided partition-face kernels (kernels_mpi.hpp)
enum class MpiKernel
{
  pack_solution,         // the flux-point solution into the send buffer
  ldg_delta,             // LDG corrections from both sides' solution
  pack_gradient,         // the corrected gradient into the send buffer
  common_invflux,        // inviscid common flux
  common_viscflux,       // viscous common flux from both sides' gradients
  pack_projected_flux,   // each side's viscous flux projected on its own normal (Fn) into the send buffer
  common_flux_projected, // common flux from both sides' solution and Fn
  pack_sgs_flux,         // the physical SGS flux into the send buffer
};
// one of them on a block of the GENERAL fused stage, whose projected viscous flux is `fn` (st NULL: the compute stream)
int mpi_launch_general(hfx_eles *e, hfx_inters *f, MpiKernel k, const double *fn, hipStream_t st = nullptr);
// ---- the deferred scheduler's pieces (deferred.hip) ----
// ONE stage of the split fused path (the variant that split_plan names for the context's fused mode) on a block whose
// disu_fpts belongs to the current state; write_div: store div_tconf_upts; shock: shock_capture follows AdvanceSolution
// (src/HiFiLES.cpp:214-216)
int split_deferred_stage(hfx_eles *e, hfx_inters *const *faces, int nfb, int in_step, bool write_div, bool shock);
// the same on a partitioned block with the library's transport (comm.hip); start: this state's flux-point solution has not
// been sent yet
int partitioned_stage_deferred(hfx_eles *e, hfx_inters *const *int_faces, int n_int, hfx_inters *const *mpi_faces, int n_mpi,
                               hfx_comm *comm, int rk, bool start);
} // namespace hfx
