// general.hpp -- the fused RK stage for general (non-tensor-product) element classes: a block's plan, the stage's steps (general.hip).
#pragma once
#include <vector>
#include "hfx_internal.hpp"

namespace hfx
{
constexpr int GB = 16; // elements per batch = MFMA tile edge
// the element classes of the reference's orders 1..3 (tetrahedra, then prisms: solution / flux points) have kernel instantiations with
// compile-time sizes, anything else runs the size-generic form.  THE list: dispatch, plan and the LES qualification read it
constexpr int GENERAL_SIZES[][2] = {{4, 12}, {10, 24}, {20, 40}, {6, 18}, {18, 39}, {40, 68}};
constexpr int N_GENERAL_SIZES = sizeof(GENERAL_SIZES) / sizeof(GENERAL_SIZES[0]);
constexpr int pad4(int n) { return (n + 3) & ~3; }
// LDS image of a batch: flux kernel U | D | G planes, update kernel X | S planes
constexpr size_t general_flux_lds_bytes(int nu, int nfp) { return sizeof(double) * GB * (20 * pad4(nu) + 5 * pad4(nfp)); }
constexpr size_t general_update_lds_bytes(int nu, int nfp) { return sizeof(double) * GB * (5 * pad4(nfp) + 5 * pad4(nu)); }
// two workgroups per CU where the batch's LDS image allows it (4 waves each), otherwise one of 8 waves
constexpr int general_flux_default_waves(int nu, int nfp) { return general_flux_lds_bytes(nu, nfp) <= 80 * 1024 ? 4 : 8; }
// doubles per field that a thread stages when n rows x 16 elements are dealt to `waves` waves
constexpr int general_staged(int n, int waves) { return (n * GB + 64 * waves - 1) / (64 * waves); }
// do ALL staging loads of a thread fit its registers at once?  The kernels' `if constexpr` and the plan both ask here.  (Update kernel:
// P3 prisms stage 5 + 3 doubles per field on four waves -- past the limit, every trip then waited for its own loads: 0.233 ms for 451 MB)
constexpr bool general_flux_batched(int nu, int nfp, int waves) { return (general_staged(pad4(nu), waves) + general_staged(pad4(nfp), waves)) * 5 <= 30; }
constexpr bool general_update_batched(int nu, int nfp, int waves) { return general_staged(pad4(nfp), waves) * 5 <= 20 && general_staged(nu, waves) * 5 <= 15; }
constexpr bool general_sizes_as_measured()
{
  bool ok = general_flux_lds_bytes(40, 68) == 145920;
  for (const auto &sz : GENERAL_SIZES) // P3 prisms (big): 8 flux waves, P0 batched at 8 only, update on 8; the others 4 / at 3, 4 and 8 / 4
    ok = ok && general_flux_default_waves(sz[0], sz[1]) == (sz[0] == 40 ? 8 : 4) && general_flux_batched(sz[0], sz[1], 3) == (sz[0] != 40) &&
         general_flux_batched(sz[0], sz[1], 4) == (sz[0] != 40) && general_flux_batched(sz[0], sz[1], 8) && general_update_batched(sz[0], sz[1], 4) == (sz[0] != 40);
  return ok;
}
static_assert(general_sizes_as_measured(), "the launch forms of the six instantiated element sizes have changed");

// What the general stage runs on one block (general_plan, general.hip): every launch form decided once, from the options, the
// block's sizes and flags and its partner words.  Kernel arguments, launches, byte counts and the face loop read it.
struct GeneralPlan
{
  int size_class = -1;       // index in GENERAL_SIZES; -1: the size-generic kernels
  int flux_waves = 4;        // flux kernel: option general_waves (3, 4, 8), else general_flux_default_waves
  bool flux_batched = false; // its P0 requests all loads up front (an instantiated size that passes general_flux_batched)
  bool gather = false;       // and forms the block's LDG corrections itself: gather_delta, viscous, batched, partner words (GenArgs::nbr)
  bool les = false;          // its LESG form: a closure with an SGS flux (every model but SVV, which only filters the state)
  int update_waves = 4;      // update kernel: option general_update_waves (4, 8), else 4 where general_update_batched holds, else 8
  size_t flux_lds = 0, update_lds = 0;
  bool fold = false;         // option fold_general: P4 applies GeneralData::o2f (opp_2 - opp_3 opp_1) instead of o2; no norm_tdisf
};
GeneralPlan general_plan(const hfx_eles *e);

struct GenArgs
{
  int n_eles, nu, nfp, KU, KF, MU, MF;
  unsigned inv_nu, inv_nfp; // floor(2^32 / n) + 1: q / n == __umulhi(q, inv) for the q < 2^16 of the staging loops
  const double *o0, *o1[3], *o2[3], *o3, *o4[3], *o5[3], *o6;
  const double *u0, *delta, *disu;
  // fold != 0: o2[d] holds opp_2[d] - opp_3 opp_1[d], so that P4 leaves div_tdisf - opp_3 norm_tdisf in `div` and norm_tdisf is
  // neither formed nor stored; the update kernel then adds opp_3 norm_tconf alone (as split3's folded correction)
  int fold;
  // the LDG correction of a flux point whose partner lies in the SAME element block is formed in the flux kernel from the
  // partner's flux-point solution: (partner offset << 4) | partner's block << 2 | beta sign flipped << 1 | this point is the right
  // side; -1: a boundary point (its correction is in `delta`).  NULL: `delta` holds all of them.
  const int *nbr;
  const double *disu_b[4]; // flux-point solution of the blocks a partner word may name (its bits 3:2), and their plane strides
  long plane_b[4];
  const double *detjac_upts, *JGinv_upts, *detjac_fpts, *JGinv_fpts, *norm_fpts;
  const unsigned char *meta;
  double *div, *ntd, *fn, *grad_fpts; // grad_fpts: boundary points only (NULL: no boundary faces / inviscid)
  Phys P;
  // update kernel
  double *u0w, *u1;
  const double *tconf, *div_in, *src, *dt_local;
  double *disu_next;
  unsigned long long *nan_flag;
  int adv_type, in_step, dt_local_on, write_div, need_u1;
  double dt, rk_a, rk_b;
  long long *stamps; // diagnostics (option flux_stamps): cycle counter of every wave of ONE workgroup at the phase boundaries
  // LES closure evaluated in the flux kernel (LESG form): parameters (with the Leonard terms of the similarity models), the wall
  // distance of the Smagorinsky damping, and tdA at the flux points (F_sgs . n = (F~_sgs . n~) / tdA)
  LesParams les;
  const double *les_len2, *tdA_fpts;
  // over-integration: the de-aliased transformed inviscid flux (eles::evaluate_invFlux_over_int, formed by the dense contractions
  // before this launch), taken in P3 instead of the collocated one; NULL: none
  const double *tdisf_in;
};

// ONE stage on prepared blocks (general_prepare) whose disu_fpts belong to the current state: every block's plan and kernel arguments,
// made once, and the steps (general_partitioned_stage puts the partition-face kernels and the exchanges between them)
struct GeneralStage
{
  hfx_eles *const *eles;
  hfx_inters *const *faces; // interior, boundary and (skipped by the pairwise loops) partition-face blocks
  int neb, nfb;
  std::vector<GeneralPlan> plans; // per element block, as
  std::vector<GenArgs> args;
  // this call runs the 2-D stage (one block of triangles; option blocks_2d: several two-dimensional blocks, or one of
  // quadrilaterals -- simplex2d_stage_call): every step is simplex2d.hip's, plans and args stay empty
  bool simplex2d = false;
  int in_step = 0;
  // eles::shock_capture follows this stage where a block registered it: a triangle block whose plan folds the filter
  // (Simplex2dPlan::fold_shock) runs it inside its update kernel, and general_shock_capture behind the stage passes that block by
  bool shock = true;
  GeneralStage(hfx_eles *const *eles, int neb, hfx_inters *const *faces, int nfb, int in_step, bool shock = true);
  // viscous: boundary ghost states (-> inviscid common flux, LDG common solution); face_delta_kernel unless BOTH sides' plans `gather`
  int interior_ldg() const;
  int flux_kernels() const; // behind the over-integration contraction where the block registered it
  // boundary viscous fluxes (option bdy_beside: on the side stream, beside the pairwise launch); all interior-face blocks in one launch
  int common_fluxes() const;
  int update_kernels() const; // then the disu_fpts buffers change places: the flux-point solution is the new state's
  int run() const { return interior_ldg() || flux_kernels() || common_fluxes() || update_kernels(); }
};

// drop / release the tables derived from the block's operators and face registration
void general_invalidate(hfx_eles *e);
// n_steps time steps over several element blocks (a mixed mesh) and the face blocks between them; fails loudly when a block does not
// qualify (2-D; an LES closure without an instantiated size or with over-integration); shock capturing follows every stage
int general_run_steps(hfx_eles *const *eles, int neb, hfx_inters *const *faces, int nfb, int n_steps);
// average duration (ms, HIP events on the context stream) of the stage's four steps over `reps` stages
int general_time_kernels(hfx_eles *const *eles, int neb, hfx_inters *const *faces, int nfb, int reps, double *ms);
// algorithmic HBM bytes per step, same order; every block priced from its own plan
void general_kernel_bytes(hfx_eles *const *eles, int neb, double *bytes);
// tables for these blocks unless they exist (non-zero when a block does not qualify); `faces` may hold partition-face blocks.
// partitioned: the caller is the partitioned stage (a triangle block takes partition-face blocks from it alone)
int general_prepare(hfx_eles *const *eles, int neb, hfx_inters *const *faces, int nfb, bool partitioned = false);
// the general fused stage on partitioned element blocks (comm.hip)
int general_partitioned_stage(hfx_eles *const *eles, int neb, hfx_inters *const *int_faces, int n_int, hfx_inters *const *mpi_faces,
                              int n_mpi, hfx_comm *comm, int rk, bool start, bool shock);
// the projected viscous flux array of a block (a triangle block: the 2-D simplex stage's)
const double *general_fn_fpts(const hfx_eles *e);
// eles::shock_capture of the blocks that registered it, and the flux-point values of the filtered state
int general_shock_capture(hfx_eles *const *eles, int neb);
} // namespace hfx
