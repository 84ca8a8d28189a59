// general.hpp -- the fused RK stage for general (non-tensor-product) element classes (declarations; general.hip).
#pragma once
#include "hfx_internal.hpp"

namespace hfx
{
// drop / release the tables derived from the block's operators and face registration
void general_invalidate(hfx_eles *e);
void general_destroy(hfx_eles *e);
// n_steps time steps over several element blocks (a mixed mesh) and the face blocks between them; fails loudly when a
// block does not qualify (2-D, LES, over-integration); shock capturing follows every stage (general_shock_capture)
int general_run_steps(hfx_eles *const *eles, int neb, hfx_inters *const *faces, int nfb, int n_steps);
// average duration (ms, HIP events on the context stream) of the stage's four parts over `reps` stages: face_delta,
// flux kernels (all blocks), face_flux, update kernels (all blocks)
int general_time_kernels(hfx_eles *const *eles, int neb, hfx_inters *const *faces, int nfb, int reps, double *ms);
// algorithmic HBM bytes per launch group, same order
void general_kernel_bytes(hfx_eles *const *eles, int neb, double *bytes);
// the whole stage, or one of its four launch groups (timed on their own; the partitioned driver puts the partition-face kernels
// and the exchanges between them): boundary ghost states + LDG corrections of the interior pairs, the flux kernels of all blocks,
// interior common fluxes + boundary viscous fluxes, the update kernels of all blocks
enum class GeneralPart { stage, ldg, flux, faces, update };
// tables for these blocks unless they exist (non-zero when a block does not qualify); `faces` may hold partition-face blocks
int general_prepare(hfx_eles *const *eles, int neb, hfx_inters *const *faces, int nfb);
// ONE stage, or one part of it, on prepared blocks whose disu_fpts belong to the current state
int general_stage(hfx_eles *const *eles, int neb, hfx_inters *const *faces, int nfb, int in_step, bool write_div, GeneralPart which);
// the projected viscous flux array of a block
const double *general_fn_fpts(const hfx_eles *e);
// eles::shock_capture of the blocks that registered it, and the flux-point values of the filtered state
int general_shock_capture(hfx_eles *const *eles, int neb);
} // namespace hfx
