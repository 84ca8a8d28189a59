// simplex2d.hpp -- the fused RK stage for two-dimensional simplex blocks (triangles): a block's plan and the stage's steps
// (simplex2d.hip).  The host side of the general stage (general.hip: general_prepare, GeneralStage, general_time_kernels,
// general_kernel_bytes) branches here for a block with n_dims == 2 of a non-tensor class -- and, with option blocks_2d, for several
// two-dimensional blocks or a block of quadrilaterals (simplex2d_takes, simplex2d_runs); nothing else calls these.
#pragma once
#include "hfx_internal.hpp"

namespace hfx
{
// the triangle orders with kernel instantiations: solution / flux points of P1..P5 and the elements of a group.  THE list: the
// dispatch, the plan and the byte counts read it
constexpr int SIMPLEX2D_SIZES[][3] = {{3, 6, 64}, {6, 9, 64}, {10, 12, 32}, {15, 15, 32}, {21, 18, 16}};
constexpr int N_SIMPLEX2D_SIZES = sizeof(SIMPLEX2D_SIZES) / sizeof(SIMPLEX2D_SIZES[0]);
constexpr int SIMPLEX2D_WAVES = 4;
// the quadrilateral orders P1..P4 on the same dense kernels (option blocks_2d: a quadrilateral block beside triangles, or alone): the
// PLAIN element and update kernels only.  Size classes N_SIMPLEX2D_SIZES + 0..3; P5 (36 and 24 points) does not fit: its element
// operators alone are 82 944 bytes
constexpr int QUAD2D_SIZES[][3] = {{4, 8, 64}, {9, 12, 32}, {16, 16, 16}, {25, 20, 8}};
constexpr int N_QUAD2D_SIZES = sizeof(QUAD2D_SIZES) / sizeof(QUAD2D_SIZES[0]);
constexpr int N_S2D_CLASSES = N_SIMPLEX2D_SIZES + N_QUAD2D_SIZES;
// row {solution points, flux points, elements of a group} of a size class of either table
constexpr const int *s2d_class_row(int i) { return i < N_SIMPLEX2D_SIZES ? SIMPLEX2D_SIZES[i] : QUAD2D_SIZES[i - N_SIMPLEX2D_SIZES]; }
// LDS image of a workgroup (doubles): the operators, staged once per workgroup, then a group's planes [row][element + 1 pad][.]
constexpr size_t simplex2d_element_ops(int nu, int nfp) { return (size_t)4 * nu * nu + (size_t)6 * nu * nfp; } // o4 o5 o6 o0 o2 o1
// (shock: the update kernel with the shock filter folded in stages inv_vandermonde and exp_filter behind them)
constexpr size_t simplex2d_update_ops(int nu, int nfp, bool shock = false) { return (size_t)2 * nu * nfp + (shock ? (size_t)2 * nu * nu : 0); } // o3 o0 [iv ef]
constexpr size_t simplex2d_element_lds_bytes(int nu, int nfp, int g) { return sizeof(double) * (simplex2d_element_ops(nu, nfp) + (size_t)(g + 1) * (12 * nu + 4 * nfp)); }
// (shock: + the squared modal coefficients [element + 1 pad][mode] and the group's sensors)
constexpr size_t simplex2d_update_lds_bytes(int nu, int nfp, int g, bool shock = false)
{
  return sizeof(double) * (simplex2d_update_ops(nu, nfp, shock) + (size_t)(g + 1) * (4 * nu + 4 * nfp + (shock ? nu + 1 : 0)));
}
constexpr size_t SIMPLEX2D_LDS_BUDGET = 80 * 1024; // two workgroups per CU
// the first mode of total degree p on a triangle of order p with nu = (p + 1)(p + 2) / 2 solution points: p (p + 1) / 2 -- the
// modes the sensor of eles_tris::shock_det_persson sums in its numerator
constexpr int simplex2d_first_high_mode(int nu)
{
  int p = 0;
  while ((p + 1) * (p + 2) / 2 < nu) p++;
  return p * (p + 1) / 2;
}
// over_int_order of a triangle cubature rule with n points, (o + 1)(o + 2) / 2 for o = 0..7; -1: no such rule
constexpr int simplex2d_cubature_order(int n)
{
  for (int o = 0; o <= 7; o++)
    if ((o + 1) * (o + 2) / 2 == n) return o;
  return -1;
}
constexpr bool simplex2d_sizes_fit()
{
  bool ok = true;
  for (const auto &s : SIMPLEX2D_SIZES)
    ok = ok && simplex2d_element_lds_bytes(s[0], s[1], s[2]) <= SIMPLEX2D_LDS_BUDGET && simplex2d_update_lds_bytes(s[0], s[1], s[2], true) <= SIMPLEX2D_LDS_BUDGET;
  for (const auto &s : QUAD2D_SIZES) // (the plain forms alone; at most two points of a group per lane)
    ok = ok && simplex2d_element_lds_bytes(s[0], s[1], s[2]) <= SIMPLEX2D_LDS_BUDGET && simplex2d_update_lds_bytes(s[0], s[1], s[2]) <= SIMPLEX2D_LDS_BUDGET &&
         s[0] * s[2] <= 2 * 64 * SIMPLEX2D_WAVES;
  return ok;
}
static_assert(simplex2d_sizes_fit(), "a group of an instantiated triangle or quadrilateral order no longer leaves room for two workgroups per CU");

// What the stage runs on one block: decided once, from the options and the block's sizes and tables
struct Simplex2dPlan
{
  int size_class = -1; // triangles: index in SIMPLEX2D_SIZES (order - 1); quadrilaterals: N_SIMPLEX2D_SIZES + index in QUAD2D_SIZES
  int group = 0;       // elements per group
  int waves = SIMPLEX2D_WAVES;
  bool gather = false; // the element kernel forms the LDG corrections of interior points itself (option gather_delta, viscous)
  size_t element_lds = 0, update_lds = 0;
  // the block registered shock capturing in the form of eles_tris::shock_det_persson and option fold_shock is on: a stage that
  // eles::shock_capture follows runs the update kernel's SHOCK instantiation (LDS image update_shock_lds) and no filter behind it
  bool fold_shock = false;
  size_t update_shock_lds = 0;
  // the block registered over-integration (hfx_eles_set_over_int): n_cubpts cubature points, walked by the element kernel's OVERINT
  // instantiation in chunks of over_int_chunk (= the order's solution points) where fold_over_int -- option fold_over_int, every
  // instantiated order -- and else formed by hfx_eles_evaluate_invFlux_over_int in front of the element kernel, which then reads
  // tdisf_upts.  The element kernel's LDS image is element_lds in every form
  bool over_int = false, fold_over_int = false;
  int n_cubpts = 0, over_int_chunk = 0;
  // the block registered an LES closure with an SGS flux (sgs_model 0, 1, 2, 4) whose Jacobian_fpts is the block's own, on a viscous
  // context: the element kernel's LES instantiation evaluates it and Fn carries F_sgs . n (LDS image element_lds).  les_terms: the
  // similarity models (2, 4) read Lu / Le, which hfx_eles_calc_sgs_terms leaves in front of a step's first stage
  // (first_stage_closure_filter).  sgs_model: of the registration, -1 without one (3, SVV: the plain kernels)
  bool les = false, les_terms = false;
  int sgs_model = -1;
};

// The partitioned stage's side of the plan (general_partitioned_stage, comm.hip): the kernels walk GROUPS of `group` consecutive
// elements, and a group is a partition group when one of its elements owns a partition flux point
struct Simplex2dPartitionPlan
{
  int partition_groups = 0, interior_groups = 0;
  // the element kernel reads the partners of partition points from the receive record itself (gather, ONE partition-face block);
  // else mpi_delta_kernel<2> writes their corrections to delta_disu_fpts
  bool gather_remote = false;
};
// which groups a launch of the element / update kernel walks
enum class S2dList { all, interior, partition };

inline bool is_simplex2d(const hfx_eles *e) { return e && e->n_dims == 2 && e->ele_type == 0; } // a block of triangles
// this block's tables are the 2-D stage's and the stage runs it: a triangle block, or -- option blocks_2d -- a quadrilateral block the
// stage has prepared.  What dispatches a STAGE asks here, what is specific to triangles asks is_simplex2d
bool simplex2d_runs(const hfx_eles *e);
// a call over these blocks runs the 2-D stage (every one of them simplex2d_runs)
bool simplex2d_stage_call(hfx_eles *const *eles, int neb);
// is this call for simplex2d_prepare?  One triangle block, as ever; with option blocks_2d any call with a two-dimensional block but
// the partitioned loop's over ONE quadrilateral block (the split stage's)
bool simplex2d_takes(hfx_eles *const *eles, int neb, bool partitioned);
// tables for the block unless they exist; refuses (naming fused 0) what the stage is not built for.  partitioned: the call comes
// from the partitioned stage, which alone takes partition-face blocks
int simplex2d_prepare(hfx_eles *const *eles, int neb, hfx_inters *const *faces, int nfb, bool partitioned);
void simplex2d_invalidate(hfx_eles *e);
Simplex2dPlan simplex2d_plan(const hfx_eles *e);
Simplex2dPartitionPlan simplex2d_partition_plan(const hfx_eles *e);
// the four steps of ONE stage on prepared blocks whose disu_fpts belong to the current state (GeneralStage's, in its order).  The
// two face steps walk ALL face blocks of the call (e: any block of it), the element and update kernels are launched block by block
int simplex2d_interior_ldg(hfx_eles *e, hfx_inters *const *faces, int nfb);
// the unfolded form of a registered over-integration (plan: over_int, not fold_over_int): hfx_eles_evaluate_invFlux_over_int on the
// whole block, ONCE per stage in front of the element launches; nothing in every other form
int simplex2d_over_int_unfolded(hfx_eles *e);
int simplex2d_element_kernel(hfx_eles *e, int in_step, S2dList list = S2dList::all); // an empty list launches nothing
int simplex2d_common_fluxes(hfx_eles *e, hfx_inters *const *faces, int nfb);
// S2dList::all: then the disu_fpts buffers change places; a launch on a list leaves that to simplex2d_swap_disu_fpts, called once
// behind both lists' launches
// shock: eles::shock_capture follows this stage (folded into the launch where the plan says fold_shock; else the caller runs it)
int simplex2d_update_kernel(hfx_eles *e, int in_step, S2dList list = S2dList::all, bool shock = true);
// the stage's update kernel carries the block's shock filter: nothing runs behind the stage for it
bool simplex2d_folds_shock(const hfx_eles *e);
void simplex2d_swap_disu_fpts(hfx_eles *e);
// the projected viscous flux array of the block (what a partition face sends; with an LES closure it carries F_sgs . n as well)
const double *simplex2d_fn_fpts(const hfx_eles *e);
// algorithmic HBM bytes per step, added to bytes[0..3]
void simplex2d_kernel_bytes(const hfx_eles *e, double *bytes);
// What ONE stage over the prepared blocks launches (hfx_simplex2d_stage_plan): counted by the predicates the launches use
struct Simplex2dStagePlan
{
  int blocks = 0;
  int interior_face_blocks = 0, cross_face_blocks = 0; // (non-empty ones; cross: left != right)
  int delta_launches = 0;                              // face_delta_kernel<2> per stage
  int launches = 0;                                    // all of a stage: boundary sweeps, delta, element, face flux, update
};
Simplex2dStagePlan simplex2d_stage_plan(hfx_eles *const *eles, int neb);
} // namespace hfx
