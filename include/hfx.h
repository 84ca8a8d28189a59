/* hfx.h -- C ABI of libhfx: the MI355X (gfx950) implementation of the HiFiLES
 * per-RK-stage hot path.
 *
 * The reference has no FFI: the seam this library sits behind is the C++ class
 * API of `eles`, `int_inters` (`bdy_inters`, `mpi_inters`) that
 * CalcResidual (/root/reference/src/solver.cpp:50-223) and the RK loop
 * (/root/reference/src/HiFiLES.cpp:201-217) call, plus the legacy `_GPU` seam
 * (include/cuda_kernels.h:31-120, hf_array::cp_cpu_gpu / cp_gpu_cpu
 * include/hf_array.h:541-580).  Every entry point below names the reference
 * method it replaces.  All arrays are `double`, column-major in the hf_array
 * layout (include/hf_array.h:303-325): a(i,j,k,l) = data[i + d0*(j + d1*(k + d2*l))].
 *
 * Conventions
 *  - plain pointers and sizes only; opaque handles own all device state
 *  - every function returns 0 on success, non-zero on error; the message is
 *    available from hfx_last_error() (the reference's FatalError = print + exit,
 *    include/error.h:33-43; the adapter maps non-zero to FatalError)
 *  - not re-entrant per context; one context <-> one device (the reference is
 *    single-threaded per rank, one rank <-> one device, src/geometry.cpp:97)
 *  - the authoritative copy of the state lives on the device between explicit
 *    hfx_eles_download() calls (placed where the legacy code had cp_*_gpu_cpu,
 *    src/eles.cpp:998-1062)
 */
#ifndef HFX_H
#define HFX_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hfx_ctx hfx_ctx;
typedef struct hfx_eles hfx_eles;
typedef struct hfx_inters hfx_inters;

/* Frozen scalars the path reads from the reference's global `run_input`
 * (include/input.h; src/input.cpp:138-187,596-614; data/RK_coeff.dat). */
typedef struct hfx_params
{
  double gamma, prandtl, rt_inf, mu_inf, c_sth, fix_vis;
  double ldg_beta, ldg_tau;
  double dt;
  int viscous;
  int riemann_solve_type;     /* 0 Rusanov, 2 RoeM, 3 HLLC (src/int_inters.cpp:185-205) */
  int vis_riemann_solve_type; /* 0 LDG (the only one the reference implements) */
  int adv_type;               /* 0 Euler, 1 RK24, 2 RK34, 3 RK45, 4 RK414 (src/eles.cpp:1080) */
  int dt_type;                /* 0/1 one dt for all elements, 2 per-element dt_local */
  int n_rk;
  double RK_a[16], RK_b[16];
} hfx_params;

/* Registration data of one element class = what a constructed reference
 * `eles` object holds (include/eles.h:659-899).  Host pointers; copied once. */
typedef struct hfx_eles_desc
{
  int n_eles, n_upts, n_fpts, n_fields, n_dims;
  int ele_type; /* 0 tri, 1 quad, 2 tet, 3 pri, 4 hex (include/eles.h "ele_type") */
  int order;
  const double *opp_0;    /* (n_fpts,n_upts)  src/eles.cpp:3074 */
  const double *opp_1[3]; /* (n_fpts,n_upts)  :3145 */
  const double *opp_2[3]; /* (n_upts,n_upts)  :3230 */
  const double *opp_3;    /* (n_upts,n_fpts)  :3320 */
  const double *opp_4[3]; /* (n_upts,n_upts)  :3375 ; NULL when inviscid */
  const double *opp_5[3]; /* (n_upts,n_fpts)  :3455 ; NULL when inviscid */
  const double *opp_6;    /* (n_fpts,n_upts)  :3540 ; NULL when inviscid */
  const double *detjac_upts; /* (n_upts,n_eles)               src/eles.cpp:4048 */
  const double *JGinv_upts;  /* (n_dims,n_dims,n_upts,n_eles)  :4050 */
  const double *detjac_fpts; /* (n_fpts,n_eles)               :4230 */
  const double *JGinv_fpts;  /* (n_dims,n_dims,n_fpts,n_eles)  :4233 */
  const double *tdA_fpts;    /* (n_fpts,n_eles)               :4234 */
  const double *norm_fpts;   /* (n_fpts,n_eles,n_dims)        :4235 */
} hfx_eles_desc;

/* arrays of an element block addressable by upload/download */
enum hfx_array_id
{
  HFX_DISU_UPTS0 = 0,   /* disu_upts(0)      (n_upts,n_eles,n_fields) */
  HFX_DISU_UPTS1 = 1,   /* disu_upts(1) */
  HFX_DISU_FPTS = 2,    /* (n_fpts,n_eles,n_fields) */
  HFX_TDISF_UPTS = 3,   /* (n_upts,n_eles,n_fields,n_dims) */
  HFX_NORM_TDISF_FPTS = 4,
  HFX_NORM_TCONF_FPTS = 5,
  HFX_DIV_TCONF_UPTS = 6, /* div_tconf_upts(0) */
  HFX_DELTA_DISU_FPTS = 7,
  HFX_GRAD_DISU_UPTS = 8, /* (n_upts,n_eles,n_fields,n_dims) */
  HFX_GRAD_DISU_FPTS = 9, /* (n_fpts,n_eles,n_fields,n_dims) */
  HFX_SRC_UPTS = 10,      /* (n_upts,n_eles,n_fields); zero unless uploaded */
  HFX_DT_LOCAL = 11,      /* (n_eles) */
  HFX_SENSOR = 12,        /* (n_eles) eles::sensor, written by hfx_eles_shock_capture */
  HFX_SGSF_UPTS = 13,     /* (n_upts,n_eles,n_fields,n_dims) LES: transformed SGS flux (allocated by hfx_eles_set_les) */
  HFX_SGSF_FPTS = 14,     /* (n_fpts,n_eles,n_fields,n_dims) LES: physical SGS flux at the flux points */
  HFX_DISUF_UPTS = 15,    /* (n_upts,n_eles,n_fields) LES closures 2-4: filtered solution (hfx_eles_set_les_filter allocates 15-17) */
  HFX_LU = 16,            /* (n_upts,n_eles,3|6) Leonard tensor of the similarity term */
  HFX_LE = 17,            /* (n_upts,n_eles,n_dims) Leonard vector */
  HFX_N_ARRAYS = 18
};

/* which implementation the operator contractions use */
enum hfx_contract_mode
{
  HFX_CONTRACT_AUTO = 0,   /* sparse when the registered operator is sparse enough, else dense */
  HFX_CONTRACT_DENSE = 1,  /* dense FP64 MFMA GEMM, as the reference's sparse_* = 0 */
  HFX_CONTRACT_SPARSE = 2  /* exact-zero skipping, as the reference's sparse_* = 1 (src/eles.cpp:3114) */
};

const char *hfx_last_error(void);
int hfx_version(void);

/* ---- context ---------------------------------------------------------- */
int hfx_ctx_create(int device, hfx_ctx **out);
int hfx_ctx_destroy(hfx_ctx *ctx);
int hfx_ctx_set_params(hfx_ctx *ctx, const hfx_params *p);
int hfx_ctx_set_contract_mode(hfx_ctx *ctx, int mode);
/* which variant of the split fused stage (pairwise face kernels + element kernels, three or four launches per stage) the
 * measurement entry points describe and hfx_stage_partitioned / hfx_run_steps_partitioned run: 2 keeps the reference's
 * gradient arrays in HBM, 3 (default) evaluates the fluxes in the gradient kernel.  Hexahedra of orders 6 and 7 (343 / 512
 * solution points) run variant 2 whichever is asked for: variant 3 does not fit one such element in LDS.  Variant 2 has no
 * over-integration, so such a block with over-integration stays on the per-method path (deferred execution replays it). */
int hfx_ctx_set_fused_mode(hfx_ctx *ctx, int mode);
/* run_input.CFL for dt_type 1 / 2 (src/input.cpp:141-158): hfx_run_steps and hfx_run_steps_partitioned then start every
 * time step with calc_time_step (src/HiFiLES.cpp:198, src/solver.cpp:484-549) */
int hfx_ctx_set_CFL(hfx_ctx *ctx, double CFL);
/* Measurement knobs: kernel variants with the same results (A/B runs; defaults are the product path).  name:
 * "split_grid_per_cu" (0 = the workgroups resident at once | n), "persistent_grid_cap" (0 = off | n: every persistent element kernel -- the
 * split stage's flux, gradient, update and residual kernels, the sum-factorised over-integration and shock-capturing kernels -- is launched with
 * min(its usual grid, n) workgroups, so that a mesh of a few elements runs their element loops past the first iteration; results do not change,
 * hfx_fused_launch_grids reports the grids), "xcd_order" (1), "dictionary_rows" (0), "flux_waves" (2 | 3), "buffer_addressing" (1),
 * "loader_wave" (1), "fold_general" (1: the general fused stage applies opp_2 - opp_3 opp_1 and never forms norm_tdisf), "gather_delta" (1: the loader-wave flux kernel forms the interior LDG corrections itself, no pairwise
 * LDG launch), "simd_roles" (1: the flux kernel deals its waves' parts by SIMD), "flux_two_wave" (1: on P4 hexahedra the affine flux kernel runs as
 * two-wave workgroups, four resident per CU; 0: its loader-wave form; hfx_time_fused_kernels lists "two_wave" behind the kernels when it runs), "fold_faces" (1: in a viscous run with
 * |ldg_beta| = 1/2 and a Riemann solver other than RoeM the two-wave flux kernel forms the common flux of the interior pairs itself -- the point whose projected viscous flux has the
 * non-zero weight writes norm_tconf of both sides -- and the stage launches no face_flux2_kernel on interior faces; hfx_time_fused_kernels then
 * lists "folded_faces" and reports 0.0 ms for the face kernel when the step launched nothing; 0: the three-launch stage, bit for bit as before),
 * "flux_two_wave_face" (-1: the library's choice | 0-5: the local face that carries the two-wave kernel's left-over points, reported by
 * hfx_flux_two_wave_face; results agree to rounding, the forced face makes the left-over pass of the kernel's point physics run), "comm_stream_faces" (1:
 * hfx_run_steps_partitioned launches the one-sided partition-face kernels on the communication stream), "flux_stamps" (0; n >= 1: cycle
 * stamps of iteration max(n, 2) of one workgroup of the flux kernels, printed by the hfx_time_* entry points), "tensor_ops" (1),
 * "split_flux" (1: hfx_run_steps_partitioned runs the flux kernel in three launches -- half of the elements without partition-face points,
 * those with, the other half -- so that both exchanges run beside element work), "split_update" (1: hfx_run_steps_partitioned updates the elements with partition-face points in a first launch, so that their exchange
 * runs beside the update of the others), "light_wave_short" (1: a flux-kernel wave without solution points runs the flux-point physics alone), "les_flux_kernel" (1: the LES
 * closure inside the flux kernel of variant 3), "over_int_fold" (1: the sum-factorised over-integration kernel hands the loader-wave flux kernel its
 * contribution to the divergence, n_fields values per solution point, instead of tdisf_upts), "fold_over_int" (1: the 2-D simplex
 * stage's element kernel carries a triangle block's registered over-integration; 0: the per-method launches in front of it), "blocks_2d" (0; 1: fused 4 takes several two-dimensional
 * blocks -- a mixed quadrilateral / triangle mesh -- and a block of quadrilaterals of orders 1-4 on the 2-D simplex stage, see hfx_simplex2d_stage_plan), "bdy_beside" (0; 1: the fused stages' viscous boundary-face kernels on a side stream
 * beside the interior-face kernel), "affine_metrics" (1: on a block whose elements are all parallelepipeds -- metrics constant inside an
 * element up to rounding, detected when the fused tables are made -- the split stage's flux and update kernels read one 34-double metric record per element in place of
 * the per-point metric arrays (all but JGinv at the solution points); results agree with 0 to rounding, hfx_time_fused_kernels then lists "affine_metrics" behind the kernels), "general_waves" (0 = by LDS image | 3 | 4 | 8), "general_update_waves" (0 = by the staging registers | 4 | 8), "dense_waves" (0 = by the operator's rows | 4 | 8) and "dense_split" (0 | 1 | 2 | 4:
 * shape of the dense MFMA contraction's workgroup) -- see hfx_ctx::Options in csrc/hfx_internal.hpp; and "deferred" (0), which is
 * not a measurement knob: see below;
 * tests/test_gpu_fused.py::test_split3_variant_knobs_agree holds the variants to each other. */
int hfx_ctx_set_option(hfx_ctx *ctx, const char *name, int value);
/* ---- deferred execution: the reference's UNCHANGED call sequence on the fused stages --------------------------------
 * hfx_ctx_set_option(ctx, "deferred", 1).  From then on the per-method entry points below -- exactly the calls
 * CalcResidual (src/solver.cpp:59-221) and the RK loop (src/HiFiLES.cpp:201-217) make: hfx_eles_extrapolate_solution ...
 * hfx_eles_calculate_corrected_divergence, hfx_eles_calc_sgs_terms, hfx_eles_extrapolate_sgsFlux,
 * hfx_int_inters_calculate_common_*, hfx_bdy_inters_evaluate_boundaryConditions_*, hfx_mpi_inters_send_* / receive_* /
 * calculate_common_*, hfx_eles_AdvanceSolution, hfx_eles_shock_capture -- RECORD the call and return.  The record runs
 * when the next stage begins (the first call behind an AdvanceSolution / shock_capture) or when any other entry point needs
 * the device state (upload, download, monitors, calc_dt_local, new parameters, synchronize, hfx_ctx_flush ...):
 *   - a record that is one whole stage in CalcResidual's order (every method over every block it belongs to, phases in
 *     the reference's order, one stage number) runs as ONE fused stage: the split stage for a tensor-product block
 *     (= hfx_run_steps(..., 3), or 2 in fused mode 2 / with an LES closure the flux kernel cannot carry), the partitioned split
 *     stage when the block has partition faces whose send_* / receive_* calls name one hfx_comm (= hfx_run_steps_partitioned),
 *     the general stage for tetrahedra / prisms / mixed meshes (= hfx_run_steps_blocks(..., 4)), with partition faces
 *     = hfx_run_steps_partitioned_blocks;
 *   - anything else -- a partial stage, another order, a block the fused stages refuse, the packing halves
 *     hfx_mpi_inters_pack_* of a caller-side transport -- is replayed call by call: the per-method path, unchanged.
 * Results are those of hfx_run_steps* (1e-11 of the per-method path).  The fused stages leave disu_upts(0),
 * disu_upts(1), disu_fpts of the new state, and div_tconf_upts at the last stage of a step (where the monitors read it,
 * src/output.cpp:2166) or when a pending stage is flushed by a request for it.  A download of any OTHER array that arrives
 * while a whole stage is pending makes that stage run call by call, so that the caller sees the reference's values (a
 * monitor that reads grad_disu_upts after a step, src/eles.cpp:5485, costs one per-method stage); once the next stage has
 * begun such an array is stale and its download FAILS rather than return older values.
 * An error in a recorded call surfaces at the entry point that makes the record run.
 * The stale marks hold whether or not the option is on: switching "deferred" off after a fused stage does not make the arrays it
 * left stale readable.  hfx_eles_destroy / hfx_inters_destroy run what has been recorded before the block goes (a stage left
 * pending behind its AdvanceSolution belongs to every block of the context); a failure of that run is their return value.
 * Partition faces: a partitioned fused stage ends with the NEXT state's flux-point solution already posted.  Whatever follows
 * -- that stage replayed call by call, calls made with the option off, hfx_run_steps_partitioned(_blocks) -- takes that message
 * instead of posting it again (send_solution posts nothing, receive_solution waits for it), so replay and flush decisions,
 * which are a rank's own, never change the number of messages a rank posts: that follows the partition-face calls alone
 * (hfx_comm_exchange_stats counts them).  An upload of the state, a device pointer to it or a closure that filters it waits for
 * such a message first and drops it; hfx_ctx_synchronize also waits for the communication streams that carry one. */
int hfx_ctx_flush(hfx_ctx *ctx); /* run what has been recorded (asynchronously, on the context's stream); no-op otherwise */
/* Several readers behind one step.  Every entry point that reads device state makes a pending stage run so that ITS arrays hold the
 * reference's values: the time averages and the probes read the state alone and let the stage run fused, and a stage that has run
 * fused cannot give a later reader -- hfx_eles_sample_integral_quantities with an id 1-4, hfx_eles_sample_history with viscous
 * forces, hfx_eles_sample_plot with vorticity or a Q criterion -- the gradient it kept on chip: that reader is refused.  A caller
 * that is about to take several of these samples behind the step just recorded (the main loop of src/HiFiLES.cpp:221-297 takes
 * them all) says so BEFORE the first reader: `which` is the sum of 1 (integral quantities), 2 (history row) and 4 (plot snapshot).
 * The pending record then runs once, so that the union of what those samples read of these blocks is in memory -- call by call
 * where one of them reads the gradient, fused otherwise, exactly as the sample would have asked had it come first.  A monitor the
 * context does not have, or a block without its cubature, wall faces or plot points, counts for nothing; which 0, no pending
 * record or no deferred execution: hfx_ctx_flush.  Nothing is sampled. */
int hfx_flush_for_samples(hfx_eles *const *eles, int n_ele_blocks, int which);
/* stages run fused / records replayed call by call since the context was created, and why the last replay was one */
int hfx_ctx_deferred_stats(hfx_ctx *ctx, long *n_fused, long *n_replayed, const char **why_last_replay);
/* run_input.dt as the last calc_time_step left it (dt_type 1), or as set (dt_type 0) */
int hfx_ctx_get_dt(hfx_ctx *ctx, double *dt);
/* ---- the clock of the step loops (src/HiFiLES.cpp:221-245) ----------------------------------------------------------
 * The caller keeps FlowSol.time and i_steps; hfx_ctx_set_clock hands both to the library.  From then on the four loops
 * hfx_run_steps, hfx_run_steps_blocks, hfx_run_steps_partitioned and hfx_run_steps_partitioned_blocks do after EVERY time step
 * what the reference's main loop does there: time += run_input.dt; i_steps++; if (i_steps == 1) spinup_time = time; and then
 * eles::CalcTimeAverageQuantities of every block that registered average fields (hfx_eles_set_average_fields) -- one more
 * kernel per such block and step on the compute stream, nothing at all for a context without average fields -- and, when
 * i_steps % probe_freq == 0, one sample of every block that has probes (hfx_ctx_set_probes, hfx_eles_set_probes).  A context
 * whose clock was never set is the caller's to time: its loops touch neither the clock nor the averages, and the caller calls
 * hfx_eles_CalcTimeAverageQuantities itself where the reference does.  spinup_time is kept across calls (0 in a new
 * context); setting i_steps = 0 makes the next step the one that sets it, which restarts the averages' weights as a restarted
 * reference run does.  The hfx_time_* entry points never touch the clock. */
int hfx_ctx_set_clock(hfx_ctx *ctx, double time, int i_steps);
int hfx_ctx_get_clock(hfx_ctx *ctx, double *time, int *i_steps, double *spinup_time); /* any pointer may be NULL */
/* run_input.spinup_time of a run that is continued with i_steps > 0 in another context than the one that made its first step */
int hfx_ctx_set_spinup_time(hfx_ctx *ctx, double spinup_time);
/* runs what has been recorded and waits for the context's stream and for the communication stream of every hfx_comm of the
 * context that has a solution message in flight */
int hfx_ctx_synchronize(hfx_ctx *ctx);
/* the HIP stream (hipStream_t) all kernels of this context are launched on */
void *hfx_ctx_stream(hfx_ctx *ctx);

/* ---- element blocks (reference class eles) ----------------------------- */
int hfx_eles_create(hfx_ctx *ctx, const hfx_eles_desc *desc, hfx_eles **out);
int hfx_eles_destroy(hfx_eles *e);
/* replaces hf_array::cp_cpu_gpu / cp_gpu_cpu (include/hf_array.h:541-580) */
int hfx_eles_upload(hfx_eles *e, int array_id, const double *host);
/* A download of grad_disu_upts / grad_disu_fpts is refused ("was not materialised ...") after a fused stage that keeps the
 * corrected gradients on chip -- split variant 3, the general stage; through hfx_run_steps*, the partitioned loops,
 * hfx_stage_partitioned, the timing entry points or deferred execution -- until a per-method stage, split variant 2 or an
 * upload writes them again: the arrays then hold an older stage's values. */
int hfx_eles_download(hfx_eles *e, int array_id, double *host);
/* deferred execution: *current = 1 when the array holds the last stage's values; 2 when it does not yet but a whole stage is
 * pending that a download of this array would run call by call (and so refresh it); 0 when the fused stage that ran last did
 * not refresh it and nothing pending will (its download would fail) */
int hfx_eles_is_current(hfx_eles *e, int array_id, int *current);
/* raw device pointer of an array (for zero-copy interop with a resident caller) */
int hfx_eles_device_ptr(hfx_eles *e, int array_id, double **dev);

int hfx_eles_extrapolate_solution(hfx_eles *e);           /* eles::extrapolate_solution           src/eles.cpp:1360 */
int hfx_eles_calculate_gradient(hfx_eles *e);             /* eles::calculate_gradient             :1823 */
int hfx_eles_evaluate_invFlux(hfx_eles *e);               /* eles::evaluate_invFlux               :1415 */
int hfx_eles_correct_gradient(hfx_eles *e);               /* eles::correct_gradient               :1890 */
int hfx_eles_evaluate_viscFlux(hfx_eles *e);              /* eles::evaluate_viscFlux              :2285 */
int hfx_eles_extrapolate_totalFlux(hfx_eles *e);          /* eles::extrapolate_totalFlux          :1549 */
int hfx_eles_calculate_divergence(hfx_eles *e);           /* eles::calculate_divergence           :1651 */
int hfx_eles_calculate_corrected_divergence(hfx_eles *e); /* eles::calculate_corrected_divergence :1738 */
int hfx_eles_AdvanceSolution(hfx_eles *e, int in_step, int adv_type); /* eles::AdvanceSolution    :1080 */
/* the NaN scan of src/eles.cpp:1781-1795 as a device flag: *first_nan = flat index
 * into div_tconf_upts(0) of a NaN seen since the last call, or -1.  Synchronizes. */
int hfx_eles_check_nan(hfx_eles *e, long *first_nan);
/* eles::compute_res_upts (src/eles.cpp:5045): norm_type 0 max, 1 L1 sum, 2 L2 sum */
int hfx_eles_compute_res_upts(hfx_eles *e, int norm_type, int field, double *out);

/* ---- interior faces (reference class int_inters) ----------------------- */
/* L, R: (n_fpts_per_inter, n_inters) offsets `fpt + n_fpts*ele` into the
 * (fpt,ele) plane of the left / right element block: the hf_array<double*>
 * tables of include/inters.h:86-116 minus the owning array base, with the
 * flux-point permutation `lut` (src/inters.cpp:153-262) already applied to R,
 * exactly as int_inters::set_interior (src/int_inters.cpp:67-121) wires them. */
int hfx_int_inters_create(hfx_ctx *ctx, hfx_eles *left, hfx_eles *right, int n_inters, int n_fpts_per_inter,
                          const int *L, const int *R, hfx_inters **out);
int hfx_inters_destroy(hfx_inters *f);
int hfx_int_inters_calculate_common_invFlux(hfx_inters *f);  /* int_inters::calculate_common_invFlux  src/int_inters.cpp:160 */
int hfx_int_inters_calculate_common_viscFlux(hfx_inters *f); /* int_inters::calculate_common_viscFlux src/int_inters.cpp:254 */

/* ---- partition faces (reference class mpi_inters) ------------------------ */
/* A partition face has its LEFT side on this rank; the right state arrives through an exchange.
 * L: (n_fpts_per_inter, n_inters) left offsets as for interior faces.
 * Rlut: (n_fpts_per_inter, n_inters) the flux-point slot `lut(j)` of the RECEIVED face record that
 *   meets left flux point j (mpi_inters::set_mpi wires disu_fpts_r(j,i,k) to
 *   in_buffer_disu(lut(j), k, i), src/mpi_inters.cpp:165-172).
 * Buffers (device, owned by the block): out/in_buffer_disu (fpt, field, inter) and
 *   out/in_buffer_grad_disu (fpt, field, dim, inter), filled in loop order inter -> [dim ->] field -> fpt
 *   (src/mpi_inters.cpp:56-66,225-229,284-289).  Faces of one neighbour rank are contiguous, in the
 *   order both ranks agreed on (src/geometry.cpp:1184-1239), so a message is one contiguous slice.
 * The exchange moves out_buffer slices to the neighbours' in_buffer slices between `pack` and `calculate_common_*`:
 *   either inside the library (hfx_comm_*, hfx_mpi_inters_send_* / receive_* below: grouped ncclSend / ncclRecv on the
 *   library's communication stream) or by the caller (the hfx_mpi_inters_pack_* halves + its own transport). */
int hfx_mpi_inters_create(hfx_ctx *ctx, hfx_eles *left, int n_inters, int n_fpts_per_inter, const int *L,
                          const int *Rlut, hfx_inters **out);
/* the packing half of mpi_inters::send_solution / send_corrected_gradient (src/mpi_inters.cpp:218-229,278-289) */
int hfx_mpi_inters_pack_solution(hfx_inters *f);
int hfx_mpi_inters_pack_corrected_gradient(hfx_inters *f);
/* LES, the packing half of mpi_inters::send_sgsf_fpts (src/mpi_inters.cpp:339-351): out_buffer_sgsf = the left block's
 * physical SGS flux at the partition faces' flux points (after hfx_eles_extrapolate_sgsFlux) */
int hfx_mpi_inters_pack_sgsf(hfx_inters *f);
/* device pointers and lengths (doubles) of the buffers: which = 0 out_disu, 1 in_disu, 2 out_grad, 3 in_grad;
 * 4 / 5 = the leading n_fpts_per_inter*n_fields*n_inters doubles of out_grad / in_grad, which is what
 * hfx_stage_partitioned sends in fused mode 3 (the projected viscous flux instead of the gradient);
 * 6 / 7 = out / in_buffer_sgsf (LES only; (fpt, field, dim, inter) like the gradient) */
int hfx_mpi_inters_buffer(hfx_inters *f, int which, double **dev, long *n);
int hfx_mpi_inters_calculate_common_invFlux(hfx_inters *f);  /* mpi_inters::calculate_common_invFlux  src/mpi_inters.cpp:400 */
int hfx_mpi_inters_calculate_common_viscFlux(hfx_inters *f); /* mpi_inters::calculate_common_viscFlux src/mpi_inters.cpp:485 */

/* ---- LES sub-grid closure (8f-4) ----------------------------------------- */
/* run_input.LES == 1 with an eddy-viscosity model (src/eles.cpp:2395-2650): sgs_model 0 Smagorinsky with near-wall
 * damping (wall_distance (n_upts,n_eles,n_dims), eles::calc_wall_distance), 1 WALE.  Jacobian_fpts
 * (n_dims,n_dims,n_fpts,n_eles) is what extrapolate_sgsFlux uses to take the flux back to physical space
 * (src/eles.cpp:2862-2893).  Once set, evaluate_viscFlux adds the SGS flux, hfx_CalcResidual calls
 * extrapolate_sgsFlux (src/solver.cpp:162-167) and interior faces add sgsf_fpts to both sides' viscous flux
 * (src/int_inters.cpp:302-318), partition faces after the third exchange (hfx_mpi_inters_send / receive_sgsf_fpts).
 * The filter width uses the element class's calc_ele_vol (|J| times the reference element's volume: hexes 8, quads 4,
 * prisms 4, tetrahedra 8/6, triangles 2; the block's ele_type decides).
 * The fused stages evaluate the closure inside their flux kernels -- split variant 3 on hexes / quads (option "les_flux_kernel"),
 * the general stage on tetrahedra / prisms of orders 1..3 -- and add F_sgs . n to the projected viscous flux of every flux point,
 * so a partition face's second message already carries it and the third one is not sent there; hfx_run_steps(..., fused=2) keeps
 * the reference's arrays (gradients, sgsf_upts, sgsf_fpts) and the third message (hfx_stage_partitioned). */
typedef struct hfx_les
{
  int sgs_model, pad; /* 0 Smagorinsky, 1 WALE, 2 WALE + similarity, 3 spectral vanishing viscosity, 4 similarity */
  double C_s, filter_ratio, Kappa, prandtl_t;
} hfx_les;
int hfx_eles_set_les(hfx_eles *e, const hfx_les *les, const double *wall_distance, const double *Jacobian_fpts);
/* Closures 2, 3, 4 filter the solution: filter_upts (n_upts,n_upts) is what the element class builds in
 * compute_filter_upts (src/eles_hexas.cpp:583, src/eles.cpp:138) -- registered like the operators.  Required before the
 * first stage with such a model. */
int hfx_eles_set_les_filter(hfx_eles *e, const double *filter_upts);
/* eles::calc_sgs_terms (src/eles.cpp:2058-2283), which CalcResidual calls at the FIRST RK stage of a time step for the
 * closures 2, 3, 4 (src/solver.cpp:55-62): filtered solution -> HFX_DISUF_UPTS; model 3: it replaces disu_upts(0);
 * models 2 / 4: products, their filtered values and the Leonard terms -> HFX_LU, HFX_LE, which calc_sgsf_upts reads for
 * the rest of the step.  A NaN in the filtered solution is reported through hfx_eles_check_nan.  The hfx_run_steps*
 * loops call it themselves. */
int hfx_eles_calc_sgs_terms(hfx_eles *e);
int hfx_eles_extrapolate_sgsFlux(hfx_eles *e); /* eles::extrapolate_sgsFlux, src/eles.cpp:2817 */

/* ---- integral diagnostics (8f-1: the TGV monitors) ------------------------ */
/* opp_volume_cubpts (n_cubpts,n_upts), weight_volume_cubpts (n_cubpts), vol_detjac_vol_cubpts (n_cubpts,n_eles):
 * what eles::set_opp_volume_cubpts / set_transforms_vol_cubpts build when n_integral_quantities != 0
 * (src/eles.cpp:3667,4027) */
int hfx_eles_set_volume_cubpts(hfx_eles *e, int n_cubpts, const double *opp_volume_cubpts, const double *weight_volume_cubpts,
                               const double *vol_detjac_vol_cubpts);
/* eles::CalcIntegralQuantities (src/eles.cpp:5485-5627): integral_quantities[m] += this block's integral of
 * quantity quantity_ids[m] (0 kineticenergy, 1 enstropy, 2 pressuredilatation, 3 straincolonproduct,
 * 4 devstraincolonproduct) from disu_upts(0) and grad_disu_upts (the corrected gradient of the last
 * per-method / fused-mode-2 stage).  The caller adds over blocks and ranks (src/output.cpp:2017-2050). */
int hfx_eles_CalcIntegralQuantities(hfx_eles *e, int n_quantities, const int *quantity_ids, double *integral_quantities);

/* ---- the integral monitor: the Diagnostics[...] columns of history.plt sampled on the device (src/HiFiLES.cpp:247-266) ----
 * The reference fills them at step 1 and every run_input.monitor_res_freq steps (output::CalcIntegralQuantities,
 * src/output.cpp:2017; eles::CalcIntegralQuantities, src/eles.cpp:5485-5627).  A sample pairs disu_upts(0) as it stands with
 * grad_disu_upts as it stands: behind a time step that is the new state and the corrected gradient of the last RK stage's INPUT
 * state, exactly what the reference integrates.  The monitor forms no gradient of its own.  Values are per block; adding over
 * blocks and ranks is the caller's (src/output.cpp:2023-2050). */
#define HFX_MAX_INTEGRAL_QUANTITIES 8
/* The quantities of the context: quantity_ids[n_quantities] as for hfx_eles_CalcIntegralQuantities (0-4, src/eles.cpp:5540-5620;
 * anything else is refused with the reference's words, src/eles.cpp:5618), monitor_res_freq >= 1 (steps, src/input.cpp:101) and
 * the number of samples the device history of every block holds (>= 1).  n_quantities = 0 drops the monitor and empties every
 * block's history; changing the quantities empties the histories.  A quantity that reads the gradient (ids 1-4) is refused on an
 * inviscid context: the reference has no grad_disu_upts there.  Parameters (hfx_ctx_set_params) come first. */
int hfx_ctx_set_integral_monitor(hfx_ctx *ctx, int n_quantities, const int *quantity_ids, int monitor_res_freq, int capacity);
/* ONE sample of the block (which needs hfx_eles_set_volume_cubpts) into the next free slot of its device history: one fused
 * launch and one single-workgroup launch that adds the workgroups' partials in workgroup order; no array of the size of
 * n_cubpts x n_eles, no synchronisation with the host, which notes `time` and `step` for the slot.  With an id 1-4 selected a
 * pending deferred stage runs so that it leaves the gradient (as for hfx_eles_compute_wall_forces), and a gradient the last
 * fused stage did not materialise is refused with the words of hfx_eles_download.  With the kinetic energy alone the gradient is
 * never read: the sample works after any fused stage and on inviscid contexts.  A full history is refused, nothing is
 * overwritten.  Two samples of one state are equal bit for bit, in any slot (no atomics, a fixed summation order for a given grid).
 * Once the clock is the library's (hfx_ctx_set_clock) every step loop does this itself, behind the time averages and the probes,
 * for every block with a cubature after each step with i_steps == 1 || i_steps % monitor_res_freq == 0.  Such a loop first counts
 * the samples it will take and refuses the whole call, before its first launch, when a history cannot hold them.  With an id 1-4
 * selected, a loop whose stages keep the gradient on chip (fused 3 on a variant-3 plan, fused 4) runs the last RK stage of every
 * step it samples call by call -- CalcResidual, AdvanceSolution, the shock filter -- so that grad_disu_upts holds what the
 * reference's does; the partitioned loops refuse that combination before their first launch (fused mode 2 samples everything).
 * A loop without a monitor, or with the kinetic energy alone, launches exactly the stages it launched before. */
int hfx_eles_sample_integral_quantities(hfx_eles *e, double time, int step);
/* the number of stored samples (no copy, no synchronisation) */
int hfx_eles_integral_count(hfx_eles *e, int *n_samples);
/* Synchronises, copies the history -- values (n_quantities, n_samples) with the quantity index fastest, times and steps
 * (n_samples) -- and empties it.  max_samples: what the caller's arrays hold; fewer than stored is refused, nothing is lost. */
int hfx_eles_read_integral_history(hfx_eles *e, int max_samples, double *times, int *steps, double *values, int *n_samples);
/* what the next sample launches: workgroups, and the elements a workgroup takes per pass of its loop */
int hfx_eles_integral_launch(hfx_eles *e, int *n_groups, int *eles_per_pass);
/* how many of the steps i_steps + 1 .. i_steps + n_steps the reference samples (step 1 and the multiples of monitor_res_freq):
 * what the loops' capacity check counts.  Pure host arithmetic */
int hfx_integral_monitor_samples(int i_steps, int n_steps, int monitor_res_freq, int *n_samples);
/* device milliseconds of the launches of one sample, averaged over `reps` samples into a scratch slot (the history is untouched;
 * grad_disu_upts is read as it stands, whichever stage wrote it) */
int hfx_time_integral_quantities(hfx_eles *e, int reps, double *ms);

/* ---- the history monitor: the residual and force columns of history.plt sampled on the device (src/HiFiLES.cpp:247-266) ----
 * In front of the Diagnostics[...] columns a row holds log10 of the residual norm of every field (output::CalcNormResidual,
 * src/output.cpp:2166-2248) and, with calc_force, the total force, CL and CD (output::CalcForces, src/output.cpp:1915-2014).  A row
 * of a block holds the RAW values: per field the max (norm 0) or the sum (norms 1, 2) of eles::compute_res_upts over the block's
 * solution points -- div_tconf_upts(0) / detjac_upts - src_upts -- and the 2 n_dims + 2 values of hfx_eles_compute_wall_forces.
 * Adding (or taking the max) over blocks and ranks, the division by n_upts, the square root and the log10 are the caller's, as for
 * the integral monitor.  Cp and Cf per wall point (cp_*.dat, monitor_cp_freq) are not part of a row: they stay with
 * hfx_eles_compute_wall_forces.  Blocks of other than n_dims + 2 fields (RANS, advection-diffusion) are refused. */
/* res_norm_type 0, 1 or 2 as run_input.res_norm_type (src/input.cpp:108; anything else is refused with the reference's words,
 * src/output.cpp:2241); with_forces != 0: the rows carry the forces, which needs hfx_ctx_set_force_reference first;
 * monitor_res_freq >= 1; capacity >= 1: the rows the device history of every block holds.  capacity 0 drops the monitor and empties
 * the histories; any registration empties them.  The reference has ONE monitor_res_freq: when the integral monitor is registered
 * too the two must agree, and the second registration is refused otherwise.  Parameters (hfx_ctx_set_params) come first. */
int hfx_ctx_set_history_monitor(hfx_ctx *ctx, int res_norm_type, int with_forces, int monitor_res_freq, int capacity);
/* ONE row of the block into the next free slot of its device history: one launch of the residual kernel for all fields, with forces
 * and wall faces the kernel of hfx_eles_compute_wall_forces, and one single-workgroup launch that combines the workgroups' partials
 * of both in workgroup order.  No synchronisation with the host, which notes `time` and `step` for the slot; no floating-point
 * atomics: two samples of one state are equal bit for bit in any slot, and the force columns are bit for bit those of
 * hfx_eles_compute_wall_forces on the same state, gradient and grid.  A block without wall faces has zeros in its force columns.
 * Norm 0 keeps a NaN residual (the reference stops on one, src/output.cpp:2243).
 * div_tconf_upts must be current: a pending deferred stage runs so that it stores it, and a stale one is refused with the words of
 * hfx_eles_compute_res_upts.  With forces on a viscous context and a block with wall faces the pending stage also leaves the gradient,
 * and a gradient the last fused stage kept on chip is refused, exactly as for hfx_eles_compute_wall_forces.  A full history is refused.
 * Once the clock is the library's (hfx_ctx_set_clock) every step loop does this itself, behind the sample of the integral monitor
 * and under its condition, i_steps == 1 || i_steps % monitor_res_freq == 0, for every block, after counting the rows it will take:
 * a call whose rows would not fit is refused before its first launch.  Every loop stores div_tconf_upts at the last stage of every
 * step, so residuals alone, or forces on an inviscid context, leave the loop's launches and its states as they were.  With viscous
 * forces and a block with wall faces the rule of the integral monitor's ids 1-4 applies: a loop that keeps the gradient on chip
 * runs the last RK stage of a sampled step call by call; the partitioned loops refuse that combination before their first launch
 * (fused mode 2, or residuals alone). */
int hfx_eles_sample_history(hfx_eles *e, double time, int step);
/* the number of stored rows (no copy, no synchronisation) */
int hfx_eles_history_count(hfx_eles *e, int *n_rows);
/* Synchronises, copies the history -- residuals (n_fields, n_rows) and forces (2 n_dims + 2, n_rows: inviscid force, viscous force,
 * CL, CD; not touched, and may be NULL, when the monitor has no forces) with the first index fastest, times and steps (n_rows) --
 * and empties it.  max_rows: what the caller's arrays hold; fewer than stored is refused, nothing is lost. */
int hfx_eles_read_history(hfx_eles *e, int max_rows, double *times, int *steps, double *residuals, double *forces, int *n_rows);
/* what the next sample launches for the residual: workgroups, and the solution points a workgroup takes per pass of its loop */
int hfx_eles_history_launch(hfx_eles *e, int *n_groups, int *points_per_pass);
/* device milliseconds of the launches of one sample, averaged over `reps` samples into a scratch slot (the history is untouched) */
int hfx_time_history(hfx_eles *e, int reps, double *ms);

/* ---- exact-solution error norms (run_input.test_case, error_norm_type; output::compute_error, src/output.cpp:2052) ------
 * The monitor a verification run ends with (src/HiFiLES.cpp:324-325): the state -- and for Couette flow the gradient --
 * interpolated to the volume cubature points, minus the exact solution there, integrated in the L1 or L2 sense. */
typedef struct hfx_exact
{
  int test_case, pad; /* run_input.test_case: 1 isentropic vortex (src/funcs.cpp:1724-1739), 5 Couette flow (src/funcs.cpp:1830-1922) */
  /* test case 5 only: velocity(0) of the moving isothermal wall, T_static of the one at rest (src/eles.cpp:5219-5230),
   * run_input.p_c_ic, R_ref and T_ref.  gamma and prandtl are those of hfx_params */
  double u_wall, T_wall, p_bound, R_ref, T_ref;
} hfx_exact;
/* Stored as given; hfx_eles_compute_error refuses what it cannot compute.  x NULL: the context has no exact solution any more. */
int hfx_ctx_set_exact_solution(hfx_ctx *ctx, const hfx_exact *x);
/* pos_volume_cubpts (n_cubpts,n_eles,n_dims): the physical positions of the cubature points registered with
 * hfx_eles_set_volume_cubpts (which comes first), what the reference recomputes with calc_pos on every call
 * (src/eles.cpp:5095-5097).  Every hfx_eles_set_volume_cubpts drops them: the positions are registered again behind it. */
int hfx_eles_set_error_points(hfx_eles *e, const double *pos_volume_cubpts);
/* eles::compute_error (src/eles.cpp:5076-5136) for one block.  error (2,n_fields) column-major like hf_array is OVERWRITTEN:
 * row 0 the solution error of every field, row 1 the gradient error; norm_type 1: the sum of |e| weight detjac (row 1: |e|
 * summed over the dimensions first, as the reference does), 2: of e^2 weight detjac, anything else is refused with "Error norm
 * not supported!".  The caller adds over blocks and ranks and takes the square root for norm 2 (src/output.cpp:2066-2099).
 *   test case 1: the solution error alone.  Row 1 is zero and grad_disu_upts is never read, so the call works after any fused
 *     stage and with a deferred stage pending (which runs first, fused as it would have).
 *   test case 5: on a viscous context row 1 is the error of grad_disu_upts as it stands against the exact gradient, of which
 *     the reference sets d(rho)/dy, d(rho u)/dy and dE/dy and leaves everything else zero.  A pending deferred stage is run so
 *     that it leaves the gradient; a gradient the last fused stage did not materialise is refused with the words of
 *     hfx_eles_download.  On an inviscid context row 1 is zero.
 *   test cases 2, 3, 4 (advection-diffusion) and unknown ones are refused, as are a missing cubature, missing positions and
 *     missing parameters -- all before anything is launched.
 * One fused kernel and the copy of one partial per workgroup and quantity; no array of the size of n_cubpts x n_eles.  Two
 * calls on one state agree bit for bit (no atomics; fixed summation order for a given grid). */
int hfx_eles_compute_error(hfx_eles *e, int norm_type, double time, double *error);
/* what the next hfx_eles_compute_error launches: workgroups, and the elements a workgroup takes per pass of its loop */
int hfx_eles_error_launch(hfx_eles *e, int *n_groups, int *eles_per_pass);

/* ---- plot-point interpolation (8f-3: the VTU writer's input) -------------- */
/* opp_p (n_ppts,n_upts): the nodal basis at the plot points, eles::set_opp_p (src/eles.cpp:3600-3621) */
int hfx_eles_set_opp_p(hfx_eles *e, int n_ppts, const double *opp_p);
/* eles::calc_disu_ppts (src/eles.cpp:3757-3778) for every element at once instead of per element:
 * disu_ppts (n_ppts,n_eles,n_fields) = opp_p . disu_upts(0), written to the HOST array the plot writer reads
 * (output::write_vtu loops the elements, src/output.cpp) */
int hfx_eles_calc_disu_ppts(hfx_eles *e, double *disu_ppts_host);

/* ---- the plot monitor: the rows of the plot file sampled on the device (src/HiFiLES.cpp:273-285) --------------------------
 * What output::write_tec / write_vtu put into a row behind the position, every run_input.plot_freq steps: the conserved fields at
 * the plot points (eles::calc_disu_ppts), the time averages where the block has average fields (calc_time_average_ppts,
 * hfx_eles_set_average_fields) and run_input.diagnostic_fields (calc_grad_disu_ppts, calc_sensor_ppts and
 * calc_diagnostic_fields_ppts, src/eles.cpp:3781-4006).  One fused launch per block and snapshot interpolates with the registered
 * opp_p (any element class) and evaluates the fields at the plot point; nothing of the size n_ppts x n_eles x n_fields x n_dims
 * exists in memory.  A snapshot pairs disu_upts(0) as it stands with grad_disu_upts as it stands: behind a time step that is the
 * new state and the corrected gradient of the last RK stage's INPUT state, exactly what the reference plots.  The monitor forms no
 * gradient of its own.  The CONSERVATIVE gradient is interpolated and the velocity gradient formed at the plot point, as the
 * reference does.  A NaN is stored as it is (the reference stops on one, src/eles.cpp:3996: the reader looks for it). */
enum hfx_plot_field
{
  HFX_PLOT_U = 0,        /* "u": field 1 / density */
  HFX_PLOT_V = 1,        /* "v" */
  HFX_PLOT_W = 2,        /* "w": 0 on a two-dimensional block */
  HFX_PLOT_ENERGY = 3,   /* "energy": field n_dims + 1 */
  HFX_PLOT_MACH = 4,     /* "mach" */
  HFX_PLOT_PRESSURE = 5, /* "pressure" */
  HFX_PLOT_VORTICITY = 6,          /* "vorticity": its magnitude; |dv/dx - du/dy| in 2-D.  Reads the gradient */
  HFX_PLOT_Q_CRITERION = 7,        /* "q_criterion": (OO - SS) / 2, three-dimensional blocks only.  Reads the gradient */
  HFX_PLOT_SCALED_Q_CRITERION = 8, /* "scaled_q_criterion": (OO - SS) / 2 / (SS + 1e-24).  Reads the gradient */
  HFX_PLOT_SENSOR = 9    /* "sensor": sensor(ele) at every plot point; blocks with shock capturing only */
};
#define HFX_MAX_PLOT_DIAGNOSTICS 16
/* The diagnostic fields of the context in the caller's order, plot_freq >= 1 as run_input.plot_freq, and the snapshots the device
 * history of every block holds (>= 1; 0 drops the monitor).  n_diag = 0 is a monitor of the conserved fields, with the averages where
 * registered.  Any registration empties every block's history.  Refused here, with the reference's words: an unknown code
 * ("plot_quantity not recognized") and a field that reads the gradient on an inviscid context ("Trying to calculate diagnostic field
 * only supported by viscous simualtion").  The context does not know its blocks, so what depends on one is refused where the block is
 * first asked -- by hfx_eles_sample_plot, hfx_eles_calc_plot_fields and by every step loop before its first launch: a Q criterion on a
 * two-dimensional block ("Q criterion Not implemented in 2D"), the sensor on a block without shock capturing ("Sensor unavailable")
 * and blocks of other than n_dims + 2 fields.  Parameters (hfx_ctx_set_params) come first. */
int hfx_ctx_set_plot_monitor(hfx_ctx *ctx, int n_diag, const int *codes, int plot_freq, int capacity);
/* ONE snapshot of the block (which needs hfx_eles_set_opp_p) into the next free slot of its device history; no synchronisation with
 * the host, which notes `time` and `step` for the slot.  Ordinary stores, no atomics: two snapshots of one state are equal bit for bit.
 * With a field that reads the gradient the rule of hfx_eles_compute_wall_forces applies: a pending deferred stage runs so that it
 * leaves grad_disu_upts, and a gradient the last fused stage kept on chip is refused with the words of hfx_eles_download, never read
 * stale.  With gradient-free fields the gradient is never touched: the sample works after any stage and on inviscid contexts.  A
 * full history is refused, nothing is overwritten.
 * Once the clock is the library's (hfx_ctx_set_clock) every step loop does this itself as the last duty of a step, behind averages,
 * probes, the integral and the history monitor (the order of src/HiFiLES.cpp:241-285: a row's averages include the step), for every
 * block with plot points after each step with i_steps % plot_freq == 0.  Such a loop first counts the snapshots it will take and
 * refuses the whole call, before its first launch, when a history cannot hold them.  With a field that reads the gradient the
 * one-stage rule of the integral monitor's ids 1-4 holds: a loop whose stages keep the gradient on chip runs the last RK stage of
 * every step it samples call by call; the partitioned loops refuse that combination before their first launch and name the remedy
 * (fused mode 2).  With gradient-free fields every loop launches exactly the stages it launched before. */
int hfx_eles_sample_plot(hfx_eles *e, double time, int step);
/* the number of stored snapshots (no copy, no synchronisation) | fields per plot point: n_fields + n_average_fields + n_diag */
int hfx_eles_plot_count(hfx_eles *e, int *n_snapshots);
int hfx_eles_plot_width(hfx_eles *e, int *n_out);
/* Synchronises, copies the history -- values (n_ppts, n_eles, n_fields + n_average_fields + n_diag, n_snapshots) with the first index
 * fastest: per snapshot the conserved fields, the averages, the diagnostics, field planes apart as disu_ppts lies; times and steps
 * (n_snapshots) -- and empties it.  max_snapshots: what the caller's arrays hold; fewer than stored is refused, nothing is lost. */
int hfx_eles_read_plot_snapshots(hfx_eles *e, int max_snapshots, double *times, int *steps, double *values, int *n_snapshots);
/* the same kernel on demand: one snapshot (n_ppts, n_eles, n_fields + n_average_fields + n_diag) of the state as it stands into a HOST
 * array; the history is untouched.  Bit for bit what hfx_eles_sample_plot stores for the same state.  Refusals as hfx_eles_sample_plot */
int hfx_eles_calc_plot_fields(hfx_eles *e, double *host);
/* what the next snapshot launches: workgroups, the elements a workgroup takes per pass of its loop, and the plot points of an element
 * its lanes take at a time (an element with more is taken in several passes of the lanes) */
int hfx_eles_plot_launch(hfx_eles *e, int *n_groups, int *eles_per_pass, int *ppts_per_pass);
/* how many of the steps i_steps + 1 .. i_steps + n_steps are multiples of plot_freq: what the loops' capacity check counts */
int hfx_plot_monitor_samples(int i_steps, int n_steps, int plot_freq, int *n_samples);
/* The pointwise formulas of the kernel (csrc/plot_point.hpp) on the HOST, at one plot point: u[n_dims + 2] the interpolated conserved
 * fields, grad (n_dims + 2, n_dims) column-major their interpolated gradient (may be NULL without a gradient field), the element's
 * sensor; out[n_diag] the fields `codes` in their order.  No device is needed: what host-side unit tests call */
int hfx_plot_point_fields(int n_dims, const double *u, const double *grad, double gamma, double sensor, int n_diag, const int *codes,
                          double *out);
/* device milliseconds of one snapshot, averaged over `reps` launches into a scratch snapshot (the history is untouched;
 * grad_disu_upts is read as it stands, whichever stage wrote it) */
int hfx_time_plot_fields(hfx_eles *e, int reps, double *ms);

/* ---- time-averaged fields (run_input.average_fields, src/input.cpp:115-133) -------------------------------------------
 * The running time averages the reference's main loop updates after every time step (run_output.CalcTimeAverageQuantities,
 * src/HiFiLES.cpp:240-245) and every output writer takes to the plot points. */
enum hfx_average_field
{
  HFX_AVG_RHO = 0, /* "rho_average": density */
  HFX_AVG_U = 1,   /* "u_average": field 1 / density */
  HFX_AVG_V = 2,   /* "v_average": field 2 / density */
  HFX_AVG_W = 3,   /* "w_average": field 3 / density (three-dimensional blocks only) */
  HFX_AVG_E = 4    /* "e_average": field n_dims + 1 / density -- field 3 in 2-D, 4 in 3-D (src/eles.cpp:5664-5674) */
};
#define HFX_MAX_AVERAGE_FIELDS 16
/* Registers run_input.average_fields of one block: codes[n] in the order of the input file, names may repeat.  Allocates
 * disu_average_upts (n_upts, n_eles, n) on the device, zeroed as the reference does (src/eles.cpp:124-127).  n = 0 drops the
 * array; registering again replaces it (zeroed).  HFX_AVG_W on a two-dimensional block is refused. */
int hfx_eles_set_average_fields(hfx_eles *e, int n, const int *codes);
/* host <-> device copies of disu_average_upts (n_upts, n_eles, n_average_fields): what a run that is to be continued saves
 * and restores (together with the clock) */
int hfx_eles_upload_average(hfx_eles *e, const double *host);
int hfx_eles_download_average(hfx_eles *e, double *host);
/* eles::CalcTimeAverageQuantities (src/eles.cpp:5630-5702): ONE update of every registered field from disu_upts(0),
 *   average = a * average + b * current,   a = 0, b = 1 when time == spinup_time,
 *   else a = (time - spinup_time - dt) / (time - spinup_time), b = dt / (time - spinup_time)
 * with dt = run_input.dt (dt_type 0 / 1: a and b are evaluated once, on the host) or dt_local(ele) (dt_type 2: per element,
 * in the kernel, from HFX_DT_LOCAL, which must exist).  One streaming kernel; with deferred execution a recorded stage runs
 * first.  The reference's abort on a NaN average (src/eles.cpp:5698) is NOT built: a NaN average means a NaN state, and that
 * is what hfx_eles_check_nan already reports.  The step loops call this themselves once the clock is theirs
 * (hfx_ctx_set_clock). */
int hfx_eles_CalcTimeAverageQuantities(hfx_eles *e, double time, double spinup_time);
/* eles::calc_time_average_ppts (src/eles.cpp:3820-3846) for every element at once: disu_average_ppts
 * (n_ppts, n_eles, n_average_fields) = opp_p . disu_average_upts, with the operator of hfx_eles_set_opp_p and the
 * contraction of hfx_eles_calc_disu_ppts, written to the HOST array the plot writer reads */
int hfx_eles_calc_time_average_ppts(hfx_eles *e, double *disu_average_ppts_host);

/* ---- point probes (run_input.probe, probe_input, output::write_probe; src/HiFiLES.cpp:287-297) --------------------------
 * Time series of the flow at points: a probe is an element and one operator row, opp_probe(i) = eval_nodal_basis(i, loc)
 * (src/eles.cpp:3625-3631); a sample is the state interpolated to the probe and the registered fields formed from it
 * (src/output.cpp:1479-1538).  The history of samples lives on the device; the caller reads it when it wants to write.
 * Values are in the library's non-dimensional units. */
enum hfx_probe_field
{
  HFX_PROBE_RHO = 0, /* "rho": field 0 */
  HFX_PROBE_U = 1,   /* "u": field 1 / rho */
  HFX_PROBE_V = 2,   /* "v": field 2 / rho */
  HFX_PROBE_W = 3,   /* "w": field 3 / rho (three-dimensional blocks only) */
  HFX_PROBE_E = 4,   /* "specific_total_energy": field n_dims + 1 / rho */
  HFX_PROBE_P = 5    /* "pressure": (gamma - 1) (E - 0.5 rho |v|^2), |v|^2 over n_dims components, E = field n_dims + 1 */
};
#define HFX_MAX_PROBE_FIELDS 16
/* The probe fields of the context: codes[n_fields] in the order of the input file (names may repeat), the sampling
 * frequency probe_freq >= 1 (steps) and the number of samples the device history of every block holds.  n_fields = 0 drops
 * everything: no block samples any more and every block's history is emptied (its probes stay registered).  Changing the
 * fields empties the histories of the blocks registered so far. */
int hfx_ctx_set_probes(hfx_ctx *ctx, int n_fields, const int *codes, int probe_freq, int capacity);
/* The probes of one block: ele[n_probes] the element of each probe (0 <= ele < n_eles, checked here), opp_probe
 * (n_upts, n_probes) column-major.  Registering again replaces the probes and empties the history; a failed registration
 * leaves the block as it was; n_probes = 0 removes them (a block of a mixed mesh may have none).  HFX_PROBE_W among the
 * context's fields is refused on a two-dimensional block.  The library sorts the probes by element internally (probes of
 * one element read the same cache lines); every result is in the caller's order.  Removing a probe that two ranks both
 * locate on their common face is the caller's (the reference all-gathers for it). */
int hfx_eles_set_probes(hfx_eles *e, int n_probes, const int *ele, const double *opp_probe);
/* ONE sample: a single launch on the compute stream writes n_fields x n_probes doubles into the next free slot of the
 * device history; the host notes `time` and `step` for that slot (no synchronisation).  With deferred execution a recorded
 * stage runs first.  A full history is refused, nothing is overwritten.  Two samples of one state are equal bit for bit (no
 * atomics, a fixed summation order).  Once the clock is the library's (hfx_ctx_set_clock) every step loop does this itself for
 * every block with probes after each step with i_steps % probe_freq == 0 (src/HiFiLES.cpp:289-297), behind the time
 * averages; such a loop first counts the samples it will take and refuses the whole call, before its first launch, when a
 * block's history cannot hold them.  Without the clock the caller samples. */
int hfx_eles_sample_probes(hfx_eles *e, double time, int step);
/* the number of stored samples (no copy, no synchronisation) and of registered probes; either pointer may be NULL */
int hfx_eles_probe_count(hfx_eles *e, int *n_samples, int *n_probes);
/* Synchronises, copies the history -- values (n_fields, n_probes, n_samples) with the field index fastest, times and steps
 * (n_samples) -- and empties it.  max_samples: what the caller's arrays hold; fewer than stored is refused, nothing is lost. */
int hfx_eles_read_probes(hfx_eles *e, int max_samples, double *times, int *steps, double *values, int *n_samples);
/* device milliseconds of one sampling launch, averaged over `reps` launches into a scratch slot (the history is untouched) */
int hfx_time_probes(hfx_eles *e, int reps, double *ms);

/* ---- mass-flux body force of driven periodic channels (run_input.forcing, src/input.cpp:312) ---------------------------
 * The `forcing == 1` branch of CalcResidual (src/solver.cpp:96-109): at the first RK stage of every time step
 * eles::evaluate_body_force (src/eles.cpp:5281-5482) integrates density and x-momentum over the cyclic inflow plane, turns the
 * mass-flux defect into a streamwise momentum force and an energy force and ADDS them to src_upts (HFX_SRC_UPTS), which every
 * AdvanceSolution scheme subtracts from the residual.  Here the integral, the controller and the addition are three small
 * kernels on the compute stream; on one rank an evaluation makes no copy and no host synchronisation.
 *
 * hfx_eles_set_body_force registers (src/eles.cpp:5312-5373, 5393-5395):
 *   face_ele[n_faces], face_inter[n_faces]   the block's inflow faces as (element, local face) pairs -- the faces the reference
 *       flags at :5312-5338 (cyclic group, x-component of the unit normal at the first cubature point == -1).  n_faces == 0 is
 *       legal: the block (or rank) then only receives the force
 *   n_inters_per_ele, and per local face l: n_cubpts_per_inter[l], opp_inters_cubpts[l] (n_cubpts, n_upts),
 *       weight_inters_cubpts[l] (n_cubpts) -- eles::set_opp_inters_cubpts (src/eles.cpp:3635-3665) and the class's
 *       set_inters_cubpts; entries of local faces no listed face names may be NULL
 *   inter_detjac_inters_cubpts   per listed face, in list order, the n_cubpts values of its local face (packed)
 *       (set_transforms_inters_cubpts, src/eles.cpp:4480-4595)
 *   area, mdot0   the reference hard-codes 9.162 for both (:5393-5395)
 *   history_capacity   evaluations whose (mass_flux, ubulk, body_force(1)) -- the columns of massflux.dat -- are kept
 * The three arrays are folded into one weight per solution point and face, c(k, face) = sum_j w_j detjac(j, face) opp(j, k),
 * so an evaluation costs a dot product of length n_upts per face and field.  Registering again replaces everything and resets
 * the controller: what it had added to src_upts is taken out, and the next evaluation uses mdot_old = mdot0, as a fresh or
 * restarted reference run does (:5398-5403).  Refused: two-dimensional blocks and n_fields != 5 (the reference runs the branch
 * for n_dims == 3, equation == 0 only), a face outside the block. */
int hfx_eles_set_body_force(hfx_eles *e, int n_faces, const int *face_ele, const int *face_inter, int n_inters_per_ele,
                            const int *n_cubpts_per_inter, const double *const *opp_inters_cubpts,
                            const double *const *weight_inters_cubpts, const double *inter_detjac_inters_cubpts, double area,
                            double mdot0, int history_capacity);
/* drops the registration and takes its contribution out of src_upts; no-op without one */
int hfx_eles_clear_body_force(hfx_eles *e);
/* eles::evaluate_body_force (src/eles.cpp:5281-5482), ONE evaluation on this rank's faces alone, for callers that drive the stages
 * themselves (at the first RK stage, before it: nothing between the top of the stage and src/solver.cpp:96 changes
 * disu_upts(0) or src_upts).  integral(0), integral(1) over the registered faces (fields 2 and 3, which the reference integrates
 * and never reads, are not) in a fixed summation order -- the same state gives the same bits --, then :5411-5428 with dt =
 * hfx_params.dt:  ubulk = integral(0) == 0 ? 0 : integral(1) / integral(0);  mass_flux = ubulk * integral(0);
 * body_force(1) = 1 / area / dt * (mdot0 - 2 mass_flux + mdot_old);  body_force(4) = body_force(1) * ubulk;  mdot_old = mdot0
 * at the first evaluation after a registration, the previous mass_flux afterwards; then src_upts(., ., k) += body_force(k),
 * k = 1, 4.  HFX_SRC_UPTS is allocated (zeroed) by the first evaluation when the caller uploaded none; an uploaded source
 * term keeps its values and the force adds on top (upload it BEFORE the registration: an upload of HFX_SRC_UPTS replaces the
 * whole array, the controller's contribution included).  dt_type 2 is refused with the reference's message (:5409).
 * Immediate: with deferred execution the recorded stage runs first.  hfx_run_steps, hfx_run_steps_blocks,
 * hfx_run_steps_partitioned and hfx_run_steps_partitioned_blocks evaluate every registered block themselves, behind their
 * calc_time_step and before the first stage of every step; the partitioned ones sum the two integrals over the communicator
 * (the MPI_Allreduce of :5375-5385; one host round trip per step).  The hfx_time_* entry points never evaluate it. */
int hfx_eles_evaluate_body_force(hfx_eles *e);
/* The two halves of an evaluation for a caller whose transport sums over the ranks (the MPI_Allreduce of src/eles.cpp:5375-5385):
 * hfx_eles_body_force_integrals returns THIS rank's integral(0), integral(1) (zeros for a rank without inflow faces; waits for
 * the compute stream), the caller adds them over the ranks, hfx_eles_body_force_apply runs the controller and the addition to
 * src_upts from the sums.  Immediate, like hfx_eles_evaluate_body_force, which is the two in one without leaving the device. */
int hfx_eles_body_force_integrals(hfx_eles *e, double integral[2]);
int hfx_eles_body_force_apply(hfx_eles *e, const double integral[2]);
/* The controller's record after the last evaluation (waits for the compute stream): mass_flux, ubulk, body_force(1),
 * accumulated[2] = the sums of body_force(1) and body_force(4) since the registration (what src_upts holds of the controller),
 * integral[2] = integral(0), integral(1) (over all ranks), n_steps = evaluations since the registration.  Any pointer may be
 * NULL.  Fails with the reference's "ERROR: NaN body force, exiting" (src/eles.cpp:5455-5458) once a body_force(1) was NaN. */
int hfx_eles_body_force_state(hfx_eles *e, double *mass_flux, double *ubulk, double *body_force_x, double accumulated[2],
                              double integral[2], long *n_steps);
/* the newest min(max_rows, history_capacity, n_steps) rows (mass_flux, ubulk, body_force(1)) -- what the reference appends to
 * massflux.dat (src/eles.cpp:5445-5451) --, oldest first: rows (3, *n_rows).  max_rows == 0 asks for the number alone */
int hfx_eles_body_force_history(hfx_eles *e, int max_rows, double *rows, int *n_rows);

/* ---- wall forces: output::CalcForces (src/output.cpp:1915-2014), eles::compute_wall_forces (src/eles.cpp:5704-5990) ----
 * The force on the walls of a block -- Fx, Fy(, Fz), CL, CD of history.plt (src/output.cpp:2381-2393) -- and Cp and Cf at every
 * wall cubature point (force_files_<step>/cp_<step>_p<rank>.dat), in one fused kernel per call.
 *
 * The reference state, non-dimensional as run_input holds it (src/input.cpp:534-612).  The library forms from it, as
 * src/eles.cpp:5733-5743 do, factor = 1 / (0.5 rho_c_ic (u_c_ic^2 + v_c_ic^2 + w_c_ic^2)), aoa = atan2(v_c_ic, u_c_ic),
 * aos = atan2(w_c_ic, u_c_ic).  Refused when the speed is zero or area_ref <= 0 (the reference would divide by zero). */
typedef struct hfx_force_ref
{
  double rho_c_ic, u_c_ic, v_c_ic, w_c_ic, p_c_ic, area_ref;
} hfx_force_ref;
int hfx_ctx_set_force_reference(hfx_ctx *ctx, const hfx_force_ref *ref);
/* The wall faces of one block, as (element, local face, bc flag) triples in the order the caller wants its results in:
 *   face_ele[n_faces], face_inter[n_faces], face_flag[n_faces]   face_flag is HFX_BC_SLIP_WALL, HFX_BC_ISOTHERM_WALL,
 *       HFX_BC_ADIABAT_WALL or HFX_BC_SLIP_WALL_DUAL (the four kinds src/eles.cpp:5768-5769 take).  n_faces == 0 is legal
 *   n_inters_per_ele, and per local face l: n_cubpts_per_inter[l], opp_inters_cubpts[l] (n_cubpts, n_upts) column-major,
 *       weight_inters_cubpts[l] (n_cubpts), as for hfx_eles_set_body_force; entries of local faces no listed face names may be NULL
 *   inter_detjac_inters_cubpts   per listed face, in list order, the n_cubpts values of its local face (packed)
 *   norm_inters_cubpts           per listed face, in list order, (n_cubpts, n_dims) column-major (packed): the unit normals
 * A face is one whose bcid names a group of one of the four kinds; the reference's loop also takes local faces of boundary
 * elements that belong to NO group (bcid == -1, an out-of-bounds read of bc_list): those are not wall faces and are not to be
 * listed.  The library sorts the faces by (local face, element) internally; every result is in the caller's order.
 * Registering again replaces everything.  Refused, before anything changes: a face outside the block, an unknown flag, a local
 * face without its operator, more than 256 cubature points on a face.  Should a device allocation fail after that, the block is
 * left without wall faces. */
int hfx_eles_set_wall_faces(hfx_eles *e, int n_faces, const int *face_ele, const int *face_inter, const int *face_flag,
                            int n_inters_per_ele, const int *n_cubpts_per_inter, const double *const *opp_inters_cubpts,
                            const double *const *weight_inters_cubpts, const double *inter_detjac_inters_cubpts,
                            const double *norm_inters_cubpts);
/* drops the registration; no-op without one */
int hfx_eles_clear_wall_faces(hfx_eles *e);
/* eles::compute_wall_forces for one block: inv_force[n_dims], vis_force[n_dims], *cl, *cd are this block's sums (the caller adds
 * blocks and ranks, src/output.cpp:1980-2009); cp and cf, either of which may be NULL, take one value per (listed face, cubature
 * point) in the caller's list order, faces packed as inter_detjac_inters_cubpts is; inside a face the index is the reference's j
 * (the reference PRINTS j descending).  Per point (src/eles.cpp:5773-5986): the state -- and on a viscous context the gradient --
 * interpolated by opp_inters_cubpts(l); the pressure, for HFX_BC_SLIP_WALL_DUAL from the momenta with their normal part removed
 * (which the viscous part then uses too); Cp = (p - p_c_ic) factor; Finv = wgt (p - p_c_ic) n detjac factor / area_ref; on a
 * viscous context, for walls of ALL four kinds, mu from Sutherland's law blended by fix_vis, S with its trace / 3.0 removed (in
 * two dimensions too), taun = 2 mu S n, Cf = |taun - (taun . n) n| factor, Fvis = -wgt taun detjac factor / area_ref; cl and cd by the
 * reference's formulas, in three dimensions cd = F0 cos(aoa) cos(aos) + F1 sin(aoa) + F2 sin(aoa) cos(aos).  On an inviscid
 * context vis_force and cf are zero and grad_disu_upts is never touched.
 * The gradient: a viscous context reads grad_disu_upts AS IT STANDS, like the reference, which pairs the new state with the
 * gradient of the last RK stage.  With deferred execution a pending stage is replayed call by call so that it leaves that
 * gradient.  After a fused stage that kept the gradient on chip (hfx_run_steps(..., 3), hfx_run_steps_blocks(..., 4)) the call is
 * refused, as hfx_eles_download is: run hfx_CalcResidual first -- its correct_gradient writes the gradient of the CURRENT state --
 * and the forces are then those of the current state and its own gradient.
 * Reproducible: shuffles inside a wave, the waves in their order, one partial per workgroup, added by the host in workgroup
 * order; no floating-point atomics, two calls on one state agree bit for bit.  Every refusal -- no registration, no force
 * reference, a block that is not n_dims + 2 fields in two or three dimensions, a stale gradient -- comes before anything is
 * launched; a block with zero wall faces returns zeros and launches nothing.  Waits for the compute stream. */
int hfx_eles_compute_wall_forces(hfx_eles *e, double *inv_force, double *vis_force, double *cl, double *cd, double *cp, double *cf);
/* what the next hfx_eles_compute_wall_forces launches: workgroups, and the consecutive faces a workgroup takes per pass */
int hfx_eles_wall_force_launch(hfx_eles *e, int *n_groups, int *faces_per_pass);
/* device milliseconds of the kernel of one hfx_eles_compute_wall_forces, averaged over `reps` launches */
int hfx_time_wall_forces(hfx_eles *e, int reps, double *ms);

/* ---- CFL time stepping (calc_time_step, src/solver.cpp:484-549) ---------- */
int hfx_eles_set_h_ref(hfx_eles *e, const double *h_ref); /* eles::h_ref (n_eles), src/eles.cpp:3985 */
/* dt_local(ic) = eles::calc_dt_local(ic) (src/eles.cpp:1267-1356) for every element -> HFX_DT_LOCAL, and the
 * block's minimum.  dt_type 1: the caller takes the minimum over blocks and ranks (all-reduce MIN) and sets
 * hfx_params.dt; dt_type 2: AdvanceSolution reads HFX_DT_LOCAL. */
int hfx_eles_calc_dt_local(hfx_eles *e, double CFL, double *dt_min);

/* ---- over-integration (row a5) ------------------------------------------- */
/* Registers what eles_hexas::set_over_int (src/eles_hexas.cpp:1096-1129) and set_transforms build when
 * run_input.over_int == 1: opp_over_int_cubpts (n_cubpts,n_upts), over_int_filter (n_upts,n_cubpts),
 * JGinv_over_int_cubpts (n_dims,n_dims,n_cubpts,n_eles).  Once set, hfx_CalcResidual evaluates the inviscid
 * flux through evaluate_invFlux_over_int as the reference does (src/solver.cpp:82-91). */
int hfx_eles_set_over_int(hfx_eles *e, int n_cubpts, const double *opp_over_int_cubpts, const double *over_int_filter,
                          const double *JGinv_over_int_cubpts);
int hfx_eles_evaluate_invFlux_over_int(hfx_eles *e); /* eles::evaluate_invFlux_over_int, src/eles.cpp:1480-1545 */

/* ---- shock capturing (row a16) ------------------------------------------ */
/* Registers what eles_hexas / eles_quads build when run_input.shock_cap == 1 (src/eles_hexas.cpp:74-85):
 * inv_vandermonde (n_upts,n_upts), exp_filter (n_upts,n_upts), norm_basis_persson (n_upts), and
 * high_modes(j) = 1 where a 1-D index of Legendre mode j equals the order (the set summed in
 * shock_det_persson, src/eles_hexas.cpp:1042-1047); s0 and shock_det_field are run_input's.
 * A block of TRIANGLES registers what eles_tris builds (src/eles_tris.cpp:432-469): inv_vandermonde of the orthonormal Dubiner
 * basis at the solution points (modes by total degree k, within k by j = 0..k), exp_filter = V sigma V^-1, norm_basis_persson all
 * ones and high_modes(j) = 1 exactly for j >= p (p + 1) / 2, the modes of total degree p (eles_tris::shock_det_persson,
 * src/eles_tris.cpp:472-524).  The 2-D simplex fused stage folds exactly this form into its update kernel
 * (hfx_simplex2d_shock_plan); the per-method call below takes any registration. */
int hfx_eles_set_shock_capture(hfx_eles *e, const double *inv_vandermonde, const double *exp_filter,
                               const double *norm_basis_persson, const int *high_modes, double s0, int shock_det_field);
/* eles::shock_capture (src/eles.cpp:2918-2959), shock_det 0 (Persson) + shock_cap 1 (exponential modal
 * filter): sensor(ele) -> HFX_SENSOR; disu_upts(0) of every element with sensor >= s0 is filtered.
 * Called by the caller after AdvanceSolution (src/HiFiLES.cpp:214-216); invalidates disu_fpts. */
int hfx_eles_shock_capture(hfx_eles *e);

/* ---- boundary faces (reference class bdy_inters) ------------------------ */
/* bc_flag values of the reference (src/bc.cpp:36-48) */
enum hfx_bc_flag
{
  HFX_BC_SUB_IN_SIMP = 0, HFX_BC_SUB_OUT_SIMP = 1, HFX_BC_SUB_IN_CHAR = 2, HFX_BC_SUB_OUT_CHAR = 3, HFX_BC_SUP_IN = 4,
  HFX_BC_SUP_OUT = 5, HFX_BC_SLIP_WALL = 6, HFX_BC_CYCLIC = 7, HFX_BC_ISOTHERM_WALL = 8, HFX_BC_ADIABAT_WALL = 9,
  HFX_BC_CHAR = 10, HFX_BC_SLIP_WALL_DUAL = 11
};
/* one entry of run_input.bc_list (include/bc.h:48-62), values AFTER input::read_boundary_param's
 * non-dimensionalisation (src/input.cpp:440-525); fields a type does not use are ignored */
typedef struct hfx_bc
{
  int flag, pressure_ramp, use_wm, pad;
  double rho, velocity[3], p_static, T_static, p_total, T_total, nx, ny, nz;
  double p_ramp_coeff, T_ramp_coeff, p_total_old, T_total_old;
} hfx_bc;
/* L(j,i): offset of the face's flux point in the left block's (fpt,ele) plane (what bdy_inters::set_boundary,
 * src/bdy_inters.cpp:75-135, stores as pointers); boundary_id(i): index into bcs (bdy_inters::boundary_id);
 * R_ref: run_input.R_ref for viscous runs, run_input.R_gas for inviscid ones (src/bdy_inters.cpp:368-369).
 * An isotherm_wall / adiabat_wall group with use_wm takes the wall model of the context (hfx_ctx_set_wall_model, which
 * comes first); under a context without one such a group is refused, as is the LES inlet. */
int hfx_bdy_inters_create(hfx_ctx *ctx, hfx_eles *left, int n_inters, int n_fpts_per_inter, const int *L,
                          const int *boundary_id, const hfx_bc *bcs, int n_bcs, double R_ref, hfx_inters **out);
/* The wall model of the reference (run_input.wall_model, src/wall_model_funcs.cpp): 0 off, 1 Werner-Wengle, 2 the
 * compressible wall function of Breuer-Rodi; anything else: "Wall model not implemented!".  prandtl_t: run_input.prandtl_t
 * (default 0.9); Kappa: the reference's constant 0.41 (src/input.cpp:666).  At a face of a use_wm group the ghost states are
 * the slip mirror (inviscid Riemann problem) and the wall-parallel velocity (LDG common solution), and the viscous sweep adds
 * (0, tau_w, -q_w + v_w . tau_w) tdA from calc_wall_stress in place of the LDG flux (src/bdy_inters.cpp:1095-1132).  The
 * Newton loop of model 2 ends after 64 iterations with a NaN flux, where the reference's would not end. */
int hfx_ctx_set_wall_model(hfx_ctx *ctx, int wall_model, double prandtl_t, double Kappa);
/* The model's input point of every face (n_inters entries each): upt[i] a solution point of the face's own (left) element,
 * whose disu_upts(0) of the current stage the model reads for ALL flux points of face i, and dist[i] its distance from the
 * wall (eles::calc_wm_upts_dist, src/eles.cpp:4873-4903: the first solution point with the strictly largest minimum over the
 * face's flux points of (pos_fpt - pos_upt) . n_fpt).  Entries of faces without a model are ignored; upt is range-checked.
 * A viscous sweep or step loop over a block with wall-model faces and no registered points is refused before any launch. */
int hfx_bdy_inters_set_wall_model_points(hfx_inters *f, const int *upt, const double *dist);
int hfx_bdy_inters_wall_model_faces(hfx_inters *f, int *n); /* the wall-model faces of the block */
int hfx_bdy_inters_set_ramp_counter(hfx_inters *f, int ramp_counter); /* run_input.ramp_counter (pressure ramps) */
int hfx_bdy_inters_evaluate_boundaryConditions_invFlux(hfx_inters *f, double time_bound);  /* src/bdy_inters.cpp:213 */
int hfx_bdy_inters_evaluate_boundaryConditions_viscFlux(hfx_inters *f, double time_bound); /* src/bdy_inters.cpp:1024 */

/* ---- the caller contract ---------------------------------------------- */
/* CalcResidual (src/solver.cpp:50-223) for one element block and its interior and boundary
 * face blocks (any mix, in `faces`), RANS off; same call order as the reference.  The `forcing == 1` branch
 * (src/solver.cpp:96-109) is not in here: a caller that drives the stages itself calls hfx_eles_evaluate_body_force at the
 * first RK stage of a step, the hfx_run_steps* loops do so themselves (see "mass-flux body force" above). */
int hfx_CalcResidual(hfx_eles *e, hfx_inters *const *faces, int n_face_blocks);
/* The same for a MIXED mesh: several element blocks (the reference's mesh_eles(i), one per element class) and face blocks
 * whose left and right sides may belong to different element blocks (int_inters::set_interior is called with
 * ctype(ic_l), ctype(ic_r), src/geometry.cpp:637-706).  Every method runs for all element blocks before the next one,
 * exactly as src/solver.cpp:59-221 loops `for (i = 0; i < n_ele_types; i++) mesh_eles(i)->method()`. */
int hfx_CalcResidual_blocks(hfx_eles *const *eles, int n_ele_blocks, hfx_inters *const *faces, int n_face_blocks);
/* n_steps time steps = the RK-stage loop of src/HiFiLES.cpp:194-217:
 * for each stage CalcResidual + AdvanceSolution.  `fused`: 0 the per-method path, 2 the split fused
 * kernels, 3 the split kernels with the fluxes evaluated in the gradient kernel (same results to
 * rounding).  All leave disu_upts(0), disu_upts(1), disu_fpts of the new state and, for the step's last
 * stage, div_tconf_upts in the public arrays; mode 2 also leaves grad_disu_upts / grad_disu_fpts of the
 * last stage, mode 3 keeps them in registers and folds opp_3 . norm_tdisf_fpts into the divergence it stores, so
 * norm_tdisf_fpts is not refreshed either; nor is delta_disu_fpts at interior points, whose LDG corrections the flux kernel
 * forms itself from the partner's flux-point solution (run one per-method stage when a monitor needs them).
 * With dt_type 1 / 2 every step starts with calc_time_step (hfx_ctx_set_CFL, hfx_eles_set_h_ref); boundary
 * blocks whose groups ramp get run_input.ramp_counter advanced after every step (src/HiFiLES.cpp:224-225). */
int hfx_run_steps(hfx_eles *e, hfx_inters *const *faces, int n_face_blocks, int n_steps, int fused);
/* The RK loop over several element blocks (mixed meshes).  fused 0: the per-method path; fused 4: the fused stage for
 * general (non-tensor-product) element classes, three-dimensional Navier-Stokes / Euler blocks with interior and
 * boundary faces (csrc/general.hip): three or four launches per element block and stage, the dense operator contractions on the
 * FP64 matrix cores over batches of 16 elements; like fused 3 it keeps the corrected gradients on chip (only boundary
 * points get grad_disu_fpts) and leaves disu_upts(0), disu_upts(1), disu_fpts of the new state and div_tconf_upts;
 * norm_tdisf_fpts (folded into the divergence operator) and delta_disu_fpts of pairs inside a block are not refreshed.
 * What the blocks registered takes part: an LES closure is evaluated inside the flux kernel (tetrahedra / prisms of orders 1..3;
 * calc_sgs_terms before the first stage of a step), over-integration forms tdisf_upts by the dense contractions and the flux kernel
 * takes it, shock capturing follows every stage (the filter, then disu_fpts of the filtered state); a closure TOGETHER with
 * over-integration is refused (run fused 0).
 * ONE block of triangles (orders 1-5) runs the 2-D simplex fused stage (csrc/simplex2d.hip), at most
 * four launches per stage.  A registered LES closure is evaluated INSIDE its element kernel (hfx_simplex2d_les_plan; not beside
 * over-integration, and only with the block's own Jacobian_fpts).  Registered over-integration (a triangle rule of over_int_order 0..7: 1..36 cubature points) runs INSIDE
 * its element kernel, which walks the cubature points in chunks and keeps the de-aliased flux in registers (option "fold_over_int"
 * 0: hfx_eles_evaluate_invFlux_over_int in front of the element kernel, which then reads tdisf_upts; hfx_simplex2d_over_int_plan).  Shock capturing registered in the form of eles_tris::shock_det_persson (below) runs INSIDE its update
 * kernel: sensor, filter and the flux-point solution of the filtered state in the stage's last launch (option "fold_shock" 0: the
 * per-method filter behind the stage, as on tetrahedra); any other registration is refused before the first launch (run fused 0).
 * A block with one element class may of course be passed alone (hfx_run_steps(e, ..., 4) is the same call). */
int hfx_run_steps_blocks(hfx_eles *const *eles, int n_ele_blocks, hfx_inters *const *faces, int n_face_blocks, int n_steps,
                         int fused);

/* One RK stage of the split fused path on a PARTITIONED block, cut so that the caller can move the
 * partition-face buffers while interior faces are being worked on (the order of CalcResidual's
 * send / receive calls, src/solver.cpp:70-72,134-138,150-154,200-209):
 *   phase 0: (first stage only) extrapolate, pack out_buffer_disu          -> caller STARTS solution exchange
 *   phase 1: LDG common solution on interior faces                         -> caller WAITS for the solution
 *   phase 2: the same on partition faces, corrected gradients, pack out_buffer_grad_disu
 *                                                                          -> caller STARTS gradient exchange
 *   phase 3: common fluxes on interior faces, inviscid part on partition faces
 *                                                                          -> caller WAITS for the gradient
 *   phase 4: viscous common flux on partition faces, residual, RK update (in_step), the new state's
 *            flux-point solution packed into out_buffer_disu               -> caller STARTS solution exchange
 * Inviscid runs have nothing to send after phase 2.  `first` != 0 on the first stage after the caller
 * changed disu_upts(0).  With the context's fused mode 2 the kernels are those of hfx_run_steps(fused=2)
 * and the second exchange carries the corrected gradient (buffers 2/3, as the reference does); otherwise
 * (default) those of fused=3, and the second exchange carries each side's viscous flux projected on
 * its own normal (buffers 4/5: n_fields instead of n_fields*n_dims doubles per flux point) and the
 * partition faces' common flux is evaluated in phase 4. */
int hfx_stage_partitioned(hfx_eles *e, hfx_inters *const *int_faces, int n_int, hfx_inters *const *mpi_faces,
                          int n_mpi, int phase, int in_step, int first);

/* ---- partition-face transport inside the library: RCCL point-to-point over xGMI ------------------------
 * Replaces the MPI_Isend / MPI_Irecv / MPI_Waitall of mpi_inters::send_* / receive_* (src/mpi_inters.cpp:244-270,
 * 304-332) by grouped ncclSend / ncclRecv on a communication stream the library owns, ordered against the
 * context's compute stream with events -- no host synchronisation inside a stage.  librccl is resolved at run time
 * (dlopen "librccl.so.1"; the copy already mapped into the process is reused), so callers that never create a
 * communicator do not need it.  Launch contract: one process per GPU; rank 0 calls hfx_comm_get_unique_id and the
 * launcher distributes the 128 bytes (MPI_Bcast in the reference's world, a file / store / gloo broadcast under
 * Python); then every rank calls hfx_comm_create collectively. */
typedef struct hfx_comm hfx_comm;
#define HFX_COMM_ID_BYTES 128
int hfx_comm_get_unique_id(char id[HFX_COMM_ID_BYTES]);
int hfx_comm_create(hfx_ctx *ctx, const char id[HFX_COMM_ID_BYTES], int nranks, int rank, hfx_comm **out);
int hfx_comm_destroy(hfx_comm *c);
/* Exchange accounting of this communicator since its creation: posted[k] / waited[k] = messages of kind k (0 the flux-point
 * solution, 1 the corrected gradient or projected viscous flux, 2 the SGS flux) posted / waited for, counted per partition-face
 * block (a fused stage's grouped exchange over n blocks counts n, as n send_* calls would); *in_flight = solution messages
 * posted and not yet consumed by a stage (a partitioned fused stage leaves the next state's one so); *stream_busy = 1 while the
 * communication stream has work queued (hipStreamQuery).  posted[0] - *in_flight equals what the same partition-face calls post
 * with the option "deferred" off, whatever the rank downloaded or flushed in between.  Any argument may be NULL. */
int hfx_comm_exchange_stats(hfx_comm *c, long posted[3], long waited[3], int *in_flight, int *stream_busy);
/* what RCCL reports for this communicator: ncclCommCount, ncclCommUserRank, ncclCommCuDevice, and that device's PCI bus id
 * (hipDeviceGetPCIBusId) -- evidence in a benchmark line that N ranks on N different devices took part */
int hfx_comm_info(hfx_comm *c, int *nranks, int *rank, int *device, char pci_bus_id[32]);
/* MPI_Allreduce(MIN / MAX / SUM) of a few doubles (calc_time_step's dt, src/solver.cpp:511,543; the monitors'
 * reductions); op 0 min, 1 max, 2 sum.  Synchronises the host with the communication stream. */
int hfx_comm_allreduce(hfx_comm *c, double *values, int n, int op);
/* Neighbour table of a partition-face block = mpi_inters::Nout_proc generalised to segments: the faces
 * [send_first[s], send_first[s]+count[s]) of out_buffer_* go to rank peer[s], and what peer[s] sends in return lands
 * in the faces [recv_first[s], recv_first[s]+count[s]) of in_buffer_*.  The reference's layout (faces of one rank
 * contiguous, ordered by rank, src/mpi_inters.cpp:244-256) is send_first == recv_first == running sum of Nout_proc.
 * peer[s] == own rank is allowed (a periodic direction that is not split). */
int hfx_mpi_inters_set_neighbours(hfx_inters *f, int n_seg, const int *peer, const int *send_first, const int *recv_first,
                                  const int *count);
/* mpi_inters::send_solution / receive_solution / send_corrected_gradient / receive_corrected_gradient
 * (src/mpi_inters.cpp:218-336): send_* packs on the compute stream and starts the grouped exchange on the
 * communication stream; receive_* makes the compute stream wait for it (the MPI_Waitall). */
int hfx_mpi_inters_send_solution(hfx_inters *f, hfx_comm *c);
int hfx_mpi_inters_receive_solution(hfx_inters *f, hfx_comm *c);
int hfx_mpi_inters_send_corrected_gradient(hfx_inters *f, hfx_comm *c);
int hfx_mpi_inters_receive_corrected_gradient(hfx_inters *f, hfx_comm *c);
/* LES: mpi_inters::send_sgsf_fpts / receive_sgsf_fpts (src/mpi_inters.cpp:339-397), called by CalcResidual after
 * extrapolate_sgsFlux and before the partition faces' viscous flux (src/solver.cpp:168-178,203-206) */
int hfx_mpi_inters_send_sgsf_fpts(hfx_inters *f, hfx_comm *c);
int hfx_mpi_inters_receive_sgsf_fpts(hfx_inters *f, hfx_comm *c);
/* n_steps time steps of the split fused path on a partitioned block: the five phases of hfx_stage_partitioned with
 * the two exchanges of every stage started and awaited from inside the library in CalcResidual's order
 * (src/solver.cpp:68-72,131-139,148-155,197-210): solution exchange in flight during the interior LDG sweep, flux /
 * gradient exchange in flight during the interior common-flux sweep.  With dt_type 1 / 2 the step starts with
 * calc_time_step (src/HiFiLES.cpp:198): per-element CFL steps, block minimum, all-reduce MIN over the ranks.
 * h_ref (hfx_eles_set_h_ref) and run_input.CFL (hfx_ctx_set_CFL) must have been set then.  Boundary blocks in
 * int_faces get run_input.ramp_counter advanced after every step when one of their groups ramps
 * (src/HiFiLES.cpp:224-225). */
int hfx_run_steps_partitioned(hfx_eles *e, hfx_inters *const *int_faces, int n_int, hfx_inters *const *mpi_faces, int n_mpi,
                              hfx_comm *comm, int n_steps);
/* The same for a mesh of SEVERAL element blocks and / or non-tensor classes (tetrahedra, prisms, mixed meshes): the general fused
 * stage (hfx_run_steps_blocks(..., 4)) on partitioned blocks.  A partition-face block belongs to one element block
 * (mpi_inters::set_mpi takes any in_ele_type_l, src/mpi_inters.cpp:154); int_faces holds the interior blocks (whose two sides may
 * lie in different element blocks) and the boundary blocks.  Each stage: LDG corrections and common fluxes of the partition faces
 * by the one-sided kernels, the flux-point solution and each side's projected viscous flux Fn as the two messages.  With dt_type
 * 1 / 2 every step starts with calc_time_step (src/solver.cpp:484-549, src/HiFiLES.cpp:198): hfx_eles_calc_dt_local of every
 * block, the minimum over the blocks, all-reduce MIN over the ranks (h_ref and run_input.CFL must have been set).
 * Three-dimensional blocks as hfx_run_steps_blocks(..., 4) takes them -- an LES closure is evaluated in the
 * flux kernel (its F_sgs . n travels inside Fn: no third message; the SVV closure is refused here), over-integration feeds it,
 * shock capturing follows the update before the next solution message is packed.
 * ONE block of triangles (orders 1-5; no LES closure; over-integration inside the element kernel on either group list, or with
 * "fold_over_int" 0 per method on the compute stream in front of the interior groups' element launch; shock capturing in the triangle's own form is folded into the
 * update kernel, so the partition groups' filtered flux-point solution is what is packed) runs the 2-D simplex fused stage, interior
 * groups first: the element and the update kernel walk the groups without a partition flux point beside the solution message, the
 * groups with one behind it (hfx_simplex2d_partition_plan); with one partition-face block the element kernel reads the partners
 * of partition points from the receive record itself.  hfx_run_steps_blocks(..., 4) keeps refusing a partition-face block.
 * With deferred execution the mirrored CalcResidual of such a mesh runs this stage when its send_* / receive_* name one hfx_comm. */
int hfx_run_steps_partitioned_blocks(hfx_eles *const *eles, int n_ele_blocks, hfx_inters *const *int_faces, int n_int,
                                     hfx_inters *const *mpi_faces, int n_mpi, hfx_comm *comm, int n_steps);
/* Average durations (ms, HIP events) over `reps` stages of the same loop: ms[0..3] phases 1-4 on the compute stream,
 * ms[4] solution exchange and ms[5] flux / gradient exchange on the communication stream (from the moment their
 * data is packed to the last byte received), ms[6] the whole stage, ms[7] the element kernel of phase 2 alone (the split flux
 * kernel; 0 for inviscid runs and fused mode 2).  This is the SERIALISED schedule: every kernel on the compute stream so that
 * the events bracket the phases -- hfx_run_steps_partitioned itself puts the one-sided partition-face kernels on the
 * communication stream (option "comm_stream_faces") and is timed as a whole by the caller.  The state advances by reps stages. */
int hfx_time_partitioned(hfx_eles *e, hfx_inters *const *int_faces, int n_int, hfx_inters *const *mpi_faces, int n_mpi,
                         hfx_comm *comm, int reps, double ms[8]);

/* ---- measurement ------------------------------------------------------- */
/* Average duration (ms, HIP events on the context's stream) of every per-method entry
 * point over `reps` repetitions of one RK stage, in CalcResidual order:
 *  0 extrapolate_solution  1 calculate_gradient  2 evaluate_invFlux  3 common_invFlux (all face blocks)
 *  4 correct_gradient      5 evaluate_viscFlux   6 extrapolate_totalFlux  7 calculate_divergence
 *  8 common_viscFlux       9 calculate_corrected_divergence  10 AdvanceSolution
 * The state advances by reps stages (stage index cycles through the scheme). */
#define HFX_N_TIMED_METHODS 11
int hfx_time_methods(hfx_eles *e, hfx_inters *const *faces, int n_face_blocks, int reps, double ms[HFX_N_TIMED_METHODS]);
/* The three kernels of one evaluation of the body force (hfx_eles_evaluate_body_force), each between two HIP events:
 * ms[0] mass_flux_kernel, ms[1] body_force_kernel, ms[2] add_body_force_kernel, averaged over `reps` evaluations -- which do
 * take place: the controller and src_upts advance by reps evaluations. */
int hfx_time_body_force_kernels(hfx_eles *e, int reps, double ms[3]);
/* The same for the kernels of the fused path: ms[8] (unused entries 0), names = comma-separated
 * kernel names (buffer of 256 chars); the state advances by reps stages. */
int hfx_time_fused_kernels(hfx_eles *e, hfx_inters *const *faces, int n_face_blocks, int reps, double ms[8], char names[256]);
/* ALGORITHMIC HBM bytes per launch of each fused kernel (same order), see DESIGN.md.  Variant 3, once the block's fused tables are
 * built: bytes[5] is the number of flux points whose projected viscous flux Fn the stage needs (one-sided LDG, |ldg_beta| = 1/2, hexahedra: one
 * point of every interior pair and every boundary / partition-face point; otherwise every point), bytes[6] the bytes per stage that
 * the flux kernel does not write and the face kernel does not read for the others (bytes[1] and bytes[2] count every point: the two
 * kernels together move bytes[6] less).  bytes[7]: with folded faces (option "fold_faces"), the bytes per stage that the stage no longer
 * moves because the flux kernel forms the interior pairs' common flux and face_flux2_kernel is not launched (0 otherwise); bytes[1]
 * and bytes[2] do not change with it. */
int hfx_fused_kernel_bytes(hfx_eles *e, double bytes[8]);
/* The launches of the persistent element kernels since the block's last split fused stage began, in launch order: slot[i] is the
 * kernel's entry in hfx_time_fused_kernels (1 flux / gradient kernel, 3 update / residual kernel, 4 over-integration kernel) or 5 for the
 * shock-capturing kernel, grid[i] its workgroups, work[i] the elements -- on a partitioned block the entries of the element list -- it walks.
 * Writes min(*n_launches, max_launches) entries; at most 16 launches are kept. */
int hfx_fused_launch_grids(hfx_eles *e, int max_launches, int *slot, int *grid, long *work, int *n_launches);
/* The two-wave form of the affine flux kernel (P4 hexahedra on an affine block, option "flux_two_wave"): 22 of an element's 150 flux
 * points have no partner lane and run as an extra pass, which is skipped when none of them needs its projected viscous flux
 * (one-sided LDG).  The library puts them on the local face whose flux the block needs least often: *face is that face (0..5; -1:
 * the form does not run on this block; the forced face with option "flux_two_wave_face"), need[f] the number of elements that would take the pass with the points on face f (counted
 * from the partner words and ldg_beta). */
int hfx_flux_two_wave_face(hfx_eles *e, hfx_inters *const *faces, int n_face_blocks, int *face, long need[6]);
/* The same for the general fused stage (hfx_run_steps_blocks(..., fused = 4)): ms[0..3] = pairwise LDG kernels, flux
 * kernels of all element blocks, pairwise common-flux kernels, update kernels of all blocks */
int hfx_time_general_kernels(hfx_eles *const *eles, int n_ele_blocks, hfx_inters *const *faces, int n_face_blocks, int reps,
                             double ms[8], char names[256]);
int hfx_general_kernel_bytes(hfx_eles *const *eles, int n_ele_blocks, double bytes[8]);
/* The launch forms the general fused stage runs on this block with the context's current options (read-only; valid once a fused-4
 * call has prepared the block, refused before): out[0] size class (index of the kernel instantiation with compile-time sizes:
 * 0-2 tetrahedra P1-P3, 3-5 prisms P1-P3; -1: the size-generic kernels), out[1] waves of the flux kernel (3, 4, 8), out[2] 1: its
 * staging requests all loads up front, 0: the looped staging, out[3] 1: it forms the interior LDG corrections itself (no
 * face_delta_kernel), out[4] 1: its LES form, out[5] waves of the update kernel (4, 8), out[6] 1: the folded correction
 * (opp_2 - opp_3 opp_1), out[7] bytes of the flux kernel's LDS image of a batch. */
int hfx_general_plan(hfx_eles *e, int out[8]);
/* Over-integration and shock capturing on this block: what the registered matrices allow and what ran last (read-only; valid at
 * any time).  out[0] 1: opp_over_int_cubpts and over_int_filter were recognised as Kronecker powers of 1-D matrices (the
 * sum-factorised kernel can run), 0: not (or none registered); out[1], out[2] their 1-D extents N (solution points) and Nc
 * (cubature points), 0 where out[0] is 0; out[3] 1: the matrices of the form folded into the divergence are set (a split fused
 * stage made them); out[4] 1: inv_vandermonde and exp_filter were recognised, out[5] their N.  out[6]: the form the last
 * hfx_eles_evaluate_invFlux_over_int of this block ran, per method or inside a stage (1 sum-factorised, 0 dense, -1 none since
 * the registration); out[7] the same for hfx_eles_shock_capture.  Option "tensor_ops" 0 and HFX_CONTRACT_DENSE leave out[0..5] as
 * they are and show in out[6..7]. */
int hfx_eles_tensor_ops_plan(hfx_eles *e, int out[8]);
/* The same for a block of triangles, which fused 4 runs through the 2-D simplex fused stage (read-only; valid once a fused-4 call or a
 * deferred stage has prepared the block, refused before): out[0] size class (order - 1: the kernel instantiation of P1..P5), out[1]
 * elements per group, out[2] waves per workgroup, out[3] 1: the element kernel forms the interior LDG corrections itself (no
 * face_delta_kernel), out[4] bytes of the element kernel's LDS image (operators + one group), out[5] the update kernel's, out[6..7] 0.
 * hfx_time_general_kernels and hfx_general_kernel_bytes answer for such a block with the stage's four steps. 
 * With option "blocks_2d" 1 it answers for every block the stage has prepared; a block of quadrilaterals of order p has size class
 * 5 + (p - 1) (orders 1-4: 4/8, 9/12, 16/16, 25/20 solution / flux points, 64, 32, 16, 8 elements per group). */
int hfx_simplex2d_plan(hfx_eles *e, int out[8]);
/* With option "blocks_2d" 1 (default 0: every call below is refused as ever) hfx_run_steps_blocks(..., 4), hfx_time_general_kernels
 * and the deferred stage run the 2-D simplex fused stage over SEVERAL two-dimensional blocks -- a mixed quadrilateral / triangle mesh,
 * several triangle blocks -- and over one block of quadrilaterals: triangles of orders 1-5, quadrilaterals of orders 1-4 on the same
 * dense kernels (plain forms; hfx_simplex2d_plan answers for each block, a quadrilateral block with size class 5 + (order - 1)),
 * all blocks of one order.  An interior-face block between two element blocks (a cross block) takes each side's arrays from its own
 * block; its LDG corrections are face_delta_kernel's (no partner word crosses blocks).  Refused before the first launch, naming
 * fused 0: a block with a registered LES closure, over-integration or shock capturing, a partition-face block, blocks of different
 * order, a three-dimensional block beside a two-dimensional one, quadrilaterals of order 5 and above;
 * hfx_run_steps_partitioned_blocks keeps refusing several two-dimensional blocks.  A single block of triangles runs as with 0.
 * What ONE stage over the prepared blocks launches (read-only; the list of blocks of the fused-4 call that prepared them, refused
 * otherwise): out[0] element blocks, out[1] non-empty interior-face blocks, out[2] how many of them are cross blocks, out[3]
 * face_delta_kernel launches per stage, out[4] all launches per stage (boundary sweeps, face_delta_kernel, one element and one update
 * kernel per block, one face_flux2_kernel per interior-face block), out[5..7] 0. */
int hfx_simplex2d_stage_plan(hfx_eles *const *eles, int n_ele_blocks, int out[8]);
/* What the partitioned loop (hfx_run_steps_partitioned_blocks, or the deferred stage) runs on a block of triangles (read-only; valid
 * once a stage has prepared the block, refused before).  The kernels walk groups of out[1] of hfx_simplex2d_plan consecutive
 * elements: out[0] partition groups (an element of the group owns a partition flux point), out[1] interior groups (launched
 * first, beside the solution message), out[2] 1: the element kernel reads the partners of partition points from the receive
 * record itself (option gather_delta, one partition-face block), 0: mpi_delta_kernel writes their LDG corrections, out[3] 0.
 * A block prepared by hfx_run_steps_blocks(..., 4) has no partition groups. */
int hfx_simplex2d_partition_plan(hfx_eles *e, int out[4]);
/* Shock capturing on a block of triangles behind / inside the 2-D simplex fused stage (read-only; valid once a fused-4 call or a
 * deferred stage has prepared the block, refused before): out[0] 1: the update kernel carries the filter (the registration has the
 * form of eles_tris::shock_det_persson and option "fold_shock" is 1), out[1] bytes of the LDS image of the update kernel that runs
 * (with the filter: + inv_vandermonde, exp_filter, a group's squared modal coefficients and sensors), out[2] the first mode the
 * sensor's numerator sums, p (p + 1) / 2, out[3] per-method launches behind every stage for the filter (0 when folded or nothing is
 * registered; else the two dense contractions, the sensor and the selection kernel and extrapolate_solution). */
int hfx_simplex2d_shock_plan(hfx_eles *e, int out[4]);
/* Over-integration (hfx_eles_set_over_int) on a block of triangles inside / in front of the 2-D simplex fused stage (read-only; valid
 * once a fused-4 call or a deferred stage has prepared the block, refused before): out[0] 1: the element kernel carries it (something
 * is registered and option "fold_over_int" is 1; every instantiated order P1..P5 folds), out[1] cubature points of the registration (0:
 * none), out[2] cubature points per chunk the element kernel walks (the order's solution points), out[3] chunks, out[4] bytes of the
 * element kernel's LDS image (the same in every form: a chunk lives in the regions of the LDG corrections and the gradient), out[5]
 * per-method launches in front of every stage (0 when folded or nothing is registered; else the three of
 * hfx_eles_evaluate_invFlux_over_int, after which the element kernel reads tdisf_upts), out[6..7] 0.  In the unfolded form
 * hfx_time_general_kernels reports those launches in slot 4 (name evaluate_invFlux_over_int) and hfx_general_kernel_bytes their bytes
 * there; folded, slot 4 stays 0 and the element kernel's bytes grow by the cubature points' metrics. */
int hfx_simplex2d_over_int_plan(hfx_eles *e, int out[8]);

/* An LES closure on a block of triangles in the 2-D simplex fused stage (valid once a fused-4 call or a deferred stage has prepared
 * the block, refused before): out[0] 1: the element kernel's LES form evaluates the closure and the projected viscous flux carries
 * F_sgs . n (sgs_model 0, 1, 2, 4 on a viscous context, registered with the block's own Jacobian_fpts: sum_k Jacobian_fpts(i,k)
 * JGinv_fpts(k,j) = detjac_fpts delta_ij to 1e-9 of max |detjac_fpts|; any other registration is refused before the first launch, run
 * fused 0), out[1] sgs_model of the registration (-1: none; 3, SVV, has no SGS flux: the plain kernels run behind the step loop's
 * filter, and partitioned blocks refuse it), out[2] 1: the kernel reads Lu / Le (the similarity models 2 and 4), out[3] per-method
 * kernels in front of a step's FIRST stage (0 for the eddy-viscosity models; the 5 of hfx_eles_calc_sgs_terms for models 2 and 4; 3
 * for SVV: filter, products, and the extrapolation of the filtered state), 0 in front of every other stage, out[4] bytes of the
 * element kernel's LDS image (the same in every form), out[5..7] 0.  hfx_general_kernel_bytes counts the added reads of the element
 * kernel per stage: 8 B per solution point (the squared length scale), 8 B per flux point (tdA_fpts) and, for models 2 and 4, 40 B
 * per solution point (Lu, Le). */
int hfx_simplex2d_les_plan(hfx_eles *e, int out[8]);

#ifdef __cplusplus
}
#endif
#endif
