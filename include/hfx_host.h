/* hfx_host.h -- extern "C" facade of libhfx_host: the host-side mirror of the reference's
 * eles / int_inters / solver interface (C++ classes under hifiles-solver_amd/csrc/host, same
 * method names as /root/reference/include/eles.h:55-125, int_inters.h:48-60, solver.h:34),
 * built on the C ABI of libhfx (hfx.h).  The facade exists for test / bench plumbing written
 * in Python; a C++ caller uses the classes directly.
 *
 * A "case" is a periodic box of quads (dims 2) or hexes (dims 3) -- the synthetic meshes of
 * BASELINE.json's configurations -- with its elements, metrics, interior faces and initial state.
 */
#ifndef HFX_HOST_H
#define HFX_HOST_H

#include "hfx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hfxh_case hfxh_case;

/* one boundary group: `bc_<name>_type` (as hfx_bc_flag) and its parameters as the reference's input file
 * gives them, DIMENSIONAL (/root/reference/src/input.cpp:328-437); T_total / T_total_old < 0: not given
 * (default T_free_stream) */
typedef struct hfxh_bc_desc
{
  int flag, pressure_ramp;
  double rho, u, v, w, p_static, T_static, p_total, T_total, nx, ny, nz, mach;
  double p_ramp_coeff, T_ramp_coeff, p_total_old, T_total_old;
  int use_wm; /* `bc_<name>_use_wm` of an isotherm_wall / adiabat_wall group: read only when the case has a wall model */
} hfxh_bc_desc;

/* inputs are DIMENSIONAL, exactly the keys of the reference's input file
 * (/root/reference/src/input.cpp:62-327); they are non-dimensionalised as input::setup_params does */
typedef struct hfxh_case_desc
{
  int dims;         /* 2 quads, 3 hexes */
  int n[3];         /* cells per direction (>= 3) */
  int order;        /* `order` */
  double length;    /* box edge = dx_cyclic = dy_cyclic = dz_cyclic */
  double amp;       /* amplitude of the smooth periodic vertex deformation (0: uniform) */
  const double *xv; /* optional vertices (nv,dims) column-major, v = ix + (nx+1)*(iy + (ny+1)*iz); NULL: generate */
  const double *loc_1d_upts; /* optional order+1 solution-point abscissae (e.g. the reference's data/JacobiGQ.bin
                              * row, which is not bit-symmetric); NULL: computed Gauss / Lobatto nodes */
  int viscous, riemann_solve_type, adv_type, ic_form;
  int upts_type;   /* upts_type_hexa / upts_type_quad: 0 Gauss, 1 Gauss-Lobatto */
  int vcjh_scheme; /* vcjh_scheme_hexa / _quad: 0 eta given, 1 DG, 2 SD, 3 Huynh, 4 c+ */
  double eta;
  int fix_vis;
  double dt, ldg_beta, ldg_tau;
  double gamma, prandtl, S_gas, T_gas, R_gas, mu_gas;
  double Mach_free_stream, rho_free_stream, L_free_stream, T_free_stream;
  double rho_c_ic, Mach_c_ic, T_c_ic;     /* viscous initial condition */
  double u_c_ic, v_c_ic, w_c_ic, p_c_ic;  /* inviscid initial condition */
  /* block decomposition (all 0: one rank).  n[] is THIS rank's block, the global box has n[d]*pgrid[d]
   * cells per direction and edge `length`; rank = px + pgrid[0]*(py + pgrid[1]*pz).  Stands in for the
   * reference's ParMETIS partition (src/mesh.cpp:72-314). */
  int rank, nproc, pgrid[3];
  /* boundary groups (n_bcs 0: fully periodic).  side_bc[f], f = element-local face number of the side of the
   * GLOBAL box (hexes: z- y- x+ y+ x- z+; quads: y- x+ y+ x-), is an index into bcs; a group of type
   * HFX_BC_CYCLIC (or index -1) makes the side periodic.  Mirrors the mesh file's boundary groups + the input
   * file's bc_<name>_* keys. */
  int n_bcs;
  const hfxh_bc_desc *bcs;
  int side_bc[6];
  /* time step: dt_type 0 fixed `dt`, 1 global CFL minimum, 2 local CFL steps (src/input.cpp:141-158) */
  int dt_type;
  double CFL;
  /* polynomial de-aliasing and shock capturing, the reference's keys (src/input.cpp:248-263): over_int,
   * over_int_order; shock_cap (1: exponential modal filter), shock_det_field (0 density, 1 total energy), s0,
   * expf_fac, expf_order, expf_cutoff.  The matrices (opp_over_int_cubpts, over_int_filter, JGinv_over_int_cubpts,
   * inv_vandermonde, exp_filter, norm_basis_persson, persson_high_modes -- the last read as doubles) are built by the host
   * mirror (csrc/host/eles_modal.cpp) and handed out by hfxh_case_get_array. */
  int over_int, over_int_order;
  int shock_cap, shock_det_field;
  double s0, expf_fac;
  int expf_order, expf_cutoff;
  /* LES closure (src/input.cpp:167-182): LES 1, SGS_model 1 WALE / 2 WALE + similarity / 3 SVV / 4 similarity, C_s,
   * filter_ratio, prandtl_t (0: 0.9); filter_type at the end of this struct */
  int LES, SGS_model;
  double C_s, filter_ratio, prandtl_t;
  int p_res; /* plot points per edge (`p_res`, src/input.cpp:110); 0: the reference's default 2 */
  /* self_partition[d] != 0: the wrap-around faces of the periodic direction d (which must not be split, pgrid[d] 1)
   * become partition faces whose neighbour is this rank itself.  The complete partition-face path -- pack, exchange,
   * one-sided kernels -- then runs on ONE rank: how the RCCL transport is exercised on a one-GPU box, and how
   * bench.py prices the partitioned stage on one GPU (--self-partition). */
  int self_partition[3];
  /* LES closures 2 (WALE + similarity), 3 (spectral vanishing viscosity), 4 (similarity) filter the solution:
   * filter_type 0 high-order-commuting Vasilyev, 1 discrete Gaussian, 2 modal, other: average (src/input.cpp:173,
   * src/eles_hexas.cpp:583-790, src/eles_quads.cpp:428-622; the mirror builds filter_upts in csrc/host/eles_modal.cpp) */
  int filter_type;
  /* the mass-flux body force of periodic channels: `body_forcing` (src/input.cpp:312; 1: on, three-dimensional cases), and two
   * keys of this mirror, forcing_area and forcing_mdot0 -- the inflow area and the target mass flux, which the reference
   * hard-codes (src/eles.cpp:5393-5395); 0: its value, 9.162.  The mirror then builds the surface cubature of the hexahedra
   * (set_inters_cubpts, set_opp_inters_cubpts, set_transforms_inters_cubpts), selects the inflow faces by the reference's rule
   * (cyclic group, x-component of the unit normal at the first cubature point == -1; src/eles.cpp:5312-5338), registers them
   * with hfx_eles_set_body_force, and CalcResidual evaluates the force at the first RK stage of every step. */
  int body_forcing;
  double forcing_area, forcing_mdot0;
  /* the direction of the initial / reference velocity of a viscous case, `nx_c_ic`, `ny_c_ic`, `nz_c_ic` (src/input.cpp:646-649);
   * all three 0: the reference's default (1, 0, 0) */
  double nx_c_ic, ny_c_ic, nz_c_ic;
  /* wall forces (src/input.cpp:102-107): `calc_force` 1, `area_ref` (dimensional; must then be positive) and `monitor_cp_freq`
   * (0: never, src/input.cpp:536-537).  The mirror then builds the surface cubature of the quadrilaterals / hexahedra (src/eles.cpp:4023),
   * lists the wall faces, and hfxh_case_to_device registers them (hfx_eles_set_wall_faces) and the reference state
   * rho_c_ic, u_c_ic, v_c_ic, w_c_ic, p_c_ic, area_ref (hfx_ctx_set_force_reference). */
  int calc_force;
  double area_ref;
  int monitor_cp_freq;
  /* `wall_model` (src/input.cpp:176): 0 none, 1 Werner-Wengle, 2 Breuer-Rodi, anything else "Wall model not implemented!"; reads
   * prandtl_t above (0: 0.9) and the groups' use_wm.  The mirror finds every model face's input point (eles::calc_wm_upts_dist, in
   * the face's own element: nothing crosses ranks) and hfxh_case_to_device registers the model and the points
   * (hfx_ctx_set_wall_model, hfx_bdy_inters_set_wall_model_points). */
  int wall_model;
} hfxh_case_desc;

const char *hfxh_last_error(void);

/* host only: builds operators, metrics, faces, initial state (no GPU needed) */
int hfxh_case_create(const hfxh_case_desc *d, hfxh_case **out);
int hfxh_case_destroy(hfxh_case *c);
/* {n_eles, n_upts, n_fpts, n_fields, n_dims, order, ele_type, n_rk_stages} */
int hfxh_case_sizes(hfxh_case *c, int sizes[8]);
int hfxh_case_params(hfxh_case *c, hfx_params *p);
/* host array by the reference's member name (opp_0, opp_1_0, ..., JGinv_upts, disu_upts0, ...) */
int hfxh_case_get_array(hfxh_case *c, const char *name, const double **ptr, int dims[4]);
int hfxh_case_get_faces(hfxh_case *c, const int **L, const int **R, int *n_fpts_per_inter, int *n_inters);

/* boundary faces (bdy_inters): left offsets L(j,i), boundary_id(i), and the non-dimensional bc_list
 * (what input::read_boundary_param leaves in run_input.bc_list) with R_ref and ramp_counter */
int hfxh_case_get_bdy_faces(hfxh_case *c, const int **L, const int **boundary_id, int *n_fpts_per_inter, int *n_inters);
int hfxh_case_get_bcs(hfxh_case *c, const hfx_bc **bcs, int *n_bcs, double *R_ref, int *ramp_counter);
/* the wall model's input points: per boundary face (n_inters entries, the order of hfxh_case_get_bdy_faces) the solution point of
 * the face's element and its wall distance; faces without a model hold 0.  On a mesh where several solution points tie for the
 * largest distance (a Cartesian one: the whole far row) the point is the first strictly larger in the mirror's own arithmetic,
 * which need not be the reference's pick.  Any pointer may be NULL */
int hfxh_case_get_wall_model_points(hfxh_case *c, int *wall_model, const int **upt, const double **dist, int *n_inters,
                                    int *n_wall_model_inters);
/* partition faces (mpi_inters): left offsets L(j,i), received-record slots Rlut(j,i), and Nout_proc[nproc]
 * = faces shared with each rank; a rank's faces are contiguous and ordered by rank */
int hfxh_case_get_mpi_faces(hfxh_case *c, const int **L, const int **Rlut, int *n_fpts_per_inter, int *n_inters,
                            const int **nout_proc);
/* exchange hook called by mpi_inters::send_* (phase 0, after packing) and receive_* (phase 1); kind 0
 * solution, 1 corrected gradient.  The transport (RCCL / gloo through torch.distributed) belongs to the caller. */
typedef void (*hfxh_exchange_cb)(void *user, int kind, int phase);
int hfxh_case_set_exchange(hfxh_case *c, hfxh_exchange_cb fn, void *user);

/* neighbour segments of the partition-face block (hfx_mpi_inters_set_neighbours): seg[s] = {peer, send_first, recv_first,
 * count}; for a block without self-partition faces: one segment per neighbour rank, send_first == recv_first */
int hfxh_case_get_mpi_segments(hfxh_case *c, const int **peer, const int **send_first, const int **recv_first, const int **count,
                               int *n_seg);
/* MPI_Allreduce(MIN) hook of calc_time_step (dt_type 1 on more than one rank) when the transport is the caller's */
typedef double (*hfxh_reduce_min_cb)(void *user, double v);
int hfxh_case_set_reduce_min(hfxh_case *c, hfxh_reduce_min_cb fn, void *user);
/* collective over the case's nproc ranks, after hfxh_case_to_device: the library's own transport (RCCL, hfx_comm_*) with the
 * 128-byte id of hfx_comm_get_unique_id (made on rank 0, distributed by the launcher).  From then on send_* / receive_*,
 * hfxh_case_run_partitioned and calc_time_step's MIN reduction go through it instead of the hooks. */
int hfxh_case_set_comm(hfxh_case *c, const char *unique_id);
/* hfx_comm_info of the case's communicator (after hfxh_case_set_comm) */
int hfxh_case_comm_info(hfxh_case *c, int *nranks, int *rank, int *device, char pci_bus_id[32]);
/* hfx_time_partitioned on this case's blocks: ms[0..3] phases 1-4, ms[4] solution exchange, ms[5] flux exchange, ms[6] stage */
int hfxh_case_time_partitioned(hfxh_case *c, int reps, double ms[8]);

/* ---- tetrahedra / prisms as producers of operators and metrics (row a17) ----------------------------------------------
 * eles_tets / eles_pris of the host mirror (csrc/host/eles_simplex.cpp) set up for `order` and the given straight-sided
 * elements: shape (3, n_spts, n_eles) column-major, n_spts 4 (tetrahedra, ele_type 2) or 6 (prisms, ele_type 3), the
 * reference's eles::shape.  Builds loc_upts, tloc_fpts, tnorm_fpts, opp_0 .. opp_6 and the metrics (set_transforms);
 * read them with hfxh_simplex_get_array (names as hfxh_case_get_array).  loc_1d_upts: optional 1-D abscissae of the
 * prism's line direction (NULL: computed Gauss nodes). */
typedef struct hfxh_simplex hfxh_simplex;
int hfxh_simplex_create(int ele_type, int order, int viscous, int n_eles, const double *shape, const double *loc_1d_upts,
                        hfxh_simplex **out);
/* the same with another member of the VCJH family on the tetrahedron / on the prism's triangle: vcjh_scheme_tet / vcjh_scheme_tri
 * 0 (the filter's c given: c_tet / c_tri), 1 DG, 2 SD-like, 3 Huynh-like, 4 c+ (/root/reference/src/eles_tets.cpp:1305-1390,
 * src/funcs.cpp:717-795) */
int hfxh_simplex_create_vcjh(int ele_type, int order, int viscous, int n_eles, const double *shape, const double *loc_1d_upts,
                             int vcjh_scheme, double c, hfxh_simplex **out);
/* the general form: the input keys the simplex classes read beyond order / viscous.
 *  - vcjh_scheme, c: as above;
 *  - SGS_model >= 0: a run with an LES closure (run_input.LES = 1; < 0: none): set_transforms also fills Jacobian_fpts (what
 *    hfx_eles_set_les takes), and for the closures that filter the solution (SGS_model 2, 3, 4) eles_tets builds filter_upts
 *    (/root/reference/src/eles_tets.cpp:576-690: filter_type 2 modal, 3 element average; 0 and 1 stop as the reference does).  The
 *    reference's prism class builds no filter (src/eles_pris.cpp:134): SGS_model >= 2 is refused there;
 *  - shock_cap 1: the operators of shock capturing (what hfx_eles_set_shock_capture takes): inv_vandermonde, exp_filter,
 *    norm_basis_persson, persson_high_modes (read as doubles) -- src/eles_tets.cpp:705-797, src/eles_pris.cpp:609-730.
 * n_spts: shape nodes per element -- 0 for the straight-sided shapes, else 4 or 10 (the quadratic tetrahedron of
 * src/eles_tets.cpp:1047-1069, nodes 4-9 on the edges (0,1) (0,2) (0,3) (1,2) (2,3) (3,1)), 6 or 15 (the quadratic prism of
 * src/eles_pris.cpp:1115-1146); shape is then (3, n_spts, n_eles). */
typedef struct hfxh_simplex_keys
{
  int vcjh_scheme; /* vcjh_scheme_tet / vcjh_scheme_tri */
  double c;        /* c_tet / c_tri (scheme 0) */
  int SGS_model;   /* < 0: no LES */
  int filter_type;
  double filter_ratio;
  int shock_cap;   /* 0 off, 1 exponential filter */
  double expf_fac;
  int expf_order, expf_cutoff;
} hfxh_simplex_keys;
int hfxh_simplex_create_keys(int ele_type, int order, int viscous, int n_eles, int n_spts, const double *shape,
                             const double *loc_1d_upts, const hfxh_simplex_keys *keys, hfxh_simplex **out);
int hfxh_simplex_get_array(hfxh_simplex *s, const char *name, const double **ptr, int dims[4]);
int hfxh_simplex_destroy(hfxh_simplex *s);

/* device */
int hfxh_case_to_device(hfxh_case *c, int device);
/* deferred execution of the mirrored method calls (hfx.h, option "deferred"): ON by default -- hfxh_case_CalcResidual / hfxh_case_run
 * make the reference's calls one by one, libhfx records them and runs every whole stage as one fused stage.  0: every call
 * launches its own kernels (the per-method path).  May be called before or after hfxh_case_to_device. */
int hfxh_case_set_deferred(hfxh_case *c, int on);
int hfxh_case_handles(hfxh_case *c, hfx_ctx **ctx, hfx_eles **e, hfx_inters ***faces, int *n_face_blocks);
int hfxh_case_CalcResidual(hfxh_case *c); /* the mirrored CalcResidual (src/solver.cpp:50-223) */
int hfxh_case_run(hfxh_case *c, int n_steps); /* the mirrored RK loop (src/HiFiLES.cpp:194-221) */
/* device handle of the partition-face block (NULL on one rank) */
int hfxh_case_mpi_handle(hfxh_case *c, hfx_inters **f);
/* the RK loop through hfx_stage_partitioned (split fused kernels), exchanging between its phases */
int hfxh_case_run_partitioned(hfxh_case *c, int n_steps);
/* ASCII restart files of the reference, "Rest_%09d_p%04d.dat" in `dir` (output::write_restart_ascii
 * src/output.cpp:1753-1818, read_restart_ascii src/solver.cpp:377-434): host state in / out; a case that is on
 * the device downloads before writing and uploads after reading */
int hfxh_case_write_restart(hfxh_case *c, const char *dir, int file_num);
int hfxh_case_read_restart(hfxh_case *c, const char *dir, int file_num, int n_files);
/* calc_time_step (src/solver.cpp:484-549) on the device; hfxh_case_run calls it before every step */
int hfxh_case_calc_time_step(hfxh_case *c, double *dt);
/* eles::calc_disu_ppts for every element (device contraction + download): out (n_ppts, n_eles, n_fields) */
int hfxh_case_calc_disu_ppts(hfxh_case *c, const double **out, int dims[3]);
int hfxh_case_sync_host(hfxh_case *c);        /* cp_*_gpu_cpu of state, divergence, gradient */

/* ---- time-averaged fields (run_input.average_fields, src/input.cpp:115-133) ---------------------------------------------
 * names[n] out of rho_average, u_average, v_average, w_average, e_average in any letter case (stored lower-cased, as the
 * reference does); a name outside the five, and w_average in a two-dimensional case, are refused and leave the case as it
 * was.  Host only; a case that is on the device also registers them there (zeroed averages), hfxh_case_to_device does so
 * otherwise.  hfxh_case_run and hfxh_case_run_partitioned then update the averages after every time step
 * (src/HiFiLES.cpp:240-245). */
int hfxh_case_set_average_fields(hfxh_case *c, int n, const char *const *names);
/* run_input.n_average_fields and the stored names (names may be NULL) */
int hfxh_case_get_average_fields(hfxh_case *c, int *n, const char *names[HFX_MAX_AVERAGE_FIELDS]);
/* disu_average_upts downloaded: out (n_upts, n_eles, n_average_fields) */
int hfxh_case_get_averages(hfxh_case *c, const double **out, int dims[3]);
/* eles::calc_time_average_ppts for every element: out (n_ppts, n_eles, n_average_fields) */
int hfxh_case_calc_time_average_ppts(hfxh_case *c, const double **out, int dims[3]);
/* FlowSol.time, i_steps (time steps of this run; a restart read resets it) and run_input.spinup_time; any pointer may be NULL */
int hfxh_case_get_clock(hfxh_case *c, double *time, int *i_steps, double *spinup_time);

/* ---- point probes (run_input.probe; src/probe_input.cpp, output::write_probe src/output.cpp:1440-1545) -------------------------
 * positions (n_dims, n) column-major, physical; names[n_fields] out of rho, u, v, w, specific_total_energy, pressure in any letter
 * case (stored lower-cased, as probe_input::read_probe_input does); probe_freq in steps; capacity: the samples the device
 * history holds between two reads.  The case locates every point -- calc_p2c of the element class (the first element for which
 * the point and the centroid lie on the same side of every face plane), then eles::pos_to_loc (Newton from 0, until the step
 * is at most 1e-6; a point that does not converge within 50 iterations is an error, where the reference loops for ever) -- and
 * builds each probe's operator row (eles::set_opp_probe).  A point found in no element is not this rank's and is left out, as
 * in the reference.  A point on the face of two ranks is located by both: removing the duplicate needs the reference's
 * all-gather and is the CALLER'S.  A refusal leaves the case as it was.  n_fields = 0 drops the probes.
 * A case on the device registers at once (hfx_ctx_set_probes, hfx_eles_set_probes), hfxh_case_to_device does otherwise.
 * hfxh_case_run and hfxh_case_run_partitioned then sample after every step with i_steps % probe_freq == 0, behind the time
 * averages (src/HiFiLES.cpp:289-297). */
int hfxh_case_set_probes(hfxh_case *c, int n, const double *positions, int n_fields, const char *const *names, int probe_freq,
                         int capacity);
/* the located probes: their element (run_probe.p2c), element class (p2t), reference location loc_probe (n_dims, n_located)
 * and index in the positions given (global_index); any pointer may be NULL */
int hfxh_case_get_probes(hfxh_case *c, int *n_located, const int **p2c, const int **p2t, const double **loc_probe,
                         const int **global_index);
/* one sample now, at the case's time and step (hfx_eles_sample_probes) */
int hfxh_case_sample_probes(hfxh_case *c);
int hfxh_case_probe_count(hfxh_case *c, int *n_samples, int *n_probes);
/* hfx_eles_read_probes of the case's block: values (n_fields, n_located, n_samples).  dimensional != 0, and only for a viscous
 * case: rho * rho_ref, u v w * uvw_ref, specific_total_energy * uvw_ref^2, pressure * p_ref, times * time_ref
 * (src/output.cpp:1475-1535) */
int hfxh_case_read_probes(hfxh_case *c, int dimensional, int max_samples, double *times, int *steps, double *values, int *n_samples);
/* {rho_ref, uvw_ref, p_ref, time_ref, viscous} of the case */
int hfxh_case_ref_values(hfxh_case *c, double ref[5]);
/* the pieces, for n points at once: calc_p2c + pos_to_loc (p2c[i] = -1 and loc = 0 for a point in no element); calc_pos of
 * (ele[i], loc(:, i)); pos_to_loc in a given element; opp_probe (n_upts, n) at loc (n_dims, n).  The _simplex_ forms: the same on
 * the tetrahedra / prisms of an hfxh_simplex */
int hfxh_case_locate(hfxh_case *c, int n, const double *positions, int *p2c, double *loc);
int hfxh_case_calc_pos(hfxh_case *c, int n, const int *ele, const double *loc, double *positions);
int hfxh_case_pos_to_loc(hfxh_case *c, int ele, const double *position, double *loc);
int hfxh_case_opp_probe(hfxh_case *c, int n, const double *loc, double *opp_probe);
int hfxh_simplex_locate(hfxh_simplex *s, int n, const double *positions, int *p2c, double *loc);
int hfxh_simplex_calc_pos(hfxh_simplex *s, int n, const int *ele, const double *loc, double *positions);
int hfxh_simplex_pos_to_loc(hfxh_simplex *s, int ele, const double *position, double *loc);
int hfxh_simplex_opp_probe(hfxh_simplex *s, int n, const double *loc, double *opp_probe);

/* ---- mass-flux body force (hfxh_case_desc.body_forcing) ------------------------------------------------------------------
 * the surface cubature is read with hfxh_case_get_array: opp_inters_cubpts_<l>, weight_inters_cubpts_<l>, loc_inters_cubpts_<l>,
 * tnorm_inters_cubpts_<l>, inter_detjac_inters_cubpts_<l> (n_cubpts, n_eles), norm_inters_cubpts_<l> (n_cubpts, n_eles, n_dims)
 * for local face l -- per ELEMENT, where the reference keeps them per boundary element */
int hfxh_case_get_forcing(hfxh_case *c, int *body_forcing, double *forcing_area, double *forcing_mdot0);
/* new forcing_area / forcing_mdot0; a case on the device registers again, which resets its controller (hfx_eles_set_body_force) */
int hfxh_case_set_forcing(hfxh_case *c, double forcing_area, double forcing_mdot0);
/* MPI_Allreduce(SUM) hook of eles::evaluate_body_force (src/eles.cpp:5375-5385) on more than one rank when the transport is
 * the caller's: fn(user, v, n) replaces v[n] by its sum over the ranks.  With hfxh_case_set_comm the library's communicator sums. */
typedef void (*hfxh_reduce_sum_cb)(void *user, double *v, int n);
int hfxh_case_set_reduce_sum(hfxh_case *c, hfxh_reduce_sum_cb fn, void *user);

/* ---- exact-solution error norms and integral diagnostics (run_input.test_case, error_norm_type, integral_quantities) ------
 * Setters in the style of hfxh_case_set_average_fields: called after hfxh_case_create, before hfxh_case_to_device (a case that
 * is on the device registers again at once).  While either is active the quadrilaterals / hexahedra of the case carry the
 * reference's volume cubature -- loc_volume_cubpts (n_dims,n_cubpts) and weight_volume_cubpts (n_cubpts): the tensor Gauss rule
 * with order + 1 points per direction, first direction fastest (src/eles_hexas.cpp:87,376, src/eles_quads.cpp:97,317);
 * opp_volume_cubpts (n_cubpts,n_upts) (src/eles.cpp:3667); vol_detjac_vol_cubpts (n_cubpts,n_eles) (src/eles.cpp:4600-4633); and,
 * for a test case, pos_volume_cubpts (n_cubpts,n_eles,n_dims) -- readable through hfxh_case_get_array and registered with the
 * device block (hfx_eles_set_volume_cubpts, hfx_eles_set_error_points).  With neither active none of the five exists.
 *
 * test_case 0: none; 1: isentropic vortex; 5: Couette flow, whose u_wall is velocity(0) of the isothermal wall that moves and
 * whose T_wall is T_static of the isothermal wall at rest (src/eles.cpp:5219-5230) -- a missing wall is refused by name, where
 * the reference reads an uninitialised value.  2, 3, 4 (advection-diffusion) and unknown cases are refused, as is an
 * error_norm_type other than 1 (L1) and 2 (L2, the reference's default, src/input.cpp:109).  A refusal leaves the case as it was. */
int hfxh_case_set_test_case(hfxh_case *c, int test_case, int error_norm_type);
/* what is set; u_wall and T_wall as found among the boundary groups (test case 5, else 0).  Any pointer may be NULL */
int hfxh_case_get_test_case(hfxh_case *c, int *test_case, int *error_norm_type, double *u_wall, double *T_wall);
/* names[n] out of kineticenergy, enstropy (the reference's spelling), pressuredilatation, straincolonproduct,
 * devstraincolonproduct, any letter case; another name is refused with "integral diagnostic quantity not recognized" */
int hfxh_case_set_integral_quantities(hfxh_case *c, int n, const char *const *names);
/* output::compute_error (src/output.cpp:2052-2110) without the file, at the mirror's clock: error (2,n_fields) column-major, row 0
 * the solution, row 1 the gradient (viscous cases); summed over the case's blocks, then over the ranks -- the library's
 * communicator, else ONE call of the hook of hfxh_case_set_reduce_sum with 2 n_fields values -- then the square root for
 * error_norm_type 2.  The case must be on the device. */
int hfxh_case_compute_error(hfxh_case *c, double *error);
/* output::CalcIntegralQuantities (src/output.cpp:2017-2038): integral_quantities[n_integral_quantities] over blocks and ranks,
 * on top of hfx_eles_CalcIntegralQuantities (which reads the corrected gradient of the last per-method stage) */
int hfxh_case_CalcIntegralQuantities(hfxh_case *c, double *integral_quantities);
/* ---- the integral monitor: the Diagnostics[...] columns of history.plt (src/HiFiLES.cpp:247-266) --------------------------
 * run_input.monitor_res_freq (default 100; 0 means 1000, src/input.cpp:101,534-535) and the samples the device history holds.
 * With integral quantities set and capacity >= 1 the case has a monitor (hfx_ctx_set_integral_monitor; registered here on a
 * device case, by hfxh_case_to_device otherwise, and again by hfxh_case_set_integral_quantities): hfxh_case_run and
 * hfxh_case_run_partitioned then take one sample after every step with i_steps == 1 || i_steps % monitor_res_freq == 0,
 * behind the time averages and the probes, and refuse a call whose samples the history cannot hold before its first launch.
 * capacity 0 (the default): no monitor.  A sample pairs the state after the step with grad_disu_upts of the last RK stage, as
 * the reference does; with deferred execution the pending last stage then runs call by call.  A refusal -- a negative value,
 * or a quantity that reads the gradient on an inviscid device case -- leaves the case as it was. */
int hfxh_case_set_monitor_res_freq(hfxh_case *c, int monitor_res_freq, int capacity);
int hfxh_case_get_monitor_res_freq(hfxh_case *c, int *monitor_res_freq, int *capacity);
/* one sample now, at the case's time and step (hfx_eles_sample_integral_quantities of every block) */
int hfxh_case_sample_integral_quantities(hfxh_case *c);
int hfxh_case_integral_count(hfxh_case *c, int *n_samples);
/* The rows as HistoryOutput prints them (src/output.cpp:2390-2402), and the histories emptied: values (n_integral_quantities,
 * n_samples) summed over the case's blocks, then over the ranks (src/output.cpp:2023-2050) -- the library's communicator, else
 * the hook of hfxh_case_set_reduce_sum -- and left raw; times x time_ref on a viscous case; steps the iteration column.  Fewer
 * than stored (max_samples) is refused and nothing is lost.  Adapter for src/HiFiLES.cpp:255-258: INTEGRATION.md */
int hfxh_case_read_integral_history(hfxh_case *c, int max_samples, double *times, int *steps, double *values, int *n_samples);
/* ---- the history monitor: the residual and force columns, and with them the whole row of history.plt ---------------------------
 * run_input.res_norm_type (0 infinity, 1 L1, 2 L2 norm; default 2, src/input.cpp:108; anything else is refused with "norm_type not
 * recognized") and the rows the device history holds; capacity 0 (the default): no monitor.  The forces of a row follow the case's
 * calc_force, the frequency is monitor_res_freq (hfxh_case_set_monitor_res_freq).  Registered (hfx_ctx_set_history_monitor) here on
 * a device case, by hfxh_case_to_device otherwise.  hfxh_case_run and hfxh_case_run_partitioned then take one row after every step
 * with i_steps == 1 || i_steps % monitor_res_freq == 0, behind the sample of the integral monitor, with deferred execution on and
 * off, and refuse a call whose rows the history cannot hold before its first launch. */
int hfxh_case_set_history(hfxh_case *c, int res_norm_type, int capacity);
/* n_cols: n_fields + (calc_force: n_dims + 2) + (the integral monitor: n_integral_quantities) + 1.  Any pointer may be NULL */
int hfxh_case_get_history(hfxh_case *c, int *res_norm_type, int *capacity, int *n_cols);
/* The finish of output::CalcNormResidual (src/output.cpp:2236-2246), host arithmetic: sum[n_fields] -- the max (type 0) or the sums
 * (types 1, 2) of eles::compute_res_upts over blocks and ranks -- and n_upts -> sum, sum / n_upts or sqrt(sum) / n_upts (the
 * reference does divide the root by n_upts).  A NaN norm is refused with "NaN residual encountered. Exiting" */
int hfxh_norm_residual(int res_norm_type, int n_fields, const double *sum, long n_upts, double *norm_residual);
/* output::CalcNormResidual (src/output.cpp:2166-2248) now: norm_residual[n_fields] over the case's blocks and the ranks -- the
 * library's communicator, else the hooks of hfxh_case_set_reduce_sum (types 1, 2) / hfxh_case_set_reduce_min (type 0, on the negated
 * values).  The case must be on the device */
int hfxh_case_CalcNormResidual(hfxh_case *c, double *norm_residual);
/* one row now, at the case's time and step (hfx_eles_sample_history of every block) */
int hfxh_case_sample_history(hfxh_case *c);
int hfxh_case_history_count(hfxh_case *c, int *n_rows);
/* The rows as HistoryOutput writes them (src/output.cpp:2375-2402), and the histories -- the integral monitor's too -- emptied:
 * rows (n_cols, n_rows) with the column index fastest, steps the iteration column.  Per row log10(norm_residual) of every field;
 * with calc_force inv + vis force per dimension, then CL, CD; the integral quantities where that monitor is registered; the time,
 * x time_ref on a viscous case.  The computing-time column is left out.  A NaN norm is the reference's error.  Fewer than stored
 * (max_rows) and a case without the monitor are refused before anything is read, and nothing is lost.
 * An error behind that -- a failed reduction over the ranks, the NaN norm, which ends the reference's run -- comes after the blocks'
 * histories have been read and emptied: those rows are gone.  Changing monitor_res_freq (hfxh_case_set_monitor_res_freq) registers
 * both monitors anew and empties both histories; changing the integral quantities alone leaves the history monitor's rows. */
int hfxh_case_read_history(hfxh_case *c, int max_rows, int *steps, double *rows, int *n_cols, int *n_rows);
/* ---- the plot monitor: the rows of the plot file (src/HiFiLES.cpp:273-285; output::write_tec, src/output.cpp:366-427) -----------
 * run_input.diagnostic_fields: names out of u, v, w, energy, mach, pressure, vorticity, q_criterion, scaled_q_criterion, sensor, any
 * letter case (lower-cased as src/input.cpp:125-129 does); another name is refused with "plot_quantity not recognized".  On a device
 * case the context's refusals (hfx_ctx_set_plot_monitor) come back and leave the fields as they were. */
int hfxh_case_set_diagnostic_fields(hfxh_case *c, int n, const char *const *names);
/* run_input.plot_freq (>= 1; the default is the reference's INT32_MAX: never) and the snapshots the device history holds; capacity 0
 * (the default): no monitor.  Registered (hfx_ctx_set_plot_monitor) here on a device case, by hfxh_case_to_device otherwise.
 * hfxh_case_run and hfxh_case_run_partitioned then take one snapshot of every block after every step with i_steps % plot_freq == 0,
 * as the last output of the step (the averages of a row include the step), with deferred execution on and off, and refuse a call
 * whose snapshots the history cannot hold before its first launch.  Deferred, the sample's need mask makes the pending last stage
 * run call by call where a field reads the gradient, and only that stage; with gradient-free fields every stage runs fused. */
int hfxh_case_set_plot(hfxh_case *c, int plot_freq, int capacity);
/* n_cols: n_dims + n_fields + n_average_fields + n_diagnostic_fields; n_points: the plot points of all blocks, the rows of one
 * snapshot.  Any pointer may be NULL */
int hfxh_case_get_plot(hfxh_case *c, int *plot_freq, int *capacity, int *n_cols, long *n_points);
/* one snapshot now, at the case's time and step (hfx_eles_sample_plot of every block) */
int hfxh_case_sample_plot(hfxh_case *c);
int hfxh_case_plot_count(hfxh_case *c, int *n_snapshots);
/* The rows exactly as write_tec prints them, and the histories emptied: rows (n_cols, n_points, n_snapshots) with the column index
 * fastest; per snapshot the blocks in class order, per element and plot point the position (eles::calc_pos_ppts), the conserved
 * fields, the averages, the diagnostic fields.  times (FlowSol.time, what SolutionTime prints) and steps per snapshot.  A NaN is the
 * reference's error: "Nan in tecplot file, exiting" in a conserved or averaged column (src/output.cpp:397), "NaN" with the field's
 * name in a diagnostic one (src/eles.cpp:3996-3999); the histories have been read and emptied by then.  Fewer than stored
 * (max_snapshots) and a case without the monitor are refused before anything is read.  The file itself -- header, connectivity --
 * stays with the caller, as do the plot points of simplex classes. */
int hfxh_case_read_plot_rows(hfxh_case *c, int max_snapshots, double *times, int *steps, double *rows, int *n_snapshots);
/* the inflow faces the reference's rule selects, elements ascending: (element, local face) */
int hfxh_case_get_inflow_faces(hfxh_case *c, const int **ele, const int **inter, int *n_faces);
/* hfx_eles_body_force_state / hfx_eles_body_force_history of the case's block */
int hfxh_case_body_force_state(hfxh_case *c, double *mass_flux, double *ubulk, double *body_force_x, double accumulated[2],
                               double integral[2], long *n_steps);
int hfxh_case_body_force_history(hfxh_case *c, int max_rows, double *rows, int *n_rows);

/* ---- wall forces (hfxh_case_desc.calc_force) --------------------------------------------------------------------------------
 * output::CalcForces (src/output.cpp:1915-2014) without the file, at the mirror's clock: inv_force[n_dims], vis_force[n_dims], *cl,
 * *cd summed over the case's blocks, then over the ranks -- the library's communicator, else ONE call of the hook of
 * hfxh_case_set_reduce_sum with 2 n_dims + 2 values (the MPI_Reduce of :1992-2009; every rank gets the sums).  What the
 * reference puts into every line of history.plt (src/output.cpp:2381-2393).  The case must be on the device; a viscous case reads
 * grad_disu_upts as it stands (hfx_eles_compute_wall_forces): behind hfxh_case_run that is the gradient of the last RK stage,
 * the reference's pairing.
 * The wall faces are those whose boundary group is a slip, isothermal, adiabatic or dual-consistent slip wall.  The reference's
 * loop also reads run_input.bc_list(-1) for the local faces of a boundary element that belong to no group and may take them for
 * walls; that defect is not reproduced. */
int hfxh_case_CalcForces(hfxh_case *c, double *inv_force, double *vis_force, double *cl, double *cd);
/* The rows of force_files_<step>/cp_<step>_p<rank>.dat: the wall faces in the reference's order (boundary elements ascending, local
 * faces ascending) as ele[n_faces], inter[n_faces], flag[n_faces] (hfx_bc_flag: the label the file prints above a face's rows) and
 * n_points[n_faces]; then, over all faces' points in file order (inside a face the cubature index DESCENDING), pos (n_dims, points)
 * column-major -- calc_pos of the point, evaluated once when the case is made -- and cp, cf (points) of the last
 * hfxh_case_CalcForces (NULL before the first).  Host only but for cp and cf; any pointer may be NULL. */
int hfxh_case_get_wall_points(hfxh_case *c, int *n_faces, const int **ele, const int **inter, const int **flag, const int **n_points,
                              const double **pos, const double **cp, const double **cf);
/* calc_force, area_ref (non-dimensional, as the device gets it), monitor_cp_freq and the reference state as the case holds them:
 * ref[5] = rho_c_ic, u_c_ic, v_c_ic, w_c_ic, p_c_ic.  Any pointer may be NULL */
int hfxh_case_get_calc_force(hfxh_case *c, int *calc_force, double *area_ref, int *monitor_cp_freq, double ref[5]);

#ifdef __cplusplus
}
#endif
#endif
