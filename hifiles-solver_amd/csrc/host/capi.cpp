// capi.cpp -- small extern "C" facade over the host-side mirror so that the Python test and
// bench plumbing (ctypes) can build a case, read its host arrays and drive it.  Declared in
// include/hfx_host.h.
#include "../../../include/hfx_host.h"

#include <cstring>
#include <map>
#include <string>

#include "solver.hpp"

struct hfxh_case
{
  solution S;
  box_mesh mesh;
  std::vector<hfx_inters *> faces;
  std::string err;
  hf_array<double> high_modes_d;
};

static thread_local std::string g_err;
extern "C" const char *hfxh_last_error(void) { return g_err.c_str(); }

static eles *the_eles(hfxh_case *c) { return c->S.n_dims == 3 ? (eles *)&c->S.mesh_eles_hexas : (eles *)&c->S.mesh_eles_quads; }
static int_inters *the_faces(hfxh_case *c) { return &c->S.mesh_int_inters(c->S.n_dims == 3 ? 2 : 0); }

extern "C" int hfxh_case_create(const hfxh_case_desc *d, hfxh_case **out)
{
  if (!d || !out) { g_err = "hfxh_case_create: NULL argument"; return 1; }
  hfxh_case *c = new hfxh_case();
  input &in = c->S.run_input;
  in.equation = 0;
  in.viscous = d->viscous; in.order = d->order;
  in.riemann_solve_type = d->riemann_solve_type; in.vis_riemann_solve_type = 0;
  in.ic_form = d->ic_form; in.adv_type = d->adv_type; in.dt_type = d->dt_type; in.dt = d->dt; in.CFL = d->CFL;
  in.ldg_tau = d->ldg_tau; in.ldg_beta = d->ldg_beta;
  in.upts_type_hexa = in.upts_type_quad = d->upts_type;
  in.vcjh_scheme_hexa = in.vcjh_scheme_quad = d->vcjh_scheme;
  in.eta_hexa = in.eta_quad = d->eta;
  in.gamma = d->gamma; in.prandtl = d->prandtl; in.S_gas = d->S_gas; in.T_gas = d->T_gas; in.R_gas = d->R_gas;
  in.mu_gas = d->mu_gas; in.fix_vis = d->fix_vis;
  in.Mach_free_stream = d->Mach_free_stream; in.L_free_stream = d->L_free_stream;
  in.T_free_stream = d->T_free_stream; in.rho_free_stream = d->rho_free_stream;
  in.Mach_c_ic = d->Mach_c_ic; in.T_c_ic = d->T_c_ic; in.rho_c_ic = d->rho_c_ic;
  in.u_c_ic = d->u_c_ic; in.v_c_ic = d->v_c_ic; in.w_c_ic = d->w_c_ic; in.p_c_ic = d->p_c_ic;
  in.dx_cyclic = in.dy_cyclic = in.dz_cyclic = d->length;
  if (d->p_res >= 2) in.p_res = d->p_res;
  in.LES = d->LES;
  if (d->LES)
  {
    in.SGS_model = d->SGS_model; in.C_s = d->C_s; in.filter_ratio = d->filter_ratio; in.filter_type = d->filter_type;
    if (d->prandtl_t > 0) in.prandtl_t = d->prandtl_t;
  }
  in.over_int = d->over_int; in.over_int_order = d->over_int_order;
  in.shock_cap = d->shock_cap; in.shock_det_field = d->shock_det_field; in.s0 = d->s0;
  if (d->shock_cap)
  {
    in.expf_fac = d->expf_fac; in.expf_order = d->expf_order; in.expf_cutoff = d->expf_cutoff;
  }
  if (d->loc_1d_upts)
  {
    in.loc_1d_upts_override.setup(d->order + 1);
    for (int i = 0; i <= d->order; i++) in.loc_1d_upts_override(i) = d->loc_1d_upts[i];
  }
  in.forcing = d->body_forcing;
  if (d->forcing_area != 0.0) in.forcing_area = d->forcing_area;
  if (d->forcing_mdot0 != 0.0) in.forcing_mdot0 = d->forcing_mdot0;
  if (d->nx_c_ic != 0.0 || d->ny_c_ic != 0.0 || d->nz_c_ic != 0.0)
  {
    in.nx_c_ic = d->nx_c_ic; in.ny_c_ic = d->ny_c_ic; in.nz_c_ic = d->nz_c_ic;
  }
  in.calc_force = d->calc_force;
  if (d->calc_force) /* src/input.cpp:103-107 */
  {
    in.area_ref = d->area_ref;
    in.monitor_cp_freq = d->monitor_cp_freq;
  }
  in.wall_model = d->wall_model;
  if (d->wall_model != 0)
  {
    /* src/wall_model_funcs.cpp:106 (the reference finds out at the first viscous boundary sweep) */
    if (d->wall_model != 1 && d->wall_model != 2) { g_err = "Wall model not implemented!"; delete c; return 1; }
    if (d->prandtl_t > 0) in.prandtl_t = d->prandtl_t;
  }
  if (in.setup_params(g_err)) { delete c; return 1; }
  for (int i = 0; i < d->n_bcs; i++)
  {
    const hfxh_bc_desc &b = d->bcs[i];
    bc_spec s;
    s.flag = b.flag; s.pressure_ramp = b.pressure_ramp;
    s.rho = b.rho; s.u = b.u; s.v = b.v; s.w = b.w; s.p_static = b.p_static; s.T_static = b.T_static;
    s.p_total = b.p_total; s.T_total = b.T_total; s.T_total_given = b.T_total >= 0;
    s.nx = b.nx; s.ny = b.ny; s.nz = b.nz; s.mach = b.mach;
    s.p_ramp_coeff = b.p_ramp_coeff; s.T_ramp_coeff = b.T_ramp_coeff; s.p_total_old = b.p_total_old;
    s.T_total_old = b.T_total_old; s.T_total_old_given = b.T_total_old >= 0;
    s.use_wm = b.use_wm;
    in.bc_specs.push_back(s);
  }
  if (in.read_boundary_param(g_err)) { delete c; return 1; }
  for (int i = 0; i < 6; i++) c->mesh.side_bc[i] = (d->n_bcs > 0) ? d->side_bc[i] : -1;

  c->mesh.dims = d->dims;
  c->S.nproc = d->nproc > 0 ? d->nproc : 1;
  c->S.rank = d->nproc > 0 ? d->rank : 0;
  {
    int r = c->S.rank;
    for (int i = 0; i < 3; i++)
    {
      c->mesh.pgrid[i] = (d->nproc > 0 && d->pgrid[i] > 0 && i < d->dims) ? d->pgrid[i] : 1;
      c->mesh.pcoord[i] = r % c->mesh.pgrid[i];
      r /= c->mesh.pgrid[i];
    }
  }
  for (int i = 0; i < 3; i++) c->mesh.n[i] = d->n[i];
  for (int i = 0; i < 3; i++) c->mesh.self_partition[i] = (i < d->dims) ? d->self_partition[i] : 0;
  c->mesh.length = d->length;
  c->mesh.amp = d->amp;
  if (d->xv)
    c->mesh.xv.assign(d->xv, d->xv + (size_t)c->mesh.nv() * d->dims);
  else
    c->mesh.generate();
  if (GeoPreprocess_box(&c->S, c->mesh)) { g_err = c->S.err; delete c; return 1; }
  if (InitSolution(&c->S)) { g_err = c->S.err; delete c; return 1; }
  *out = c;
  return 0;
}

extern "C" int hfxh_case_destroy(hfxh_case *c)
{
  delete c;
  return 0;
}

extern "C" int hfxh_case_sizes(hfxh_case *c, int sizes[8])
{
  eles *E = the_eles(c);
  sizes[0] = E->n_eles; sizes[1] = E->n_upts_per_ele; sizes[2] = E->n_fpts_per_ele; sizes[3] = E->n_fields;
  sizes[4] = E->n_dims; sizes[5] = E->order; sizes[6] = E->ele_type; sizes[7] = c->S.run_input.n_rk_stages();
  return 0;
}

extern "C" int hfxh_case_params(hfxh_case *c, hfx_params *p)
{
  c->S.run_input.fill(*p);
  return 0;
}

extern "C" int hfxh_case_get_array(hfxh_case *c, const char *name, const double **ptr, int dims[4])
{
  eles *E = the_eles(c);
  std::string n(name);
  hf_array<double> *a = nullptr;
  if (n == "opp_0") a = &E->opp_0;
  else if (n == "opp_3") a = &E->opp_3;
  else if (n == "opp_6") a = &E->opp_6;
  else if (n.rfind("opp_", 0) == 0 && n.size() == 7)
  {
    const int which = n[4] - '0', d = n[6] - '0';
    if (d < 0 || d >= E->n_dims) { g_err = "bad operator dimension"; return 1; }
    if (which == 1) a = &E->opp_1(d);
    else if (which == 2) a = &E->opp_2(d);
    else if (which == 4 && E->viscous) a = &E->opp_4(d);
    else if (which == 5 && E->viscous) a = &E->opp_5(d);
  }
  else if (n == "Jacobian_fpts") a = &E->Jacobian_fpts;
  else if (n == "opp_p") a = &E->opp_p;
  else if (n == "loc_ppts") a = &E->loc_ppts;
  else if (n == "inv_vandermonde") a = &E->inv_vandermonde;
  else if (n == "vandermonde") a = &E->vandermonde;
  else if (n == "exp_filter") a = &E->exp_filter;
  else if (n == "norm_basis_persson") a = &E->norm_basis_persson;
  else if (n == "persson_high_modes" && E->persson_high_modes.get_dim(0) > 0)
  {
    // (an int array: handed out as doubles through this double-typed getter)
    hf_array<int> &hm = E->persson_high_modes;
    c->high_modes_d.setup(hm.get_dim(0));
    for (int i = 0; i < hm.get_dim(0); i++) c->high_modes_d(i) = hm(i);
    a = &c->high_modes_d;
  }
  else if (n == "opp_over_int_cubpts") a = &E->opp_over_int_cubpts;
  else if (n == "over_int_filter") a = &E->over_int_filter;
  else if (n == "filter_upts") a = &E->filter_upts;
  else if (n == "wall_distance" && E->wall_distance.get_dim(0) > 0) a = &E->wall_distance;
  else if (n == "filter_upts_1D") a = &E->filter_upts_1D;
  else if (n == "JGinv_over_int_cubpts") a = &E->JGinv_over_int_cubpts;
  else if (n == "loc_over_int_cubpts") a = &E->loc_over_int_cubpts;
  else if (n == "detjac_upts") a = &E->detjac_upts;
  else if (n == "JGinv_upts") a = &E->JGinv_upts;
  else if (n == "detjac_fpts") a = &E->detjac_fpts;
  else if (n == "JGinv_fpts") a = &E->JGinv_fpts;
  else if (n == "tdA_fpts") a = &E->tdA_fpts;
  else if (n == "norm_fpts") a = &E->norm_fpts;
  else if (n == "pos_upts") a = &E->pos_upts;
  else if (n == "pos_fpts") a = &E->pos_fpts;
  else if (n == "shape") a = &E->shape;
  else if (n == "loc_upts") a = &E->loc_upts;
  else if (n == "tloc_fpts") a = &E->tloc_fpts;
  else if (n == "tnorm_fpts") a = &E->tnorm_fpts;
  else if (n == "loc_1d_upts") a = &E->loc_1d_upts;
  else if (n == "disu_upts0") a = &E->disu_upts(0);
  else if (n == "disu_upts1") a = &E->disu_upts(1);
  else if (n == "div_tconf_upts") a = &E->div_tconf_upts(0);
  else if (n == "grad_disu_upts") a = &E->grad_disu_upts;
  else if (n == "h_ref") a = &E->h_ref;
  // volume cubature: exists once a test case or integral quantities are set
  else if (n == "loc_volume_cubpts" && E->weight_volume_cubpts.get_dim(0) > 0) a = &E->loc_volume_cubpts;
  else if (n == "weight_volume_cubpts" && E->weight_volume_cubpts.get_dim(0) > 0) a = &E->weight_volume_cubpts;
  else if (n == "opp_volume_cubpts" && E->weight_volume_cubpts.get_dim(0) > 0) a = &E->opp_volume_cubpts;
  else if (n == "vol_detjac_vol_cubpts" && E->weight_volume_cubpts.get_dim(0) > 0) a = &E->vol_detjac_vol_cubpts;
  else if (n == "pos_volume_cubpts" && E->pos_volume_cubpts.get_dim(0) > 0) a = &E->pos_volume_cubpts;
  // surface cubature of local face l (body forcing): <name>_<l>
  else if (n.size() > 2 && n[n.size() - 2] == '_' && E->n_cubpts_per_inter.get_dim(0) == E->n_inters_per_ele)
  {
    const int l = n.back() - '0';
    const std::string base = n.substr(0, n.size() - 2);
    if (l >= 0 && l < E->n_inters_per_ele)
    {
      if (base == "opp_inters_cubpts") a = &E->opp_inters_cubpts(l);
      else if (base == "weight_inters_cubpts") a = &E->weight_inters_cubpts(l);
      else if (base == "loc_inters_cubpts") a = &E->loc_inters_cubpts(l);
      else if (base == "tnorm_inters_cubpts") a = &E->tnorm_inters_cubpts(l);
      else if (base == "inter_detjac_inters_cubpts") a = &E->inter_detjac_inters_cubpts(l);
      else if (base == "norm_inters_cubpts") a = &E->norm_inters_cubpts(l);
    }
  }
  if (!a) { g_err = "hfxh_case_get_array: unknown array " + n; return 1; }
  *ptr = a->get_ptr_cpu();
  for (int i = 0; i < 4; i++) dims[i] = a->get_dim(i);
  return 0;
}

extern "C" int hfxh_case_get_faces(hfxh_case *c, const int **L, const int **R, int *n_fpts_per_inter, int *n_inters)
{
  int_inters *I = the_faces(c);
  *L = I->disu_fpts_l.get_ptr_cpu();
  *R = I->disu_fpts_r.get_ptr_cpu();
  *n_fpts_per_inter = I->n_fpts_per_inter;
  *n_inters = I->n_inters;
  return 0;
}

static bdy_inters *the_bdy_faces(hfxh_case *c) { return &c->S.mesh_bdy_inters(c->S.n_dims == 3 ? 2 : 0); }

extern "C" int hfxh_case_get_bdy_faces(hfxh_case *c, const int **L, const int **boundary_id, int *n_fpts_per_inter, int *n_inters)
{
  bdy_inters *B = the_bdy_faces(c);
  *L = B->disu_fpts_l.get_ptr_cpu();
  *boundary_id = B->boundary_id.get_ptr_cpu();
  *n_fpts_per_inter = B->n_fpts_per_inter;
  *n_inters = B->n_inters;
  return 0;
}

extern "C" int hfxh_case_get_wall_model_points(hfxh_case *c, int *wall_model, const int **upt, const double **dist, int *n_inters,
                                               int *n_wall_model_inters)
{
  if (!c) { g_err = "hfxh_case_get_wall_model_points: NULL case"; return 1; }
  bdy_inters *B = the_bdy_faces(c);
  if (wall_model) *wall_model = c->S.run_input.wall_model;
  if (upt) *upt = B->wm_upt.get_ptr_cpu();
  if (dist) *dist = B->wm_dist.get_ptr_cpu();
  if (n_inters) *n_inters = B->n_inters;
  if (n_wall_model_inters) *n_wall_model_inters = B->n_wm_inters;
  return 0;
}

extern "C" int hfxh_case_get_bcs(hfxh_case *c, const hfx_bc **bcs, int *n_bcs, double *R_ref, int *ramp_counter)
{
  input &in = c->S.run_input;
  *bcs = in.bc_list.data();
  *n_bcs = (int)in.bc_list.size();
  *R_ref = in.bc_R_ref();
  *ramp_counter = in.ramp_counter;
  return 0;
}

static mpi_inters *the_mpi_faces(hfxh_case *c) { return &c->S.mesh_mpi_inters(c->S.n_dims == 3 ? 2 : 0); }

extern "C" int hfxh_case_get_mpi_faces(hfxh_case *c, const int **L, const int **Rlut, int *n_fpts_per_inter, int *n_inters,
                                       const int **nout_proc)
{
  mpi_inters *M = the_mpi_faces(c);
  *L = M->disu_fpts_l.get_ptr_cpu();
  *Rlut = M->disu_fpts_r.get_ptr_cpu();
  *n_fpts_per_inter = M->n_fpts_per_inter;
  *n_inters = M->n_inters;
  *nout_proc = M->Nout_proc.get_ptr_cpu();
  return 0;
}

extern "C" int hfxh_case_get_mpi_segments(hfxh_case *c, const int **peer, const int **send_first, const int **recv_first,
                                          const int **count, int *n_seg)
{
  mpi_inters *M = the_mpi_faces(c);
  *peer = M->seg_peer.data(); *send_first = M->seg_send.data(); *recv_first = M->seg_recv.data(); *count = M->seg_count.data();
  *n_seg = (int)M->seg_peer.size();
  return 0;
}

extern "C" int hfxh_case_set_reduce_min(hfxh_case *c, hfxh_reduce_min_cb fn, void *user)
{
  SetReduceMin(&c->S, fn, user);
  return 0;
}

extern "C" int hfxh_case_set_comm(hfxh_case *c, const char *unique_id)
{
  if (SetComm(&c->S, unique_id)) { g_err = c->S.err; return 1; }
  return 0;
}

extern "C" int hfxh_case_time_partitioned(hfxh_case *c, int reps, double ms[8])
{
  if (TimePartitioned(&c->S, reps, ms)) { g_err = c->S.err; return 1; }
  return 0;
}

extern "C" int hfxh_case_set_exchange(hfxh_case *c, hfxh_exchange_cb fn, void *user)
{
  SetExchange(&c->S, fn, user);
  return 0;
}

extern "C" int hfxh_case_mpi_handle(hfxh_case *c, hfx_inters **f)
{
  *f = the_mpi_faces(c)->device();
  return 0;
}

extern "C" int hfxh_case_run_partitioned(hfxh_case *c, int n_steps)
{
  if (RunStepsPartitionedFused(&c->S, n_steps)) { g_err = c->S.err; return 1; }
  return 0;
}

extern "C" int hfxh_case_comm_info(hfxh_case *c, int *nranks, int *rank, int *device, char pci_bus_id[32])
{
  if (CommInfo(&c->S, nranks, rank, device, pci_bus_id)) { g_err = c->S.err; return 1; }
  return 0;
}

extern "C" int hfxh_case_set_deferred(hfxh_case *c, int on)
{
  if (SetDeferred(&c->S, on != 0)) { g_err = c->S.err; return 1; }
  return 0;
}

extern "C" int hfxh_case_to_device(hfxh_case *c, int device)
{
  if (MoveToDevice(&c->S, device)) { g_err = c->S.err; return 1; }
  c->faces.clear();
  for (int i = 0; i < c->S.n_int_inter_types; i++)
    if (c->S.mesh_int_inters(i).device()) c->faces.push_back(c->S.mesh_int_inters(i).device());
  for (int i = 0; i < c->S.n_bdy_inter_types; i++)
    if (c->S.mesh_bdy_inters(i).device()) c->faces.push_back(c->S.mesh_bdy_inters(i).device());
  return 0;
}

extern "C" int hfxh_case_handles(hfxh_case *c, hfx_ctx **ctx, hfx_eles **e, hfx_inters ***faces, int *n_face_blocks)
{
  if (!c->S.ctx) { g_err = "case is not on the device"; return 1; }
  *ctx = c->S.ctx;
  *e = the_eles(c)->device();
  *faces = c->faces.data();
  *n_face_blocks = (int)c->faces.size();
  return 0;
}

extern "C" int hfxh_case_CalcResidual(hfxh_case *c)
{
  CalcResidual(0, 0, &c->S);
  eles *E = the_eles(c);
  if (E->failed()) { g_err = E->last_error(); return 1; }
  if (the_faces(c)->failed()) { g_err = the_faces(c)->last_error(); return 1; }
  if (the_mpi_faces(c)->failed()) { g_err = the_mpi_faces(c)->last_error(); return 1; }
  if (the_bdy_faces(c)->failed()) { g_err = the_bdy_faces(c)->last_error(); return 1; }
  return 0;
}

extern "C" int hfxh_case_run(hfxh_case *c, int n_steps)
{
  if (RunSteps(&c->S, n_steps)) { g_err = c->S.err; return 1; }
  return 0;
}

extern "C" int hfxh_case_write_restart(hfxh_case *c, const char *dir, int file_num)
{
  eles *E = the_eles(c);
  if (c->S.ctx && E->cp_disu_upts_gpu_cpu()) { g_err = E->last_error(); return 1; }
  if (write_restart_ascii(&c->S, dir ? dir : "", file_num)) { g_err = c->S.err; return 1; }
  return 0;
}

extern "C" int hfxh_case_read_restart(hfxh_case *c, const char *dir, int file_num, int n_files)
{
  if (read_restart_ascii(&c->S, dir ? dir : "", file_num, n_files)) { g_err = c->S.err; return 1; }
  eles *E = the_eles(c);
  if (c->S.ctx && hfx_eles_upload(E->device(), HFX_DISU_UPTS0, E->disu_upts(0).get_ptr_cpu())) { g_err = hfx_last_error(); return 1; }
  return 0;
}

extern "C" int hfxh_case_calc_time_step(hfxh_case *c, double *dt)
{
  if (calc_time_step(&c->S)) { g_err = c->S.err; return 1; }
  *dt = c->S.run_input.dt;
  return 0;
}

extern "C" int hfxh_case_sync_host(hfxh_case *c)
{
  eles *E = the_eles(c);
  // the gradient first: with deferred execution a pending stage then runs call by call and leaves every array of the
  // reference behind (asked for the state first it would run fused and keep the gradient on chip)
  // (... unless an earlier request has already made the last stage run fused: the gradient then stays what it was, as
  // hfx_run_steps(..., 3) leaves it)
  int grad_current = 1;
  if (E->viscous && E->device() && hfx_eles_is_current(E->device(), HFX_GRAD_DISU_UPTS, &grad_current)) { g_err = hfx_last_error(); return 1; }
  if (E->viscous && grad_current && E->cp_grad_disu_upts_gpu_cpu()) { g_err = E->last_error(); return 1; }
  if (E->cp_disu_upts_gpu_cpu() || E->cp_div_tconf_upts_gpu_cpu() || E->cp_array_gpu_cpu(HFX_DISU_UPTS1, E->disu_upts(1)))
  {
    g_err = E->last_error();
    return 1;
  }
  return 0;
}

extern "C" int hfxh_case_calc_disu_ppts(hfxh_case *c, const double **out, int dims[3])
{
  eles *E = the_eles(c);
  if (E->calc_disu_ppts_all()) { g_err = E->last_error(); return 1; }
  *out = E->disu_ppts.get_ptr_cpu();
  dims[0] = E->n_ppts_per_ele; dims[1] = E->n_eles; dims[2] = E->n_fields;
  return 0;
}

// ---- time-averaged fields ----------------------------------------------------------------------------------------------
extern "C" int hfxh_case_set_average_fields(hfxh_case *c, int n, const char *const *names)
{
  if (!c || n < 0 || (n > 0 && !names)) { g_err = "hfxh_case_set_average_fields: bad argument"; return 1; }
  std::vector<std::string> v;
  for (int i = 0; i < n; i++) v.push_back(names[i] ? names[i] : "");
  if (c->S.run_input.set_average_fields(v, c->S.n_dims, g_err)) return 1;
  eles *E = the_eles(c);
  if (E->register_average_fields()) { g_err = E->last_error(); return 1; }
  return 0;
}

extern "C" int hfxh_case_get_average_fields(hfxh_case *c, int *n, const char *names[HFX_MAX_AVERAGE_FIELDS])
{
  const input &in = c->S.run_input;
  *n = in.n_average_fields;
  if (names)
    for (int i = 0; i < in.n_average_fields; i++) names[i] = in.average_fields[i].c_str();
  return 0;
}

extern "C" int hfxh_case_get_averages(hfxh_case *c, const double **out, int dims[3])
{
  eles *E = the_eles(c);
  if (c->S.run_input.n_average_fields == 0) { g_err = "hfxh_case_get_averages: the case has no average_fields"; return 1; }
  if (E->cp_disu_average_upts_gpu_cpu()) { g_err = E->last_error(); return 1; }
  *out = E->disu_average_upts.get_ptr_cpu();
  dims[0] = E->n_upts_per_ele; dims[1] = E->n_eles; dims[2] = c->S.run_input.n_average_fields;
  return 0;
}

extern "C" int hfxh_case_calc_time_average_ppts(hfxh_case *c, const double **out, int dims[3])
{
  eles *E = the_eles(c);
  if (c->S.run_input.n_average_fields == 0) { g_err = "hfxh_case_calc_time_average_ppts: the case has no average_fields"; return 1; }
  if (E->calc_time_average_ppts_all()) { g_err = E->last_error(); return 1; }
  *out = E->disu_average_ppts.get_ptr_cpu();
  dims[0] = E->n_ppts_per_ele; dims[1] = E->n_eles; dims[2] = c->S.run_input.n_average_fields;
  return 0;
}

extern "C" int hfxh_case_get_clock(hfxh_case *c, double *time, int *i_steps, double *spinup_time)
{
  if (time) *time = c->S.time;
  if (i_steps) *i_steps = c->S.i_steps;
  if (spinup_time) *spinup_time = c->S.run_input.spinup_time;
  return 0;
}

// ---- exact-solution error norms and integral diagnostics ----------------------------------------------------------------
// the cubature follows run_input: built again (or dropped) on the host, registered again when the case is on the device
static int rebuild_volume_cubature(hfxh_case *c)
{
  eles *E = the_eles(c);
  if (E->set_volume_cubature() || E->register_volume_cubature()) { g_err = E->last_error(); return 1; }
  return 0;
}

extern "C" int hfxh_case_set_test_case(hfxh_case *c, int test_case, int error_norm_type)
{
  if (!c) { g_err = "hfxh_case_set_test_case: NULL case"; return 1; }
  input &in = c->S.run_input;
  const int old_case = in.test_case, old_norm = in.error_norm_type;
  if (in.set_test_case(test_case, error_norm_type, g_err)) return 1;
  if (rebuild_volume_cubature(c) || RegisterExactSolution(&c->S))
  {
    // a refusal leaves the case as it was: what was set before is set, built and registered again
    if (!c->S.err.empty()) { g_err = c->S.err; c->S.err.clear(); }
    const std::string why = g_err;
    in.test_case = old_case;
    in.error_norm_type = old_norm;
    (void)rebuild_volume_cubature(c);
    (void)RegisterExactSolution(&c->S);
    c->S.err.clear();
    g_err = why;
    return 1;
  }
  return 0;
}

extern "C" int hfxh_case_get_test_case(hfxh_case *c, int *test_case, int *error_norm_type, double *u_wall, double *T_wall)
{
  if (!c) { g_err = "hfxh_case_get_test_case: NULL case"; return 1; }
  const input &in = c->S.run_input;
  if (test_case) *test_case = in.test_case;
  if (error_norm_type) *error_norm_type = in.error_norm_type;
  double u = 0.0, T = 0.0;
  if (in.test_case == 5 && in.couette_walls(u, T, g_err)) return 1;
  if (u_wall) *u_wall = u;
  if (T_wall) *T_wall = T;
  return 0;
}

extern "C" int hfxh_case_set_integral_quantities(hfxh_case *c, int n, const char *const *names)
{
  if (!c || n < 0 || (n > 0 && !names)) { g_err = "hfxh_case_set_integral_quantities: bad argument"; return 1; }
  std::vector<std::string> v;
  for (int i = 0; i < n; i++) v.push_back(names[i] ? names[i] : "");
  input &in = c->S.run_input;
  const std::vector<std::string> old = in.integral_quantities;
  if (in.set_integral_quantities(v, g_err)) return 1;
  if (rebuild_volume_cubature(c)) return 1;
  if (RegisterIntegralMonitor(&c->S))
  {
    // a refusal (a gradient quantity on an inviscid case with a history) leaves the case as it was
    const std::string why = c->S.err;
    std::string ignore;
    in.set_integral_quantities(old, ignore);
    (void)rebuild_volume_cubature(c);
    (void)RegisterIntegralMonitor(&c->S);
    c->S.err.clear();
    g_err = why;
    return 1;
  }
  return 0;
}

extern "C" int hfxh_case_set_monitor_res_freq(hfxh_case *c, int monitor_res_freq, int capacity)
{
  if (!c) { g_err = "hfxh_case_set_monitor_res_freq: NULL case"; return 1; }
  input &in = c->S.run_input;
  const int old_freq = in.monitor_res_freq, old_capacity = in.integral_capacity;
  if (in.set_monitor_res_freq(monitor_res_freq, capacity, g_err)) return 1;
  if (RegisterIntegralMonitor(&c->S))
  {
    const std::string why = c->S.err;
    in.monitor_res_freq = old_freq;
    in.integral_capacity = old_capacity;
    (void)RegisterIntegralMonitor(&c->S);
    c->S.err.clear();
    g_err = why;
    return 1;
  }
  return 0;
}

extern "C" int hfxh_case_get_monitor_res_freq(hfxh_case *c, int *monitor_res_freq, int *capacity)
{
  if (!c) { g_err = "hfxh_case_get_monitor_res_freq: NULL case"; return 1; }
  if (monitor_res_freq) *monitor_res_freq = c->S.run_input.monitor_res_freq;
  if (capacity) *capacity = c->S.run_input.integral_capacity;
  return 0;
}

extern "C" int hfxh_case_sample_integral_quantities(hfxh_case *c)
{
  if (!c) { g_err = "hfxh_case_sample_integral_quantities: NULL case"; return 1; }
  if (!c->S.run_input.integral_monitor_on()) { g_err = "hfxh_case_sample_integral_quantities: the case has no integral monitor (integral quantities and a capacity)"; return 1; }
  if (SampleIntegralQuantities(&c->S, true)) { g_err = c->S.err; c->S.err.clear(); return 1; }
  return 0;
}

extern "C" int hfxh_case_integral_count(hfxh_case *c, int *n_samples)
{
  if (!c || !n_samples) { g_err = "hfxh_case_integral_count: NULL argument"; return 1; }
  if (IntegralCount(&c->S, n_samples)) { g_err = c->S.err; c->S.err.clear(); return 1; }
  return 0;
}

extern "C" int hfxh_case_read_integral_history(hfxh_case *c, int max_samples, double *times, int *steps, double *values, int *n_samples)
{
  if (!c || !n_samples) { g_err = "hfxh_case_read_integral_history: NULL argument"; return 1; }
  if (ReadIntegralHistory(&c->S, max_samples, times, steps, values, n_samples)) { g_err = c->S.err; c->S.err.clear(); return 1; }
  return 0;
}

// ---- the history monitor: residual and force columns of history.plt ---------------------------------------------------------
extern "C" int hfxh_case_set_history(hfxh_case *c, int res_norm_type, int capacity)
{
  if (!c) { g_err = "hfxh_case_set_history: NULL case"; return 1; }
  input &in = c->S.run_input;
  const int old_norm = in.res_norm_type, old_capacity = in.history_capacity;
  if (in.set_history(res_norm_type, capacity, g_err)) return 1;
  if (RegisterHistoryMonitor(&c->S))
  {
    const std::string why = c->S.err;
    in.res_norm_type = old_norm;
    in.history_capacity = old_capacity;
    (void)RegisterHistoryMonitor(&c->S);
    c->S.err.clear();
    g_err = why;
    return 1;
  }
  return 0;
}

extern "C" int hfxh_case_get_history(hfxh_case *c, int *res_norm_type, int *capacity, int *n_cols)
{
  if (!c) { g_err = "hfxh_case_get_history: NULL case"; return 1; }
  if (res_norm_type) *res_norm_type = c->S.run_input.res_norm_type;
  if (capacity) *capacity = c->S.run_input.history_capacity;
  if (n_cols) *n_cols = HistoryColumns(&c->S);
  return 0;
}

extern "C" int hfxh_norm_residual(int res_norm_type, int n_fields, const double *sum, long n_upts, double *norm_residual)
{
  if (!sum || !norm_residual || n_fields < 0) { g_err = "hfxh_norm_residual: bad argument"; return 1; }
  return NormResidual(res_norm_type, n_fields, sum, n_upts, norm_residual, g_err);
}

extern "C" int hfxh_case_CalcNormResidual(hfxh_case *c, double *norm_residual)
{
  if (!c || !norm_residual) { g_err = "hfxh_case_CalcNormResidual: NULL argument"; return 1; }
  if (CalcNormResidual(&c->S, norm_residual)) { g_err = c->S.err; c->S.err.clear(); return 1; }
  return 0;
}

extern "C" int hfxh_case_sample_history(hfxh_case *c)
{
  if (!c) { g_err = "hfxh_case_sample_history: NULL case"; return 1; }
  if (!c->S.run_input.history_monitor_on()) { g_err = "hfxh_case_sample_history: the case has no history monitor (a capacity)"; return 1; }
  if (SampleHistory(&c->S, true)) { g_err = c->S.err; c->S.err.clear(); return 1; }
  return 0;
}

extern "C" int hfxh_case_history_count(hfxh_case *c, int *n_rows)
{
  if (!c || !n_rows) { g_err = "hfxh_case_history_count: NULL argument"; return 1; }
  if (HistoryCount(&c->S, n_rows)) { g_err = c->S.err; c->S.err.clear(); return 1; }
  return 0;
}

extern "C" int hfxh_case_read_history(hfxh_case *c, int max_rows, int *steps, double *rows, int *n_cols, int *n_rows)
{
  if (!c || !n_rows || (max_rows > 0 && (!steps || !rows))) { g_err = "hfxh_case_read_history: NULL argument"; return 1; }
  if (ReadHistory(&c->S, max_rows, steps, rows, n_cols, n_rows)) { g_err = c->S.err; c->S.err.clear(); return 1; }
  return 0;
}

// ---- the plot monitor: the rows of the plot file ----------------------------------------------------------------------------
extern "C" int hfxh_case_set_diagnostic_fields(hfxh_case *c, int n, const char *const *names)
{
  if (!c || n < 0 || (n > 0 && !names)) { g_err = "hfxh_case_set_diagnostic_fields: bad argument"; return 1; }
  std::vector<std::string> v;
  for (int i = 0; i < n; i++) v.push_back(names[i] ? names[i] : "");
  input &in = c->S.run_input;
  const std::vector<std::string> old = in.diagnostic_fields;
  if (in.set_diagnostic_fields(v, g_err)) return 1;
  if (RegisterPlotMonitor(&c->S))
  {
    const std::string why = c->S.err;
    std::string ignored;
    (void)in.set_diagnostic_fields(old, ignored);
    (void)RegisterPlotMonitor(&c->S);
    c->S.err.clear();
    g_err = why;
    return 1;
  }
  return 0;
}

extern "C" int hfxh_case_set_plot(hfxh_case *c, int plot_freq, int capacity)
{
  if (!c) { g_err = "hfxh_case_set_plot: NULL case"; return 1; }
  input &in = c->S.run_input;
  const int old_freq = in.plot_freq, old_capacity = in.plot_capacity;
  if (in.set_plot(plot_freq, capacity, g_err)) return 1;
  if (RegisterPlotMonitor(&c->S))
  {
    const std::string why = c->S.err;
    in.plot_freq = old_freq;
    in.plot_capacity = old_capacity;
    (void)RegisterPlotMonitor(&c->S);
    c->S.err.clear();
    g_err = why;
    return 1;
  }
  return 0;
}

extern "C" int hfxh_case_get_plot(hfxh_case *c, int *plot_freq, int *capacity, int *n_cols, long *n_points)
{
  if (!c) { g_err = "hfxh_case_get_plot: NULL case"; return 1; }
  if (plot_freq) *plot_freq = c->S.run_input.plot_freq;
  if (capacity) *capacity = c->S.run_input.plot_capacity;
  if (n_cols) *n_cols = PlotColumns(&c->S);
  if (n_points) *n_points = PlotPoints(&c->S);
  return 0;
}

extern "C" int hfxh_case_sample_plot(hfxh_case *c)
{
  if (!c) { g_err = "hfxh_case_sample_plot: NULL case"; return 1; }
  if (!c->S.run_input.plot_monitor_on()) { g_err = "hfxh_case_sample_plot: the case has no plot monitor (a capacity)"; return 1; }
  if (SamplePlot(&c->S, true)) { g_err = c->S.err; c->S.err.clear(); return 1; }
  return 0;
}

extern "C" int hfxh_case_plot_count(hfxh_case *c, int *n_snapshots)
{
  if (!c || !n_snapshots) { g_err = "hfxh_case_plot_count: NULL argument"; return 1; }
  if (PlotCount(&c->S, n_snapshots)) { g_err = c->S.err; c->S.err.clear(); return 1; }
  return 0;
}

extern "C" int hfxh_case_read_plot_rows(hfxh_case *c, int max_snapshots, double *times, int *steps, double *rows, int *n_snapshots)
{
  if (!c || !n_snapshots || (max_snapshots > 0 && (!times || !steps || !rows))) { g_err = "hfxh_case_read_plot_rows: NULL argument"; return 1; }
  if (ReadPlotRows(&c->S, max_snapshots, times, steps, rows, n_snapshots)) { g_err = c->S.err; c->S.err.clear(); return 1; }
  return 0;
}

extern "C" int hfxh_case_compute_error(hfxh_case *c, double *error)
{
  if (!c || !error) { g_err = "hfxh_case_compute_error: NULL argument"; return 1; }
  if (ComputeError(&c->S, error)) { g_err = c->S.err; c->S.err.clear(); return 1; }
  return 0;
}

extern "C" int hfxh_case_CalcIntegralQuantities(hfxh_case *c, double *integral_quantities)
{
  if (!c || !integral_quantities) { g_err = "hfxh_case_CalcIntegralQuantities: NULL argument"; return 1; }
  if (CalcIntegralQuantities(&c->S, integral_quantities)) { g_err = c->S.err; c->S.err.clear(); return 1; }
  return 0;
}

// ---- point probes --------------------------------------------------------------------------------------------------------
static int locate_points(eles *E, int n, const double *positions, int *p2c, double *loc)
{
  hf_array<double> pos(E->n_dims), l(E->n_dims);
  for (int i = 0; i < n; i++)
  {
    for (int d = 0; d < E->n_dims; d++) pos(d) = positions[d + (size_t)E->n_dims * i];
    p2c[i] = E->calc_p2c(pos);
    if (p2c[i] == -2) { g_err = E->probe_error; return 1; }
    for (int d = 0; d < E->n_dims; d++) loc[d + (size_t)E->n_dims * i] = 0.0;
    if (p2c[i] < 0) continue;
    if (E->pos_to_loc(pos, p2c[i], l)) { g_err = E->probe_error; return 1; }
    for (int d = 0; d < E->n_dims; d++) loc[d + (size_t)E->n_dims * i] = l(d);
  }
  return 0;
}

static int loc_to_pos(eles *E, int n, const int *ele, const double *loc, double *positions)
{
  hf_array<double> pos(E->n_dims), l(E->n_dims);
  for (int i = 0; i < n; i++)
  {
    if (ele[i] < 0 || ele[i] >= E->n_eles) { g_err = "calc_pos: element out of range"; return 1; }
    for (int d = 0; d < E->n_dims; d++) l(d) = loc[d + (size_t)E->n_dims * i];
    E->calc_pos_probe(l, ele[i], pos);
    for (int d = 0; d < E->n_dims; d++) positions[d + (size_t)E->n_dims * i] = pos(d);
  }
  return 0;
}

static int newton_in_element(eles *E, int ele, const double *position, double *loc)
{
  if (ele < 0 || ele >= E->n_eles) { g_err = "pos_to_loc: element out of range"; return 1; }
  hf_array<double> pos(E->n_dims), l(E->n_dims);
  for (int d = 0; d < E->n_dims; d++) pos(d) = position[d];
  if (E->pos_to_loc(pos, ele, l)) { g_err = E->probe_error; return 1; }
  for (int d = 0; d < E->n_dims; d++) loc[d] = l(d);
  return 0;
}

static int opp_probe_rows(eles *E, int n, const double *loc, double *opp_probe)
{
  hf_array<double> l(E->n_dims);
  for (int i = 0; i < n; i++)
  {
    for (int d = 0; d < E->n_dims; d++) l(d) = loc[d + (size_t)E->n_dims * i];
    E->set_opp_probe(l);
    for (int k = 0; k < E->n_upts_per_ele; k++) opp_probe[k + (size_t)E->n_upts_per_ele * i] = E->opp_probe(k);
  }
  return 0;
}

extern "C" int hfxh_case_locate(hfxh_case *c, int n, const double *positions, int *p2c, double *loc) { return locate_points(the_eles(c), n, positions, p2c, loc); }
extern "C" int hfxh_case_calc_pos(hfxh_case *c, int n, const int *ele, const double *loc, double *positions) { return loc_to_pos(the_eles(c), n, ele, loc, positions); }
extern "C" int hfxh_case_pos_to_loc(hfxh_case *c, int ele, const double *position, double *loc) { return newton_in_element(the_eles(c), ele, position, loc); }
extern "C" int hfxh_case_opp_probe(hfxh_case *c, int n, const double *loc, double *opp_probe) { return opp_probe_rows(the_eles(c), n, loc, opp_probe); }

extern "C" int hfxh_case_set_probes(hfxh_case *c, int n, const double *positions, int n_fields, const char *const *names, int probe_freq,
                                    int capacity)
{
  if (!c || n < 0 || (n > 0 && !positions) || n_fields < 0 || (n_fields > 0 && !names)) { g_err = "hfxh_case_set_probes: bad argument"; return 1; }
  std::vector<std::string> v;
  for (int i = 0; i < n_fields; i++) v.push_back(names[i] ? names[i] : "");
  input check; // (the names are checked on a scratch input first: a refusal leaves the case as it was)
  if (check.set_probe_fields(v, c->S.n_dims, probe_freq, capacity, g_err)) return 1;
  eles *E = the_eles(c);
  if (E->locate_probes(n_fields ? n : 0, positions)) { g_err = E->probe_error; return 1; }
  c->S.run_input.set_probe_fields(v, c->S.n_dims, probe_freq, capacity, g_err);
  if (RegisterProbeFields(&c->S)) { g_err = c->S.err; c->S.err.clear(); return 1; }
  if (E->register_probes()) { g_err = E->last_error(); return 1; }
  return 0;
}

extern "C" int hfxh_case_get_probes(hfxh_case *c, int *n_located, const int **p2c, const int **p2t, const double **loc_probe,
                                    const int **global_index)
{
  eles *E = the_eles(c);
  static thread_local std::vector<int> type;
  type.assign(E->probe_p2c.size(), E->ele_type); // run_probe.p2t: the element class of each probe (one class per case)
  if (n_located) *n_located = (int)E->probe_p2c.size();
  if (p2c) *p2c = E->probe_p2c.data();
  if (p2t) *p2t = type.data();
  if (loc_probe) *loc_probe = E->probe_loc.data();
  if (global_index) *global_index = E->probe_global.data();
  return 0;
}

extern "C" int hfxh_case_sample_probes(hfxh_case *c)
{
  eles *E = the_eles(c);
  if (c->S.run_input.n_probe_fields == 0) { g_err = "hfxh_case_sample_probes: the case has no probes"; return 1; }
  if (!E->device()) { g_err = "case is not on the device"; return 1; }
  if (hfx_eles_sample_probes(E->device(), c->S.time, c->S.i_steps)) { g_err = hfx_last_error(); return 1; }
  return 0;
}

extern "C" int hfxh_case_probe_count(hfxh_case *c, int *n_samples, int *n_probes)
{
  eles *E = the_eles(c);
  if (!E->device()) { g_err = "case is not on the device"; return 1; }
  if (hfx_eles_probe_count(E->device(), n_samples, n_probes)) { g_err = hfx_last_error(); return 1; }
  return 0;
}

extern "C" int hfxh_case_read_probes(hfxh_case *c, int dimensional, int max_samples, double *times, int *steps, double *values,
                                     int *n_samples)
{
  eles *E = the_eles(c);
  const input &in = c->S.run_input;
  if (!E->device()) { g_err = "case is not on the device"; return 1; }
  if (hfx_eles_read_probes(E->device(), max_samples, times, steps, values, n_samples)) { g_err = hfx_last_error(); return 1; }
  if (!dimensional || !in.viscous) return 0; /* src/output.cpp:1475-1535: the reference factors of a viscous run */
  const int nf = in.n_probe_fields;
  const size_t np = E->probe_p2c.size();
  for (int s = 0; s < *n_samples; s++) times[s] *= in.time_ref;
  for (int f = 0; f < nf; f++)
  {
    const int code = in.probe_code(f);
    const double scale = code == HFX_PROBE_RHO ? in.rho_ref : code == HFX_PROBE_E ? in.uvw_ref * in.uvw_ref : code == HFX_PROBE_P ? in.p_ref : in.uvw_ref;
    for (size_t i = 0; i < np * (size_t)*n_samples; i++) values[f + (size_t)nf * i] *= scale;
  }
  return 0;
}

extern "C" int hfxh_case_ref_values(hfxh_case *c, double ref[5])
{
  const input &in = c->S.run_input;
  ref[0] = in.rho_ref; ref[1] = in.uvw_ref; ref[2] = in.p_ref; ref[3] = in.time_ref; ref[4] = in.viscous;
  return 0;
}

// ---- mass-flux body force ------------------------------------------------------------------------------------------------
extern "C" int hfxh_case_get_forcing(hfxh_case *c, int *body_forcing, double *forcing_area, double *forcing_mdot0)
{
  const input &in = c->S.run_input;
  if (body_forcing) *body_forcing = in.forcing;
  if (forcing_area) *forcing_area = in.forcing_area;
  if (forcing_mdot0) *forcing_mdot0 = in.forcing_mdot0;
  return 0;
}

extern "C" int hfxh_case_set_forcing(hfxh_case *c, double forcing_area, double forcing_mdot0)
{
  input &in = c->S.run_input;
  if (in.forcing != 1 || c->S.n_dims != 3) { g_err = "hfxh_case_set_forcing: the case was not made with body_forcing 1 in three dimensions"; return 1; }
  in.forcing_area = forcing_area;
  in.forcing_mdot0 = forcing_mdot0;
  eles *E = the_eles(c);
  if (E->register_body_force()) { g_err = E->last_error(); return 1; }
  return 0;
}

extern "C" int hfxh_case_set_reduce_sum(hfxh_case *c, hfxh_reduce_sum_cb fn, void *user)
{
  SetReduceSum(&c->S, fn, user);
  return 0;
}

extern "C" int hfxh_case_get_inflow_faces(hfxh_case *c, const int **ele, const int **inter, int *n_faces)
{
  eles *E = the_eles(c);
  *ele = E->inflow_ele.data();
  *inter = E->inflow_inter.data();
  *n_faces = (int)E->inflow_ele.size();
  return 0;
}

extern "C" int hfxh_case_body_force_state(hfxh_case *c, double *mass_flux, double *ubulk, double *body_force_x, double accumulated[2],
                                          double integral[2], long *n_steps)
{
  eles *E = the_eles(c);
  if (!E->device()) { g_err = "case is not on the device"; return 1; }
  if (hfx_eles_body_force_state(E->device(), mass_flux, ubulk, body_force_x, accumulated, integral, n_steps)) { g_err = hfx_last_error(); return 1; }
  return 0;
}

extern "C" int hfxh_case_body_force_history(hfxh_case *c, int max_rows, double *rows, int *n_rows)
{
  eles *E = the_eles(c);
  if (!E->device()) { g_err = "case is not on the device"; return 1; }
  if (hfx_eles_body_force_history(E->device(), max_rows, rows, n_rows)) { g_err = hfx_last_error(); return 1; }
  return 0;
}

// ---- wall forces ---------------------------------------------------------------------------------------------------------
extern "C" int hfxh_case_CalcForces(hfxh_case *c, double *inv_force, double *vis_force, double *cl, double *cd)
{
  if (!c || !inv_force || !vis_force || !cl || !cd) { g_err = "hfxh_case_CalcForces: NULL argument"; return 1; }
  if (CalcForces(&c->S, inv_force, vis_force, cl, cd)) { g_err = c->S.err; c->S.err.clear(); return 1; }
  return 0;
}

extern "C" int hfxh_case_get_wall_points(hfxh_case *c, int *n_faces, const int **ele, const int **inter, const int **flag,
                                         const int **n_points, const double **pos, const double **cp, const double **cf)
{
  if (!c) { g_err = "hfxh_case_get_wall_points: NULL case"; return 1; }
  if (!c->S.run_input.calc_force) { g_err = "hfxh_case_get_wall_points: the case was not made with calc_force"; return 1; }
  eles *E = the_eles(c);
  if (n_faces) *n_faces = (int)E->wall_ele.size();
  if (ele) *ele = E->wall_ele.data();
  if (inter) *inter = E->wall_inter.data();
  if (flag) *flag = E->wall_flag.data();
  if (n_points) *n_points = E->wall_n_points.data();
  if (pos) *pos = E->wall_pos.data();
  if (cp) *cp = E->wall_cp.empty() ? nullptr : E->wall_cp.data();
  if (cf) *cf = E->wall_cf.empty() ? nullptr : E->wall_cf.data();
  return 0;
}

extern "C" int hfxh_case_get_calc_force(hfxh_case *c, int *calc_force, double *area_ref, int *monitor_cp_freq, double ref[5])
{
  if (!c) { g_err = "hfxh_case_get_calc_force: NULL case"; return 1; }
  const input &in = c->S.run_input;
  if (calc_force) *calc_force = in.calc_force;
  if (area_ref) *area_ref = in.area_ref;
  if (monitor_cp_freq) *monitor_cp_freq = in.monitor_cp_freq;
  if (ref) { ref[0] = in.rho_c_ic; ref[1] = in.u_c_ic; ref[2] = in.v_c_ic; ref[3] = in.w_c_ic; ref[4] = in.p_c_ic; }
  return 0;
}


// ---- tetrahedra / prisms as producers of operators and metrics -------------------------------------------------------
struct hfxh_simplex
{
  input in;
  eles *E = nullptr;
  hf_array<double> high_modes_d;
  ~hfxh_simplex() { delete E; }
};

extern "C" int hfxh_simplex_create(int ele_type, int order, int viscous, int n_eles, const double *shape, const double *loc_1d_upts,
                                   hfxh_simplex **out)
{
  return hfxh_simplex_create_vcjh(ele_type, order, viscous, n_eles, shape, loc_1d_upts, 1, 0.0, out);
}

extern "C" int hfxh_simplex_create_vcjh(int ele_type, int order, int viscous, int n_eles, const double *shape, const double *loc_1d_upts,
                                        int vcjh_scheme, double c, hfxh_simplex **out)
{
  hfxh_simplex_keys k{};
  k.vcjh_scheme = vcjh_scheme; k.c = c; k.SGS_model = -1;
  return hfxh_simplex_create_keys(ele_type, order, viscous, n_eles, 0, shape, loc_1d_upts, &k, out);
}

extern "C" int hfxh_simplex_create_keys(int ele_type, int order, int viscous, int n_eles, int n_spts, const double *shape,
                                        const double *loc_1d_upts, const hfxh_simplex_keys *keys, hfxh_simplex **out)
{
  if (!keys) { g_err = "hfxh_simplex_create_keys: NULL keys"; return 1; }
  const int vcjh_scheme = keys->vcjh_scheme, SGS_model = keys->SGS_model, filter_type = keys->filter_type;
  const double c = keys->c, filter_ratio = keys->filter_ratio;
  if (!out || !shape || n_eles <= 0) { g_err = "hfxh_simplex_create: bad argument"; return 1; }
  if (ele_type != 2 && ele_type != 3) { g_err = "hfxh_simplex_create: ele_type must be 2 (tetrahedra) or 3 (prisms)"; return 1; }
  hfxh_simplex *s = new hfxh_simplex();
  s->in.equation = 0;
  s->in.order = order;
  s->in.viscous = viscous;
  s->in.vcjh_scheme_tet = s->in.vcjh_scheme_tri = vcjh_scheme;
  s->in.c_tet = s->in.c_tri = c;
  if (SGS_model >= 0)
  {
    s->in.LES = 1;
    s->in.SGS_model = SGS_model;
    s->in.filter_type = filter_type;
    s->in.filter_ratio = filter_ratio;
  }
  if (keys->shock_cap)
  {
    s->in.shock_cap = keys->shock_cap;
    s->in.expf_fac = keys->expf_fac; s->in.expf_order = keys->expf_order; s->in.expf_cutoff = keys->expf_cutoff;
  }
  if (loc_1d_upts)
  {
    s->in.loc_1d_upts_override.setup(order + 1);
    for (int i = 0; i <= order; i++) s->in.loc_1d_upts_override(i) = loc_1d_upts[i];
  }
  s->E = (ele_type == 2) ? (eles *)new eles_tets() : (eles *)new eles_pris();
  const int ns = n_spts > 0 ? n_spts : ((ele_type == 2) ? 4 : 6);
  if (ele_type == 2 ? (ns != 4 && ns != 10) : (ns != 6 && ns != 15))
  {
    g_err = "hfxh_simplex_create: shape nodes per element must be 4 or 10 (tetrahedra), 6 or 15 (prisms)";
    delete s;
    return 1;
  }
  if (s->E->setup(n_eles, ns, &s->in)) { g_err = s->E->last_error(); delete s; return 1; }
  hf_array<double> pos(3);
  for (int e = 0; e < n_eles; e++)
    for (int k = 0; k < ns; k++)
    {
      for (int d = 0; d < 3; d++) pos(d) = shape[d + 3 * (k + (size_t)ns * e)];
      s->E->set_shape_node(k, e, pos);
    }
  if (s->E->set_transforms()) { g_err = s->E->last_error(); delete s; return 1; }
  *out = s;
  return 0;
}

extern "C" int hfxh_simplex_get_array(hfxh_simplex *s, const char *name, const double **ptr, int dims[4])
{
  eles *E = s->E;
  std::string n(name);
  hf_array<double> *a = nullptr;
  if (n == "opp_0") a = &E->opp_0;
  else if (n == "opp_3") a = &E->opp_3;
  else if (n == "opp_6" && E->viscous) a = &E->opp_6;
  else if (n.rfind("opp_", 0) == 0 && n.size() == 7)
  {
    const int which = n[4] - '0', d = n[6] - '0';
    if (d < 0 || d >= E->n_dims) { g_err = "bad operator dimension"; return 1; }
    if (which == 1) a = &E->opp_1(d);
    else if (which == 2) a = &E->opp_2(d);
    else if (which == 4 && E->viscous) a = &E->opp_4(d);
    else if (which == 5 && E->viscous) a = &E->opp_5(d);
  }
  else if (n == "loc_upts") a = &E->loc_upts;
  else if (n == "tloc_fpts") a = &E->tloc_fpts;
  else if (n == "tnorm_fpts") a = &E->tnorm_fpts;
  else if (n == "detjac_upts") a = &E->detjac_upts;
  else if (n == "JGinv_upts") a = &E->JGinv_upts;
  else if (n == "detjac_fpts") a = &E->detjac_fpts;
  else if (n == "JGinv_fpts") a = &E->JGinv_fpts;
  else if (n == "tdA_fpts") a = &E->tdA_fpts;
  else if (n == "norm_fpts") a = &E->norm_fpts;
  else if (n == "pos_upts") a = &E->pos_upts;
  else if (n == "pos_fpts") a = &E->pos_fpts;
  else if (n == "filter_upts" && E->filter_upts.get_dim(0) > 0) a = &E->filter_upts;
  else if (n == "h_ref")
  {
    for (int i = 0; i < E->n_eles; i++) E->h_ref(i) = E->calc_h_ref_specific(i);
    a = &E->h_ref;
  }
  else if (n == "Jacobian_fpts" && E->Jacobian_fpts.get_dim(0) > 0) a = &E->Jacobian_fpts;
  else if (n == "inv_vandermonde" && E->inv_vandermonde.get_dim(0) > 0) a = &E->inv_vandermonde;
  else if (n == "exp_filter" && E->exp_filter.get_dim(0) > 0) a = &E->exp_filter;
  else if (n == "norm_basis_persson" && E->norm_basis_persson.get_dim(0) > 0) a = &E->norm_basis_persson;
  else if (n == "persson_high_modes" && E->persson_high_modes.get_dim(0) > 0)
  {
    // (an int array: handed out as doubles through this double-typed getter)
    hf_array<int> &hm = E->persson_high_modes;
    s->high_modes_d.setup(hm.get_dim(0));
    for (int i = 0; i < hm.get_dim(0); i++) s->high_modes_d(i) = hm(i);
    a = &s->high_modes_d;
  }
  if (!a) { g_err = "hfxh_simplex_get_array: unknown array " + n; return 1; }
  *ptr = a->get_ptr_cpu();
  for (int i = 0; i < 4; i++) dims[i] = a->get_dim(i);
  return 0;
}

extern "C" int hfxh_simplex_locate(hfxh_simplex *s, int n, const double *positions, int *p2c, double *loc) { return locate_points(s->E, n, positions, p2c, loc); }
extern "C" int hfxh_simplex_calc_pos(hfxh_simplex *s, int n, const int *ele, const double *loc, double *positions) { return loc_to_pos(s->E, n, ele, loc, positions); }
extern "C" int hfxh_simplex_pos_to_loc(hfxh_simplex *s, int ele, const double *position, double *loc) { return newton_in_element(s->E, ele, position, loc); }
extern "C" int hfxh_simplex_opp_probe(hfxh_simplex *s, int n, const double *loc, double *opp_probe) { return opp_probe_rows(s->E, n, loc, opp_probe); }

extern "C" int hfxh_simplex_destroy(hfxh_simplex *s)
{
  delete s;
  return 0;
}
