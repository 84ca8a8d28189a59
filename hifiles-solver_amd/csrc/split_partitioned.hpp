// split_partitioned.hpp -- the steps of a split fused stage on a PARTITIONED block (PartitionedSplit, split_common.hpp): interior
// pairs by the pairwise kernels, partition faces by the one-sided kernels of kernels_mpi.hpp.  hfx_stage_partitioned (hfx.hip) and
// partitioned_stage (comm.hip) put them in order and own the exchanges.  Included at the end of fused_hex.hip (it drives that
// file's launchers).
#pragma once

// one of the one-sided partition-face kernels on one block, on stream `st`.  sgs_ref: the SGS flux at the flux points is in
// reference space (the split variant 2 keeps sgsf_fpts so: the kernels take it to physical space; variant 3: the SGS flux is part
// of the projected flux Fn the kernels move anyway).  The arguments are filled at every launch: pack_solution behind the update
// packs the NEW state, e->arr[HFX_DISU_FPTS] as it is then
template <int ND>
static int mpi_launch(hfx_eles *e, hfx_inters *f, MpiKernel k, bool sgs_ref, hipStream_t st, const double *fn_override = nullptr)
{
  if (f->n_inters == 0) return 0;
  MpiArgs a{};
  a.npairs = (long)f->n_inters * f->n_fpts_per_inter;
  a.nfpi = f->n_fpts_per_inter;
  a.L = f->L; a.Rlut = f->R;
  a.plane = (long)e->n_fpts * e->n_eles;
  a.disu = e->arr[HFX_DISU_FPTS]; a.grad = e->arr[HFX_GRAD_DISU_FPTS];
  a.norm = e->norm_fpts; a.tdA = e->tdA_fpts;
  a.tconf = e->arr[HFX_NORM_TCONF_FPTS];
  a.delta = (k == MpiKernel::common_invflux) ? nullptr : e->arr[HFX_DELTA_DISU_FPTS];
  a.out_disu = f->out_disu; a.out_grad = f->out_grad; a.in_disu = f->in_disu; a.in_grad = f->in_grad;
  a.fn = fn_override ? fn_override : (e->fused ? e->fused->fn_fpts : nullptr);
  a.P = e->ctx->phys();
  if (e->les_ready && sgs_ref)
  {
    if (hfx_mpi_sgsf_buffers_internal(f)) return 1;
    a.sgsf = e->arr[HFX_SGSF_FPTS]; a.jac_fpts = e->Jacobian_fpts; a.detjac_fpts = e->detjac_fpts;
    a.out_sgsf = f->out_sgsf; a.in_sgsf = f->in_sgsf; a.sgs_ref = 1;
  }
  const dim3 g((unsigned)((a.npairs + 255) / 256)), b(256);
  switch (k)
  {
  case MpiKernel::pack_solution: hipLaunchKernelGGL(mpi_pack_disu_kernel<ND>, g, b, 0, st, a); break;
  case MpiKernel::ldg_delta: hipLaunchKernelGGL(mpi_delta_kernel<ND>, g, b, 0, st, a); break;
  case MpiKernel::pack_gradient: hipLaunchKernelGGL(mpi_pack_grad_kernel<ND>, g, b, 0, st, a); break;
  case MpiKernel::common_invflux: hipLaunchKernelGGL((mpi_common_invflux_kernel<ND, true>), g, b, 0, st, a); break;
  case MpiKernel::common_viscflux: hipLaunchKernelGGL((mpi_common_viscflux_kernel<ND, true>), g, b, 0, st, a); break;
  case MpiKernel::pack_projected_flux: hipLaunchKernelGGL(mpi_pack_fn_kernel<ND>, g, b, 0, st, a); break;
  case MpiKernel::common_flux_projected: hipLaunchKernelGGL(mpi_common_flux2_kernel<ND>, g, b, 0, st, a); break;
  case MpiKernel::pack_sgs_flux: hipLaunchKernelGGL(mpi_pack_sgsf_kernel<ND>, g, b, 0, st, a); break;
  }
  HFX_HIP(hipGetLastError());
  return 0;
}

// the one-sided partition-face kernels for a block of the general fused stage (fn: that block's projected flux) on stream `st`
// (NULL: the compute stream).  Triangles take the two-dimensional instantiations (no closure there: no SGS buffers).
// (sgs_ref as the SPLIT plan of the block's fused mode would have it: it decides whether a block with a closure gets SGS buffers)
int mpi_launch_general(hfx_eles *e, hfx_inters *f, MpiKernel k, const double *fn, hipStream_t st)
{
  if (!st) st = e->ctx->stream;
  if (e->n_dims == 2) return mpi_launch<2>(e, f, k, false, st, fn);
  return mpi_launch<3>(e, f, k, split_plan(e, nullptr, 0, e->ctx->fused_mode).variant == 2, st, fn);
}

int PartitionedSplit::init(hfx_eles *e_, hfx_inters *const *int_faces, int n_int, hfx_inters *const *mpi_faces_, int n_mpi_, int in_step_)
{
  e = e_; mpi_faces = mpi_faces_; n_mpi = n_mpi_; in_step = in_step_;
  for (int b = 0; b < n_mpi; b++) HFX_CHECK(mpi_faces[b]->is_mpi && mpi_faces[b]->left == e, "bad partition-face block");
  if (ensure_fused_tables(e, int_faces, n_int, true)) return 1;
  const int nst = n_rk_stages(e->ctx->params);
  HFX_CHECK(in_step >= 0 && in_step < nst, "hfx_stage_partitioned: stage %d out of range", in_step);
  // variant 3: fluxes in the gradient kernel, Fn on the wire; 2 with an LES closure
  SplitPlan pl;
  if (split_stage_plan(e, int_faces, n_int, e->ctx->fused_mode, &pl)) return 1;
  stage = SplitStage::make(e, int_faces, n_int, in_step, in_step == nst - 1, pl);
  return stage ? 0 : 1;
}

int PartitionedSplit::mpi_all(MpiKernel k, hipStream_t st) const
{
  const bool sgs_ref = stage->pl.variant == 2;
  for (int b = 0; b < n_mpi; b++)
    if ((e->n_dims == 2 ? mpi_launch<2>(e, mpi_faces[b], k, sgs_ref, st) : mpi_launch<3>(e, mpi_faces[b], k, sgs_ref, st))) return 1;
  return 0;
}

int PartitionedSplit::interior_ldg() const
{
  if (in_step == 0 && e->les_ready && e->les.sgs_model >= 2)
  {
    HFX_CHECK(e->les.sgs_model != 3, "hfx_stage_partitioned: the SVV closure filters the state at the first stage, after its flux-point "
                                     "values have left for the neighbours: run it per method");
    if (hfx_eles_calc_sgs_terms(e)) return 1; // Leonard terms of this step (src/solver.cpp:55-62)
  }
  return stage->ldg();
}

int PartitionedSplit::update(EleList list) const
{
  if (stage->update(list)) return 1; // residual, RK, new disu_fpts
  // src/HiFiLES.cpp:214-216: the filter changes disu_upts(0) after the WHOLE update (no element lists then: pl.split_update) --
  // redo the flux-point solution
  return (list == EleList::all && e->shock_ready) ? shock_capture_keep_fpts(e) : 0;
}
