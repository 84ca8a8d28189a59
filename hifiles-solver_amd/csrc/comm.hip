// comm.hip -- the partition-face transport of libhfx: RCCL point-to-point over xGMI, owned by the library.
//
// Reference side: mpi_inters::send_solution / receive_solution / send_corrected_gradient / receive_corrected_gradient
// (/root/reference/src/mpi_inters.cpp:218-336: pack, MPI_Isend + MPI_Irecv per neighbour rank, MPI_Waitall) and the
// places CalcResidual calls them (src/solver.cpp:68-72,131-139,148-155,197-210).  Here a message is one
// ncclSend / ncclRecv pair per neighbour inside one group on a communication stream; "send" = record `packed` on the
// compute stream, make the communication stream wait for it, enqueue the group, record `received`; "receive" = make the
// compute stream wait for `received`.  The host never blocks inside a stage.
//
// librccl is resolved at run time so that a process that never creates a communicator does not need it, and so that
// a launcher that already mapped a librccl (PyTorch ships one with the same soname) shares that copy.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>

#include <vector>

#include "fused_hex.hpp"
#include "general.hpp"
#include "simplex2d.hpp"
#include "split_common.hpp"
#include "step_loop.hpp"

namespace hfx
{

struct Rccl
{
  void *handle = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
  ncclResult_t (*CommCuDevice)(const ncclComm_t, int *) = nullptr;
  ncclResult_t (*CommUserRank)(const ncclComm_t, int *) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
};

static Rccl g_rccl;

static int rccl_load()
{
  if (g_rccl.handle) return 0;
  void *h = nullptr;
  // a copy that is already mapped (same soname) first, then the system one
  const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  for (const char *n : names)
    if ((h = dlopen(n, RTLD_NOW | RTLD_NOLOAD | RTLD_LOCAL))) break;
  if (!h)
    for (const char *n : names)
      if ((h = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
  HFX_CHECK(h, "librccl.so.1 could not be loaded: %s", dlerror());
#define HFX_SYM(field, name)                                             \
  g_rccl.field = (decltype(g_rccl.field))dlsym(h, name);                 \
  HFX_CHECK(g_rccl.field, "librccl lacks the symbol %s", name)
  HFX_SYM(GetUniqueId, "ncclGetUniqueId");
  HFX_SYM(CommInitRank, "ncclCommInitRank");
  HFX_SYM(CommDestroy, "ncclCommDestroy");
  HFX_SYM(GroupStart, "ncclGroupStart");
  HFX_SYM(GroupEnd, "ncclGroupEnd");
  HFX_SYM(Send, "ncclSend");
  HFX_SYM(Recv, "ncclRecv");
  HFX_SYM(AllReduce, "ncclAllReduce");
  HFX_SYM(CommCount, "ncclCommCount");
  HFX_SYM(CommCuDevice, "ncclCommCuDevice");
  HFX_SYM(CommUserRank, "ncclCommUserRank");
  HFX_SYM(GetErrorString, "ncclGetErrorString");
#undef HFX_SYM
  g_rccl.handle = h;
  return 0;
}

#define HFX_NCCL(call)                                                                                       \
  do                                                                                                         \
  {                                                                                                          \
    ncclResult_t _r = (call);                                                                                \
    if (_r != ncclSuccess)                                                                                   \
    {                                                                                                        \
      hfx::set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #call, hfx::g_rccl.GetErrorString(_r));     \
      return 1;                                                                                              \
    }                                                                                                        \
  } while (0)

// which buffers an exchange moves and how long a face record is.  kind 0: the flux-point solution; kind 2: the SGS flux; kind 1: the
// corrected gradient (per-method path and fused mode 2, as the reference sends it) or, with `projected`, each side's
// viscous flux projected on its own normal (fused mode 3: n_fields instead of n_fields * n_dims doubles per flux point)
static void exchange_buffers(const hfx_inters *f, int kind, bool projected, double *&out, double *&in, long &rec)
{
  const hfx_eles *l = f->left;
  rec = (long)f->n_fpts_per_inter * l->n_fields;
  if (kind == 0)
  {
    out = f->out_disu;
    in = f->in_disu;
    return;
  }
  if (kind == 2) // LES: the physical SGS flux, laid out like the gradient (src/mpi_inters.cpp:65-66)
  {
    out = f->out_sgsf;
    in = f->in_sgsf;
    rec *= l->n_dims;
    return;
  }
  out = f->out_grad;
  in = f->in_grad;
  if (!projected) rec *= l->n_dims;
}

// the grouped exchange of `kind` for the given partition-face blocks, ordered after everything the compute stream has
// been given so far
// ordered: the communication stream is already behind the kernels that packed the buffers (they ran on it)
static int start_exchange(hfx_comm *c, hfx_inters *const *mpi_faces, int n_mpi, int kind, bool projected, bool ordered = false)
{
  hipStream_t cs = c->stream;
  if (!ordered)
  {
    HFX_HIP(hipEventRecord(c->packed[kind], c->ctx->stream));
    HFX_HIP(hipStreamWaitEvent(cs, c->packed[kind], 0));
  }
  bool any = false;
  for (int b = 0; b < n_mpi; b++) any = any || !mpi_faces[b]->seg_peer.empty();
  if (any)
  {
    ncclComm_t comm = (ncclComm_t)c->nccl;
    // (checked before the group opens: a failure inside it must not leave the thread's group depth at 1)
    for (int b = 0; b < n_mpi; b++)
      for (int peer : mpi_faces[b]->seg_peer)
        HFX_CHECK(peer >= 0 && peer < c->nranks, "partition-face block: neighbour rank %d is not one of the communicator's %d ranks", peer, c->nranks);
    HFX_NCCL(g_rccl.GroupStart());
    ncclResult_t r = ncclSuccess;
    for (int b = 0; b < n_mpi && r == ncclSuccess; b++)
    {
      const hfx_inters *f = mpi_faces[b];
      double *out, *in;
      long rec;
      exchange_buffers(f, kind, projected, out, in, rec);
      for (size_t s = 0; s < f->seg_peer.size() && r == ncclSuccess; s++)
      {
        const size_t n = (size_t)f->seg_count[s] * rec;
        r = g_rccl.Send(out + (size_t)f->seg_send[s] * rec, n, ncclDouble, f->seg_peer[s], comm, cs);
        if (r == ncclSuccess) r = g_rccl.Recv(in + (size_t)f->seg_recv[s] * rec, n, ncclDouble, f->seg_peer[s], comm, cs);
      }
    }
    if (r != ncclSuccess)
    {
      (void)g_rccl.GroupEnd(); // close the group whatever it says, so that later RCCL calls on this thread are not queued into it
      set_error("%s:%d: ncclSend / ncclRecv of exchange %d failed: %s", __FILE__, __LINE__, kind, g_rccl.GetErrorString(r));
      return 1;
    }
    HFX_NCCL(g_rccl.GroupEnd());
  }
  HFX_HIP(hipEventRecord(c->received[kind], cs));
  c->posted[kind] += n_mpi;
  if (kind == 0) c->in_flight += n_mpi;
  return 0;
}

// the compute stream waits for the exchange of `kind`; n: the partition-face blocks whose messages that consumes
static int wait_exchange(hfx_comm *c, int kind, int n)
{
  HFX_HIP(hipStreamWaitEvent(c->ctx->stream, c->received[kind], 0));
  c->waited[kind] += n;
  if (kind == 0) c->in_flight = std::max(0, c->in_flight - n);
  return 0;
}

// is e's flux-point solution of the current state on its way over c already?
static bool sent_over(const hfx_eles *e, const hfx_comm *c) { return e->fpts_sent && e->sent_on == c->serial; }

// a partitioned fused stage left e's new flux-point solution on its way (fpts_sent) and the state changes before a stage
// consumes it: the compute stream waits for that message, which is then dropped (a stage after this one packs and posts again)
int invalidate_fpts(hfx_eles *e)
{
  for (hfx_comm *c : e->ctx->comms)
    if (sent_over(e, c) && c->in_flight > 0 && wait_exchange(c, 0, e->sent_blocks)) return 1;
  e->fpts_valid = e->fpts_sent = false;
  e->sent_on = 0;
  return 0;
}

// what a partitioned loop leaves behind: it drained the message it posted last, nothing of these blocks is on its way
static void mark_drained(hfx_eles *const *eles, int n)
{
  for (int i = 0; i < n; i++)
  {
    eles[i]->fpts_sent = false;
    eles[i]->sent_on = 0;
  }
}

struct StageTimers
{
  hipEvent_t ph[5] = {}, x0[2] = {}, x1[2] = {}, fk[2] = {};
  double acc[8] = {};
  int create()
  {
    for (auto &x : ph) HFX_HIP(hipEventCreate(&x));
    for (auto &x : x0) HFX_HIP(hipEventCreate(&x));
    for (auto &x : x1) HFX_HIP(hipEventCreate(&x));
    for (auto &x : fk) HFX_HIP(hipEventCreate(&x));
    return 0;
  }
  void destroy()
  {
    for (auto &x : ph) (void)hipEventDestroy(x);
    for (auto &x : x0) (void)hipEventDestroy(x);
    for (auto &x : x1) (void)hipEventDestroy(x);
    for (auto &x : fk) (void)hipEventDestroy(x);
  }
};

// the partition-face blocks of a partitioned fused stage on these element blocks (split: one; general: several)
static int check_partition_blocks(hfx_eles *const *eles, int neb, hfx_inters *const *mpi_faces, int n_mpi, hfx_comm *comm)
{
  HFX_CHECK(comm && comm->ctx == eles[0]->ctx, "the communicator belongs to another context");
  for (int b = 0; b < n_mpi; b++)
  {
    const hfx_inters *f = mpi_faces[b];
    HFX_CHECK(f->is_mpi, "bad partition-face block");
    bool mine = false;
    for (int i = 0; i < neb; i++) mine = mine || f->left == eles[i];
    HFX_CHECK(mine, "a partition-face block belongs to an element block that is not part of this call");
    int listed = 0;
    for (int c : f->seg_count) listed += c;
    HFX_CHECK(listed == f->n_inters, "partition-face block: %d of %d faces have a neighbour (hfx_mpi_inters_set_neighbours)", listed,
              f->n_inters);
    for (int peer : f->seg_peer)
      HFX_CHECK(peer >= 0 && peer < comm->nranks, "partition-face block: neighbour rank %d is not one of the communicator's %d ranks", peer, comm->nranks);
  }
  return 0;
}

// ONE RK stage of the split fused path on a partitioned block with the library's transport, in CalcResidual's order
// (src/solver.cpp:68-72,131-139,148-155,197-210).  start: the flux-point solution of the current state has not been packed
// and sent yet (the first stage after the caller changed the state; later stages find the exchange that the previous
// stage started after its update).  Leaves the exchange of the NEW state's flux-point solution in flight.
int partitioned_stage(hfx_eles *e, hfx_inters *const *int_faces, int n_int, hfx_inters *const *mpi_faces, int n_mpi, hfx_comm *comm,
                      int rk, bool start, StageTimers *T)
{
  hfx_ctx *ctx = e->ctx;
  const bool visc = ctx->params.viscous != 0;
  PartitionedSplit s; // the steps of this stage, and its plan
  if (s.init(e, int_faces, n_int, mpi_faces, n_mpi, rk)) return 1;
  const SplitPlan &pl = s.stage->pl; // projected: variant 3 sends the projected viscous flux
  note_gradients(e, pl.variant != 3); // (what the stage will have left once its launches below are made; deferred.hip overrides it)
  // third message: the SGS flux (src/solver.cpp:168-178,203-206) -- variant 2 only; in variant 3 it is part of the projected flux
  const bool les = e->les_ready && !pl.projected;
  hipStream_t st = ctx->stream, cs = comm->stream;
  // (the timed form keeps every kernel of a phase on the compute stream, so that its events bracket the phase)
  const bool beside = ctx->opt.comm_stream_faces && pl.projected && !les && visc && T == nullptr;
  if (start)
  {
    if (hfx_eles_extrapolate_solution(e)) return 1;
    if (s.pack_solution(st)) return 1;
    if (start_exchange(comm, mpi_faces, n_mpi, 0, false)) return 1; // later stages: started after the update of the previous one
  }
  if (beside)
  {
    // ---- partition-face kernels and exchanges on the communication stream, in its order; the compute stream meets it
    // at two events per stage: before the flux kernel (LDG corrections at the partition faces are in place) and before
    // the update kernel (common fluxes at the partition faces are in place)
    if (s.interior_ldg()) return 1;
    if (s.partition_ldg(cs)) return 1; // (behind the receive)
    HFX_HIP(hipEventRecord(comm->received[0], cs));
    // the flux kernel in three launches (option split_flux): half of the elements WITHOUT partition-face points first -- they
    // need nothing from the neighbours, so the solution exchange runs beside them --, then the elements with, whose projected
    // fluxes then leave beside the other half (and the interior common-flux kernel)
    const bool split_flux = ctx->opt.split_flux && pl.split_flux && n_mpi > 0;
    if (split_flux && s.stage->flux_kernel(EleList::interior_1)) return 1;
    if (wait_exchange(comm, 0, n_mpi)) return 1;
    if (s.stage->element_kernels(split_flux ? EleList::partition : EleList::all)) return 1;
    HFX_HIP(hipEventRecord(comm->packed[1], st));
    HFX_HIP(hipStreamWaitEvent(cs, comm->packed[1], 0));
    if (s.pack_projected_flux(cs)) return 1;
    if (start_exchange(comm, mpi_faces, n_mpi, 1, true, true)) return 1;
    if (s.partition_common_fluxes(cs)) return 1;
    HFX_HIP(hipEventRecord(comm->received[1], cs));
    if (split_flux && s.stage->flux_kernel(EleList::interior_2)) return 1;
    if (s.stage->common_fluxes()) return 1;
    if (wait_exchange(comm, 1, n_mpi)) return 1;
    // the update: first the elements with partition-face points, whose new flux-point solution is packed and sent (communication
    // stream) while the others are updated -- the exchange the next stage's flux kernel waits for is hidden behind them
    const bool split_update = ctx->opt.split_update && pl.split_update && n_mpi > 0;
    if (s.update(split_update ? EleList::partition : EleList::all)) return 1; // (the whole update: + shock capturing)
    HFX_HIP(hipEventRecord(comm->packed[0], st));
    HFX_HIP(hipStreamWaitEvent(cs, comm->packed[0], 0));
    if (s.pack_solution(cs)) return 1;
    if (start_exchange(comm, mpi_faces, n_mpi, 0, false, true)) return 1;
    return split_update ? s.update(EleList::interior) : 0;
  }
  // ---- everything on the compute stream (optionally timed): the five phases of hfx_stage_partitioned with the exchanges between
  if (T) HFX_HIP(hipEventRecord(T->ph[0], st));
  if (visc && s.interior_ldg()) return 1;
  if (T) HFX_HIP(hipEventRecord(T->ph[1], st));
  if (wait_exchange(comm, 0, n_mpi)) return 1;
  const bool pieces = T && pl.projected && visc; // the element kernel bracketed on its own
  if (visc && s.partition_ldg(st)) return 1;
  if (pieces) HFX_HIP(hipEventRecord(T->fk[0], st));
  if ((pl.projected || visc) && s.stage->element_kernels()) return 1;
  if (pieces) HFX_HIP(hipEventRecord(T->fk[1], st));
  if (visc && (pl.projected ? s.pack_projected_flux(st) : s.pack_gradient(st))) return 1;
  if (visc && les && s.pack_sgs_flux(st)) return 1;
  if (visc)
  {
    if (T) HFX_HIP(hipEventRecord(T->x1[0], st));
    if (start_exchange(comm, mpi_faces, n_mpi, 1, pl.projected)) return 1;
    if (les && start_exchange(comm, mpi_faces, n_mpi, 2, false)) return 1;
    if (T) HFX_HIP(hipEventRecord(T->x1[1], cs));
  }
  if (T) HFX_HIP(hipEventRecord(T->ph[2], st));
  if (s.stage->common_fluxes()) return 1;
  if (!pl.projected && s.partition_common_invflux(st)) return 1;
  if (T) HFX_HIP(hipEventRecord(T->ph[3], st));
  if (visc && wait_exchange(comm, 1, n_mpi)) return 1;
  if (visc && les && wait_exchange(comm, 2, n_mpi)) return 1;
  if (pl.projected ? s.partition_common_fluxes(st) : (visc && s.partition_common_viscflux(st))) return 1;
  if (s.update()) return 1; // (+ shock capturing)
  if (s.pack_solution(st)) return 1;
  if (T) HFX_HIP(hipEventRecord(T->x0[0], st));
  if (start_exchange(comm, mpi_faces, n_mpi, 0, false)) return 1;
  if (T)
  {
    HFX_HIP(hipEventRecord(T->x0[1], cs));
    HFX_HIP(hipEventRecord(T->ph[4], st));
    HFX_HIP(hipStreamSynchronize(st));
    HFX_HIP(hipStreamSynchronize(cs));
    float t = 0;
    for (int w = 0; w < 4; w++)
    {
      HFX_HIP(hipEventElapsedTime(&t, T->ph[w], T->ph[w + 1]));
      T->acc[w] += t;
    }
    HFX_HIP(hipEventElapsedTime(&t, T->x0[0], T->x0[1]));
    T->acc[4] += t;
    if (visc)
    {
      HFX_HIP(hipEventElapsedTime(&t, T->x1[0], T->x1[1]));
      T->acc[5] += t;
    }
    HFX_HIP(hipEventElapsedTime(&t, T->ph[0], T->ph[4]));
    T->acc[6] += t;
    if (pieces)
    {
      HFX_HIP(hipEventElapsedTime(&t, T->fk[0], T->fk[1]));
      T->acc[7] += t;
    }
  }
  return 0;
}

// the deferred scheduler's stage (deferred.hip): as above, no timers
int partitioned_stage_deferred(hfx_eles *e, hfx_inters *const *int_faces, int n_int, hfx_inters *const *mpi_faces, int n_mpi,
                               hfx_comm *comm, int rk, bool start)
{
  if (check_partition_blocks(&e, 1, mpi_faces, n_mpi, comm)) return 1;
  return partitioned_stage(e, int_faces, n_int, mpi_faces, n_mpi, comm, rk, start, nullptr);
}

// ONE RK stage of the 2-D simplex fused stage (simplex2d.hip) on ONE partitioned block of triangles, interior groups first.  The
// kernels walk groups of G consecutive elements; a group with a partition flux point is a partition group, the others need nothing
// from the neighbours.  `all`: the interior, boundary and partition-face blocks the tables were prepared with.
//   [solution message in flight]   boundary ghost states; element kernel on the interior groups
//   wait 0                         (LDG corrections at the partition faces unless the element kernel gathers them); element
//                                  kernel on the partition groups
//   pack Fn, start exchange 1      interior common fluxes, boundary viscous fluxes
//   wait 1; one-sided common fluxes
//   update kernel on the partition groups; pack the new flux-point solution, start exchange 0
//   update kernel on the interior groups   <- beside exchange 0, as is the next stage's interior element launch
// An inviscid run has no exchange 1 and no LDG step; the order is otherwise the same.
// shock: eles::shock_capture follows the stage.  Folded into the update kernel (Simplex2dPlan::fold_shock) nothing changes in the
// order above: the update on the partition groups writes the FILTERED state's flux-point solution of those groups (an element's
// filter reads that element alone), the event `packed[0]` is recorded behind that launch, and the pack on the communication stream
// waits for it -- what leaves is the filtered state's.  Not folded (option fold_shock 0) the filter and the extrapolation of the
// filtered state run behind BOTH update launches and the pack waits for them: nothing is hidden behind the interior groups then.
static int simplex2d_partitioned_stage(hfx_eles *e, hfx_inters *const *all, int n_all, hfx_inters *const *mpi_faces, int n_mpi,
                                       hfx_comm *comm, int rk, bool start, bool shock)
{
  hfx_ctx *ctx = e->ctx;
  const bool visc = ctx->params.viscous != 0;
  hipStream_t st = ctx->stream, cs = comm->stream;
  const Simplex2dPartitionPlan pp = simplex2d_partition_plan(e);
  // the one-sided kernels read e->arr[HFX_DISU_FPTS] when they are LAUNCHED (mpi_launch fills its arguments then): a pack
  // launched behind simplex2d_swap_disu_fpts sees the buffer the update kernels wrote, whatever stream it runs on
  auto mpi_all = [&](MpiKernel k, hipStream_t s) -> int {
    for (int b = 0; b < n_mpi; b++)
      if (mpi_launch_general(e, mpi_faces[b], k, simplex2d_fn_fpts(e), s)) return 1;
    return 0;
  };
  if (start)
  {
    if (mpi_all(MpiKernel::pack_solution, st)) return 1;
    if (start_exchange(comm, mpi_faces, n_mpi, 0, false)) return 1;
  }
  if (simplex2d_interior_ldg(e, all, n_all)) return 1;
  // (over-integration folded into the element kernel: nothing here; option fold_over_int 0: the per-method launches on the whole
  // block, on the compute stream beside the solution message -- they read the solution points alone)
  if (simplex2d_over_int_unfolded(e)) return 1;
  if (simplex2d_element_kernel(e, rk, S2dList::interior)) return 1;
  if (wait_exchange(comm, 0, n_mpi)) return 1;
  if (visc && !pp.gather_remote && mpi_all(MpiKernel::ldg_delta, st)) return 1;
  if (simplex2d_element_kernel(e, rk, S2dList::partition)) return 1;
  if (visc)
  {
    if (mpi_all(MpiKernel::pack_projected_flux, st)) return 1;
    if (start_exchange(comm, mpi_faces, n_mpi, 1, true)) return 1;
  }
  if (simplex2d_common_fluxes(e, all, n_all)) return 1;
  if (visc && wait_exchange(comm, 1, n_mpi)) return 1;
  if (mpi_all(MpiKernel::common_flux_projected, st)) return 1;
  // the partition groups first: their new flux-point solution leaves (packed on the communication stream, behind this launch
  // alone) while the interior groups are updated
  const bool filter_behind = shock && e->shock_ready && !simplex2d_folds_shock(e);
  if (simplex2d_update_kernel(e, rk, S2dList::partition, shock)) return 1;
  if (!filter_behind)
  {
    HFX_HIP(hipEventRecord(comm->packed[0], st));
    HFX_HIP(hipStreamWaitEvent(cs, comm->packed[0], 0));
  }
  if (simplex2d_update_kernel(e, rk, S2dList::interior, shock)) return 1;
  simplex2d_swap_disu_fpts(e); // once, behind both launches: what is packed now is the new state's
  if (filter_behind)
  {
    if (general_shock_capture(&e, 1)) return 1; // (the filter, then disu_fpts of the filtered state)
    HFX_HIP(hipEventRecord(comm->packed[0], st));
    HFX_HIP(hipStreamWaitEvent(cs, comm->packed[0], 0));
  }
  if (mpi_all(MpiKernel::pack_solution, cs)) return 1;
  note_gradients(e, false); // (the stage keeps them on chip)
  return start_exchange(comm, mpi_faces, n_mpi, 0, false, true);
}

// ONE RK stage of the GENERAL fused stage (general.hip: tetrahedra, prisms, several element blocks) on partitioned blocks: the
// stage's four parts with the one-sided partition-face kernels and the two exchanges between them, in CalcResidual's order
// (src/solver.cpp:68-72,131-139,148-155,197-210; mpi_inters::set_mpi takes any element class, src/mpi_inters.cpp:154):
//   [start: pack the flux-point solution, exchange]            interior LDG pairs / boundary ghost states
//   wait; LDG corrections at the partition faces               flux kernels of all blocks
//   pack each side's projected viscous flux Fn, exchange       interior common fluxes, boundary viscous fluxes
//   wait; common fluxes at the partition faces                 update kernels (new flux-point solution)
//   pack the new flux-point solution, exchange (for the next stage)
// (the prepare below is what a deferred stage relies on; hfx_run_steps_partitioned_blocks has prepared the same tables before its loop
// -- for EVERY element class, so that whatever they refuse is refused before the state is touched -- and finds it a no-op here)
int general_partitioned_stage(hfx_eles *const *eles, int neb, hfx_inters *const *int_faces, int n_int, hfx_inters *const *mpi_faces,
                              int n_mpi, hfx_comm *comm, int rk, bool start, bool shock)
{
  HFX_CHECK(neb > 0 && comm, "general partitioned stage: bad argument");
  if (check_partition_blocks(eles, neb, mpi_faces, n_mpi, comm)) return 1;
  const bool visc = eles[0]->ctx->params.viscous != 0;
  // the blocks' tables are built with ALL face blocks (every flux point needs its face)
  std::vector<hfx_inters *> all(int_faces, int_faces + n_int);
  all.insert(all.end(), mpi_faces, mpi_faces + n_mpi);
  if (general_prepare(eles, neb, all.data(), (int)all.size(), true)) return 1;
  // one block of triangles: the 2-D simplex stage, interior groups first (nothing of it is refused past this point; LES
  // and shock capturing of another form than the triangle's own were refused by the tables)
  if (neb == 1 && is_simplex2d(eles[0]))
    return simplex2d_partitioned_stage(eles[0], all.data(), (int)all.size(), mpi_faces, n_mpi, comm, rk, start, shock);
  auto mpi_all = [&](MpiKernel k) -> int {
    for (int b = 0; b < n_mpi; b++)
      if (mpi_launch_general(mpi_faces[b]->left, mpi_faces[b], k, general_fn_fpts(mpi_faces[b]->left))) return 1;
    return 0;
  };
  const GeneralStage stage(eles, neb, all.data(), (int)all.size(), rk);
  if (start)
  {
    if (mpi_all(MpiKernel::pack_solution)) return 1;
    if (start_exchange(comm, mpi_faces, n_mpi, 0, false)) return 1;
  }
  if (stage.interior_ldg()) return 1;
  if (wait_exchange(comm, 0, n_mpi)) return 1;
  if (visc && mpi_all(MpiKernel::ldg_delta)) return 1;
  if (stage.flux_kernels()) return 1;
  if (visc)
  {
    if (mpi_all(MpiKernel::pack_projected_flux)) return 1;
    if (start_exchange(comm, mpi_faces, n_mpi, 1, true)) return 1;
  }
  if (stage.common_fluxes()) return 1;
  if (visc && wait_exchange(comm, 1, n_mpi)) return 1;
  if (mpi_all(MpiKernel::common_flux_projected)) return 1;
  if (stage.update_kernels()) return 1;
  // eles::shock_capture (src/HiFiLES.cpp:214-216) before the new flux-point solution is packed: the filter, then the flux-point
  // values of the filtered state
  if (shock && general_shock_capture(eles, neb)) return 1;
  if (mpi_all(MpiKernel::pack_solution)) return 1;
  for (int i = 0; i < neb; i++) note_gradients(eles[i], false); // (the general stage keeps them on chip)
  return start_exchange(comm, mpi_faces, n_mpi, 0, false);
}

// the exchange started after the last stage belongs to a stage that is not run: the compute stream waits for it so that nothing is in
// flight when the caller reads or changes the state (a following call starts over with a first stage that posts)
static int drain(hfx_eles *const *eles, int neb, hfx_comm *comm, int n_mpi)
{
  if (wait_exchange(comm, 0, n_mpi)) return 1;
  mark_drained(eles, neb);
  return 0;
}

// the stages of hfx_time_partitioned: `reps` stages of consecutive time steps with the timers, calc_time_step in front of every step and
// the ramp counters behind it (behind a partial last one too); no body force, no clock, no samples
static int time_partitioned_stages(hfx_eles *e, hfx_inters *const *int_faces, int n_int, hfx_inters *const *mpi_faces, int n_mpi,
                                   hfx_comm *comm, int reps, StageTimers *T)
{
  if (check_partition_blocks(&e, 1, mpi_faces, n_mpi, comm)) return 1;
  const int nst = n_rk_stages(e->ctx->params);
  bool first = !sent_over(e, comm); // (as hfx_run_steps_partitioned)
  for (int done = 0; done < reps; done++)
  {
    const int rk = done % nst;
    if (rk == 0 && calc_time_step_blocks(&e, 1, comm)) return 1;
    if (partitioned_stage(e, int_faces, n_int, mpi_faces, n_mpi, comm, rk, first, T)) return 1;
    first = false;
    if (rk == nst - 1 || done == reps - 1) advance_ramp_counters(int_faces, n_int);
  }
  return drain(&e, 1, comm, n_mpi);
}

} // namespace hfx

using namespace hfx;

extern "C" {

int hfx_comm_get_unique_id(char id[HFX_COMM_ID_BYTES])
{
  HFX_CHECK(id, "hfx_comm_get_unique_id: NULL argument");
  static_assert(HFX_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");
  if (rccl_load()) return 1;
  ncclUniqueId u;
  HFX_NCCL(g_rccl.GetUniqueId(&u));
  std::memcpy(id, u.internal, HFX_COMM_ID_BYTES);
  return 0;
}

int hfx_comm_create(hfx_ctx *ctx, const char id[HFX_COMM_ID_BYTES], int nranks, int rank, hfx_comm **out)
{
  HFX_CHECK(ctx && id && out, "hfx_comm_create: NULL argument");
  HFX_CHECK(nranks >= 1 && rank >= 0 && rank < nranks, "hfx_comm_create: rank %d of %d", rank, nranks);
  if (rccl_load()) return 1;
  HFX_HIP(hipSetDevice(ctx->device));
  hfx_comm *c = new hfx_comm();
  c->ctx = ctx;
  static unsigned long n_created = 0;
  c->serial = ++n_created;
  c->nranks = nranks;
  c->rank = rank;
  ncclUniqueId u;
  std::memcpy(u.internal, id, HFX_COMM_ID_BYTES);
  ncclComm_t comm = nullptr;
  ncclResult_t r = g_rccl.CommInitRank(&comm, nranks, u, rank);
  if (r != ncclSuccess)
  {
    set_error("ncclCommInitRank(rank %d of %d) failed: %s", rank, nranks, g_rccl.GetErrorString(r));
    delete c;
    return 1;
  }
  c->nccl = comm;
  // (a failure from here on must not leak the communicator: the peers hold its other members)
  auto rest = [&]() -> int {
    HFX_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (int k = 0; k < 3; k++)
    {
      HFX_HIP(hipEventCreateWithFlags(&c->packed[k], hipEventDisableTiming));
      HFX_HIP(hipEventCreateWithFlags(&c->received[k], hipEventDisableTiming));
    }
    return c->scratch.alloc(64);
  };
  if (rest())
  {
    const std::string msg = hfx_last_error();
    (void)hfx_comm_destroy(c);
    set_error("%s", msg.c_str());
    return 1;
  }
  ctx->comms.push_back(c);
  *out = c;
  return 0;
}

int hfx_comm_destroy(hfx_comm *c)
{
  if (!c) return 0;
  if (c->ctx)
  {
    // what has been recorded may name this communicator: run it, then forget the plans that do
    (void)defer_flush(c->ctx, 0);
    c->ctx->defer.plans.clear();
    auto &v = c->ctx->comms;
    v.erase(std::remove(v.begin(), v.end(), c), v.end());
  }
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->nccl) (void)g_rccl.CommDestroy((ncclComm_t)c->nccl);
  for (int k = 0; k < 3; k++)
  {
    if (c->packed[k]) (void)hipEventDestroy(c->packed[k]);
    if (c->received[k]) (void)hipEventDestroy(c->received[k]);
  }
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return 0;
}

int hfx_comm_info(hfx_comm *c, int *nranks, int *rank, int *device, char pci_bus_id[32])
{
  HFX_CHECK(c && c->nccl, "hfx_comm_info: no communicator");
  // what RCCL itself says about this communicator (not what it was asked for)
  int n = 0, r = 0, d = 0;
  HFX_NCCL(g_rccl.CommCount((ncclComm_t)c->nccl, &n));
  HFX_NCCL(g_rccl.CommUserRank((ncclComm_t)c->nccl, &r));
  HFX_NCCL(g_rccl.CommCuDevice((ncclComm_t)c->nccl, &d));
  if (nranks) *nranks = n;
  if (rank) *rank = r;
  if (device) *device = d;
  if (pci_bus_id)
  {
    pci_bus_id[0] = 0;
    HFX_HIP(hipDeviceGetPCIBusId(pci_bus_id, 32, d));
  }
  return 0;
}

int hfx_comm_allreduce(hfx_comm *c, double *values, int n, int op)
{
  HFX_CHECK(c && values && n >= 1 && n <= 64, "hfx_comm_allreduce: bad argument");
  HFX_CHECK(op >= 0 && op <= 2, "hfx_comm_allreduce: op must be 0 (min), 1 (max) or 2 (sum)");
  const ncclRedOp_t ops[3] = {ncclMin, ncclMax, ncclSum};
  HFX_HIP(hipMemcpyAsync(c->scratch, values, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  HFX_NCCL(g_rccl.AllReduce(c->scratch, c->scratch, (size_t)n, ncclDouble, ops[op], (ncclComm_t)c->nccl, c->stream));
  HFX_HIP(hipMemcpyAsync(values, c->scratch, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HFX_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int hfx_mpi_inters_set_neighbours(hfx_inters *f, int n_seg, const int *peer, const int *send_first, const int *recv_first,
                                  const int *count)
{
  HFX_CHECK(f && f->is_mpi, "not a partition-face block");
  HFX_CHECK(n_seg >= 0 && (n_seg == 0 || (peer && send_first && recv_first && count)), "hfx_mpi_inters_set_neighbours: bad argument");
  HFX_IMMEDIATE(f->ctx, 0);
  f->ctx->defer.plans.clear();
  std::vector<char> sent((size_t)f->n_inters, 0), got((size_t)f->n_inters, 0);
  for (int s = 0; s < n_seg; s++)
  {
    HFX_CHECK(peer[s] >= 0 && count[s] > 0, "segment %d: peer %d, %d faces", s, peer[s], count[s]);
    HFX_CHECK(send_first[s] >= 0 && send_first[s] + count[s] <= f->n_inters && recv_first[s] >= 0 && recv_first[s] + count[s] <= f->n_inters,
              "segment %d leaves the block's %d faces", s, f->n_inters);
    for (int i = 0; i < count[s]; i++)
    {
      HFX_CHECK(!sent[send_first[s] + i] && !got[recv_first[s] + i], "segment %d overlaps another one", s);
      sent[send_first[s] + i] = got[recv_first[s] + i] = 1;
    }
  }
  f->seg_peer.assign(peer, peer + n_seg);
  f->seg_send.assign(send_first, send_first + n_seg);
  f->seg_recv.assign(recv_first, recv_first + n_seg);
  f->seg_count.assign(count, count + n_seg);
  return 0;
}

int hfx_mpi_inters_send_solution(hfx_inters *f, hfx_comm *c)
{
  HFX_CHECK(f && f->is_mpi && c, "hfx_mpi_inters_send_solution: bad argument");
  if (f->n_inters == 0) return 0;
  HFX_DEFER(f->ctx, DM_MPI_SEND_SOLUTION, nullptr, f, c, 0, 0);
  // the partitioned fused stage that produced this state has posted its flux-point solution already (a stage replayed after it,
  // or calls made with the option "deferred" off): posting it again would send the neighbours one message more than the calls
  // ask for, and packing it again would rewrite the buffer that message may still be reading.  receive_solution waits for it
  if (sent_over(f->left, c)) return 0;
  if (hfx_mpi_inters_pack_solution(f)) return 1;
  return start_exchange(c, &f, 1, 0, false);
}

int hfx_mpi_inters_receive_solution(hfx_inters *f, hfx_comm *c)
{
  HFX_CHECK(f && f->is_mpi && c, "hfx_mpi_inters_receive_solution: bad argument");
  if (f->n_inters == 0) return 0;
  HFX_DEFER(f->ctx, DM_MPI_RECEIVE_SOLUTION, nullptr, f, c, 0, 0);
  return wait_exchange(c, 0, 1);
}

int hfx_mpi_inters_send_corrected_gradient(hfx_inters *f, hfx_comm *c)
{
  HFX_CHECK(f && f->is_mpi && c, "hfx_mpi_inters_send_corrected_gradient: bad argument");
  if (f->n_inters == 0) return 0;
  HFX_DEFER(f->ctx, DM_MPI_SEND_GRADIENT, nullptr, f, c, 0, 0);
  if (hfx_mpi_inters_pack_corrected_gradient(f)) return 1;
  return start_exchange(c, &f, 1, 1, false);
}

int hfx_mpi_inters_receive_corrected_gradient(hfx_inters *f, hfx_comm *c)
{
  HFX_CHECK(f && f->is_mpi && c, "hfx_mpi_inters_receive_corrected_gradient: bad argument");
  if (f->n_inters == 0) return 0;
  HFX_DEFER(f->ctx, DM_MPI_RECEIVE_GRADIENT, nullptr, f, c, 0, 0);
  return wait_exchange(c, 1, 1);
}

int hfx_mpi_inters_send_sgsf_fpts(hfx_inters *f, hfx_comm *c)
{
  HFX_CHECK(f && f->is_mpi && c, "hfx_mpi_inters_send_sgsf_fpts: bad argument");
  if (f->n_inters == 0) return 0;
  HFX_DEFER(f->ctx, DM_MPI_SEND_SGSF, nullptr, f, c, 0, 0);
  if (hfx_mpi_inters_pack_sgsf(f)) return 1;
  return start_exchange(c, &f, 1, 2, false);
}

int hfx_mpi_inters_receive_sgsf_fpts(hfx_inters *f, hfx_comm *c)
{
  HFX_CHECK(f && f->is_mpi && c, "hfx_mpi_inters_receive_sgsf_fpts: bad argument");
  if (f->n_inters == 0) return 0;
  HFX_DEFER(f->ctx, DM_MPI_RECEIVE_SGSF, nullptr, f, c, 0, 0);
  return wait_exchange(c, 2, 1);
}

int hfx_run_steps_partitioned(hfx_eles *e, hfx_inters *const *int_faces, int n_int, hfx_inters *const *mpi_faces, int n_mpi,
                              hfx_comm *comm, int n_steps)
{
  HFX_CHECK(e && comm, "hfx_run_steps_partitioned: NULL argument");
  HFX_CHECK(e->ctx->have_params, "parameters not set");
  HFX_IMMEDIATE(e->ctx, 0);
  if (step_loop_check(&e, 1, int_faces, n_int, n_steps)) return 1;
  if (const char *refusal = monitor_gradient_on_chip(&e, 1))
  {
    // (a plan of variant 2 writes grad_disu_upts in every stage: everything is sampled)
    SplitPlan pl;
    if (ensure_fused_tables(e, int_faces, n_int, true) || split_stage_plan(e, int_faces, n_int, e->ctx->fused_mode, &pl)) return 1;
    HFX_CHECK(pl.variant != 3, "%s", refusal);
  }
  if (check_partition_blocks(&e, 1, mpi_faces, n_mpi, comm)) return 1;
  // a partitioned fused stage of the deferred path may have left this state's flux-point solution on its way already: the
  // first stage takes it instead of posting it again (the messages a rank posts follow its calls, not what ran deferred)
  bool first = !sent_over(e, comm);
  // (closure none: the stage's first phase filters at stage 0 itself, split_partitioned.hpp.  The body force, the time step and the
  // samples read disu_upts(0) on the compute stream; the solution exchange a stage leaves in flight reads the packed flux-point values)
  StepLoop loop{&e, 1, int_faces, n_int, [&](int rk) {
                  const bool start = first;
                  first = false;
                  return partitioned_stage(e, int_faces, n_int, mpi_faces, n_mpi, comm, rk, start, nullptr);
                }};
  loop.comm = comm;
  if (run_step_loop(loop, n_steps)) return 1;
  return drain(&e, 1, comm, n_mpi); // (after zero steps too)
}

int hfx_run_steps_partitioned_blocks(hfx_eles *const *eles, int n_ele_blocks, hfx_inters *const *int_faces, int n_int,
                                     hfx_inters *const *mpi_faces, int n_mpi, hfx_comm *comm, int n_steps)
{
  HFX_CHECK(eles && n_ele_blocks > 0 && eles[0] && comm, "hfx_run_steps_partitioned_blocks: NULL argument");
  hfx_ctx *ctx = eles[0]->ctx;
  HFX_CHECK(ctx->have_params, "parameters not set");
  HFX_IMMEDIATE(ctx, 0);
  const bool cfl_steps = ctx->params.dt_type == 1 || ctx->params.dt_type == 2;
  HFX_CHECK(!cfl_steps || ctx->have_CFL, "dt_type %d needs run_input.CFL: call hfx_ctx_set_CFL", ctx->params.dt_type);
  if (step_loop_check(eles, n_ele_blocks, int_faces, n_int, n_steps)) return 1;
  if (const char *refusal = monitor_gradient_on_chip(eles, n_ele_blocks)) // (the general stage keeps the gradient on chip)
    HFX_CHECK(false, "%s", refusal);
  // (what the blocks' tables refuse is refused HERE, before the state is touched: the closure filter of a step's first stage -- SVV
  // replaces the state -- runs in front of the stage that would prepare them)
  if (n_steps > 0)
  {
    if (check_partition_blocks(eles, n_ele_blocks, mpi_faces, n_mpi, comm)) return 1;
    std::vector<hfx_inters *> all(int_faces, int_faces + n_int);
    all.insert(all.end(), mpi_faces, mpi_faces + n_mpi);
    if (general_prepare(eles, n_ele_blocks, all.data(), (int)all.size(), true)) return 1;
  }
  for (int i = 0; i < n_ele_blocks; i++)
    if (hfx_eles_extrapolate_solution(eles[i])) return 1;
  // (as hfx_run_steps_partitioned: the solution a partitioned fused stage has posted for this state is not posted again)
  bool start = false;
  for (int i = 0; i < n_ele_blocks; i++) start = start || !sent_over(eles[i], comm);
  StepLoop loop{eles, n_ele_blocks, int_faces, n_int, [&](int rk) {
                  const bool post = start;
                  start = false;
                  return general_partitioned_stage(eles, n_ele_blocks, int_faces, n_int, mpi_faces, n_mpi, comm, rk, post, true);
                }};
  loop.closure = ClosureFilter::filtering; // (partitioned blocks refuse SVV)
  loop.comm = comm;
  if (run_step_loop(loop, n_steps)) return 1;
  return n_steps > 0 ? drain(eles, n_ele_blocks, comm, n_mpi) : 0; // (a call without steps leaves what is in flight as it found it)
}

int hfx_comm_exchange_stats(hfx_comm *c, long posted[3], long waited[3], int *in_flight, int *stream_busy)
{
  HFX_CHECK(c, "hfx_comm_exchange_stats: NULL communicator");
  for (int k = 0; k < 3; k++)
  {
    if (posted) posted[k] = c->posted[k];
    if (waited) waited[k] = c->waited[k];
  }
  if (in_flight) *in_flight = c->in_flight;
  if (stream_busy)
  {
    const hipError_t q = hipStreamQuery(c->stream);
    HFX_CHECK(q == hipSuccess || q == hipErrorNotReady, "hfx_comm_exchange_stats: hipStreamQuery failed: %s", hipGetErrorString(q));
    *stream_busy = q == hipErrorNotReady;
  }
  return 0;
}

int hfx_time_partitioned(hfx_eles *e, hfx_inters *const *int_faces, int n_int, hfx_inters *const *mpi_faces, int n_mpi,
                         hfx_comm *comm, int reps, double ms[8])
{
  HFX_CHECK(e && comm && ms && reps > 0, "hfx_time_partitioned: bad argument");
  HFX_CHECK(e->ctx->have_params, "parameters not set");
  HFX_IMMEDIATE(e->ctx, 0);
  StageTimers T;
  if (T.create()) return 1;
  const int rc = time_partitioned_stages(e, int_faces, n_int, mpi_faces, n_mpi, comm, reps, &T);
  T.destroy();
  if (rc) return 1;
  for (int i = 0; i < 8; i++) ms[i] = T.acc[i] / reps;
  return 0;
}

} // extern "C"
