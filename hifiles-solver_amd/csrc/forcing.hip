// forcing.hip -- the mass-flux body force of driven periodic channels on the device: the `forcing == 1` branch of CalcResidual
// (src/solver.cpp:96-109) and eles::evaluate_body_force (src/eles.cpp:5281-5482).  gfx950 only.
//
// The reference's GPU build copies the whole of disu_upts(0) to the host every step, integrates there and copies five doubles
// back.  Here the controller lives on the device: per evaluation three small launches on the compute stream and, on one rank,
// no copy and no host synchronisation.
//   mass_flux_kernel      integral(m) = sum over the inflow faces of c(., face) . disu_upts(0)(., ele, m), m = 0, 1; one wavefront
//                         per face, a fixed summation order, one partial per workgroup, no floating-point atomics
//   body_force_kernel     one workgroup: the partials in index order, the controller of src/eles.cpp:5411-5428, the record
//   add_body_force_kernel src_upts(j, i, k) += body_force(k) for k = 1 and 4, the force read from the record
// c(k, face) = sum_j weight(j) detjac(j, face) opp_inters_cubpts(j, k) is folded once, at registration, so the per-step integral
// is a dot product of length n_upts per face and field whatever the cubature.
#include "step_loop.hpp"

#include <cmath>
#include <cstddef>

namespace hfx
{

constexpr int BF_FACES_PER_GROUP = 4; // wavefronts of a mass_flux_kernel workgroup = faces it integrates = one partial

struct MassFluxArgs
{
  const double *disu_upts; // disu_upts(0) (n_upts, n_eles, n_fields)
  const double *weights;   // c (n_upts, n_faces)
  const int *face_ele;     // (n_faces)
  double *partial;         // (2, n_groups)
  long P;                  // n_upts * n_eles
  int n_upts, n_faces;
};

// One wavefront per face: lane l takes the points l, l + 64, ... in ascending order, the 64 lane sums are combined by a fixed
// tree, the wavefronts of the workgroup in index order.  The same state gives the same bits.
__global__ __launch_bounds__(64 * BF_FACES_PER_GROUP) void mass_flux_kernel(const MassFluxArgs A)
{
  __shared__ double s[BF_FACES_PER_GROUP][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long face = (long)blockIdx.x * BF_FACES_PER_GROUP + wave;
  double a0 = 0.0, a1 = 0.0;
  if (face < A.n_faces)
  {
    const double *c = A.weights + face * A.n_upts;
    const double *u = A.disu_upts + (long)A.face_ele[face] * A.n_upts;
    for (int k = lane; k < A.n_upts; k += 64)
    {
      const double ck = c[k];
      a0 += ck * u[k];
      a1 += ck * u[A.P + k];
    }
  }
  for (int off = 32; off > 0; off >>= 1)
  {
    a0 += __shfl_down(a0, off, 64);
    a1 += __shfl_down(a1, off, 64);
  }
  if (lane == 0)
  {
    s[wave][0] = a0;
    s[wave][1] = a1;
  }
  __syncthreads();
  if (threadIdx.x == 0)
  {
    double t0 = 0.0, t1 = 0.0;
    for (int w = 0; w < BF_FACES_PER_GROUP; w++)
    {
      t0 += s[w][0];
      t1 += s[w][1];
    }
    A.partial[2 * (long)blockIdx.x] = t0;
    A.partial[2 * (long)blockIdx.x + 1] = t1;
  }
}

enum : int { BF_SUM = 1, BF_CONTROL = 2 }; // what one launch of body_force_kernel does (one rank: both)

struct ControlArgs
{
  const double *partial;
  BodyForceRecord *rec;
  double *ring; // (3, capacity)
  int n_groups, capacity, what;
  double area, mdot0, dt;
};

// One workgroup.  BF_SUM: the partials in index order -> rec->integral.  BF_CONTROL: src/eles.cpp:5398-5428 from rec->integral
// (between the two a partitioned run sums the integrals over the ranks).
__global__ __launch_bounds__(256) void body_force_kernel(const ControlArgs A)
{
  __shared__ double s[2 * 256];
  if (A.what & BF_SUM)
  {
    double t0 = 0.0, t1 = 0.0; // thread 0's
    for (int base = 0; base < A.n_groups; base += 256)
    {
      const int cnt = min(256, A.n_groups - base);
      if ((int)threadIdx.x < cnt)
      {
        s[2 * threadIdx.x] = A.partial[2 * (long)(base + threadIdx.x)];
        s[2 * threadIdx.x + 1] = A.partial[2 * (long)(base + threadIdx.x) + 1];
      }
      __syncthreads();
      if (threadIdx.x == 0)
        for (int i = 0; i < cnt; i++)
        {
          t0 += s[2 * i];
          t1 += s[2 * i + 1];
        }
      __syncthreads();
    }
    if (threadIdx.x == 0)
    {
      A.rec->integral[0] = t0;
      A.rec->integral[1] = t1;
    }
  }
  if ((A.what & BF_CONTROL) && threadIdx.x == 0)
  {
    BodyForceRecord &R = *A.rec;
    const double i0 = R.integral[0], i1 = R.integral[1];
    const double mdot_old = R.fresh ? A.mdot0 : R.mass_flux; /* :5398-5403 */
    const double ubulk = (i0 == 0.0) ? 0.0 : i1 / i0;        /* :5412-5415 */
    const double mass_flux = ubulk * i0;                     /* :5418 */
    const double f1 = 1.0 / A.area / A.dt * (A.mdot0 - 2.0 * mass_flux + mdot_old); /* :5425 */
    const double f4 = f1 * ubulk;                                                   /* :5428 */
    R.mass_flux = mass_flux;
    R.ubulk = ubulk;
    R.force[0] = f1;
    R.force[1] = f4;
    R.accumulated[0] += f1;
    R.accumulated[1] += f4;
    if (f1 != f1) R.nan = 1; /* :5455 */
    R.fresh = 0;
    if (A.capacity > 0)
    {
      double *row = A.ring + 3 * (R.steps % A.capacity); // the columns of massflux.dat (:5447-5450)
      row[0] = mass_flux;
      row[1] = ubulk;
      row[2] = f1;
    }
    R.steps++;
  }
}

struct AddForceArgs
{
  double *src;                // src_upts (n_upts, n_eles, 5)
  const BodyForceRecord *rec; // the force of the evaluation that runs; nullptr: f1, f4 below (taking a contribution out again)
  double f1, f4;
  long P;
};

template <int W> __device__ inline void add_points(double *p, double f);
template <> __device__ inline void add_points<1>(double *p, double f) { p[0] += f; }
template <> __device__ inline void add_points<2>(double *p, double f)
{
  double2 t = *reinterpret_cast<double2 *>(p);
  t.x += f;
  t.y += f;
  *reinterpret_cast<double2 *>(p) = t;
}

// src_upts(j, i, k) += body_force(k), k = 1 and 4 (:5469-5473; the other three increments are zero).  One thread: W consecutive
// points of both planes, grid-stride; 16-byte accesses for W = 2 (P even: every plane is then 16-byte aligned)
template <int W>
__global__ __launch_bounds__(256) void add_body_force_kernel(const AddForceArgs A)
{
  const double f1 = A.rec ? A.rec->force[0] : A.f1, f4 = A.rec ? A.rec->force[1] : A.f4;
  const long n_items = A.P / W;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < n_items; it += stride)
  {
    const long p = it * W;
    add_points<W>(A.src + A.P + p, f1);
    add_points<W>(A.src + 4 * A.P + p, f4);
  }
}

static int launch_add(hfx_eles *e, const BodyForceRecord *rec, double f1, double f4)
{
  AddForceArgs A{};
  A.src = e->arr[HFX_SRC_UPTS];
  A.rec = rec;
  A.f1 = f1;
  A.f4 = f4;
  A.P = (long)e->n_upts * e->n_eles;
  const int W = (A.P % 2 == 0) ? 2 : 1;
  const long blocks = (A.P / W + 255) / 256;
  const dim3 grid((unsigned)std::max<long>(1, std::min<long>(blocks, 2048))), block(256);
  if (W == 2)
    hipLaunchKernelGGL(add_body_force_kernel<2>, grid, block, 0, e->ctx->stream, A);
  else
    hipLaunchKernelGGL(add_body_force_kernel<1>, grid, block, 0, e->ctx->stream, A);
  HFX_HIP(hipGetLastError());
  return 0;
}

static int launch_control(hfx_eles *e, int what)
{
  BodyForce &B = *e->body_force;
  ControlArgs C{};
  C.partial = B.partial;
  C.rec = B.record;
  C.ring = B.ring;
  C.n_groups = B.n_groups;
  C.capacity = B.capacity;
  C.what = what;
  C.area = B.area;
  C.mdot0 = B.mdot0;
  C.dt = e->ctx->params.dt;
  hipLaunchKernelGGL(body_force_kernel, dim3(1), dim3(256), 0, e->ctx->stream, C);
  HFX_HIP(hipGetLastError());
  return 0;
}

// the device address of the record's two integrals
static double *record_integral(const BodyForce &B)
{
  static_assert(offsetof(BodyForceRecord, integral) == 0, "integral leads the record");
  return reinterpret_cast<double *>(B.record.get());
}

// the first kernel of an evaluation (and what must hold before it): the partials of this rank's faces
static int integrate_inflow(hfx_eles *e)
{
  hfx_ctx *ctx = e->ctx;
  BodyForce &B = *e->body_force;
  HFX_CHECK(ctx->have_params, "parameters not set");
  HFX_CHECK(ctx->params.dt_type != 2, "Not sure what value of timestep to use in body force term when using local timestepping."); /* :5409 */
  if (!e->arr[HFX_SRC_UPTS])
  {
    // (the first evaluation of a block whose caller uploaded no source term; hipMemset: once, not per step)
    if (e->arr[HFX_SRC_UPTS].alloc_zeroed(e->arr_len[HFX_SRC_UPTS])) return 1;
    B.own_src = true;
  }
  e->src_nonzero = true;
  if (B.n_faces == 0) return 0;
  MassFluxArgs M{};
  M.disu_upts = e->arr[HFX_DISU_UPTS0];
  M.weights = B.weights;
  M.face_ele = B.face_ele;
  M.partial = B.partial;
  M.P = (long)e->n_upts * e->n_eles;
  M.n_upts = e->n_upts;
  M.n_faces = B.n_faces;
  hipLaunchKernelGGL(mass_flux_kernel, dim3(B.n_groups), dim3(64 * BF_FACES_PER_GROUP), 0, ctx->stream, M);
  HFX_HIP(hipGetLastError());
  return 0;
}

// this rank's integrals on the host (waits for the compute stream)
static int local_integrals(hfx_eles *e, double integral[2])
{
  if (integrate_inflow(e) || launch_control(e, BF_SUM)) return 1;
  HFX_HIP(hipMemcpyAsync(integral, record_integral(*e->body_force), 2 * sizeof(double), hipMemcpyDeviceToHost, e->ctx->stream));
  HFX_HIP(hipStreamSynchronize(e->ctx->stream));
  return 0;
}

// the controller and the addition from integrals summed over the ranks
static int apply_integrals(hfx_eles *e, const double integral[2])
{
  BodyForce &B = *e->body_force;
  B.h_integral[0] = integral[0];
  B.h_integral[1] = integral[1];
  HFX_HIP(hipMemcpyAsync(record_integral(B), B.h_integral, 2 * sizeof(double), hipMemcpyHostToDevice, e->ctx->stream));
  if (launch_control(e, BF_CONTROL)) return 1;
  return launch_add(e, B.record, 0.0, 0.0);
}

// eles::evaluate_body_force for one block, which the step loop calls in front of a step's first stage (step_loop.hpp has the contract)
int evaluate_body_force(hfx_eles *e, hfx_comm *comm)
{
  if (!e->body_force || e->n_eles == 0) return 0; /* :5285 */
  if (comm)
  {
    double v[2];
    if (local_integrals(e, v) || hfx_comm_allreduce(comm, v, 2, 2)) return 1;
    return apply_integrals(e, v);
  }
  if (integrate_inflow(e) || launch_control(e, BF_SUM | BF_CONTROL)) return 1;
  return launch_add(e, e->body_force->record, 0.0, 0.0);
}

// the record of e's controller on the host (waits for the compute stream)
static int read_record(hfx_eles *e, BodyForceRecord &r)
{
  HFX_HIP(hipStreamSynchronize(e->ctx->stream));
  HFX_HIP(hipMemcpy(&r, e->body_force->record, sizeof(r), hipMemcpyDeviceToHost));
  return 0;
}

// what the controller has put into src_upts so far goes out again (a new registration starts from a zero contribution)
static int drop_body_force(hfx_eles *e)
{
  if (!e->body_force) return 0;
  BodyForce &B = *e->body_force;
  BodyForceRecord r;
  if (read_record(e, r)) return 1;
  if (r.steps > 0 && e->arr[HFX_SRC_UPTS])
  {
    if (B.own_src)
    {
      e->arr[HFX_SRC_UPTS].reset();
      e->src_nonzero = false;
    }
    else
    {
      if (launch_add(e, nullptr, -r.accumulated[0], -r.accumulated[1])) return 1;
      HFX_HIP(hipStreamSynchronize(e->ctx->stream));
    }
  }
  e->body_force.reset();
  return 0;
}

} // namespace hfx

using namespace hfx;

extern "C" {

int hfx_eles_set_body_force(hfx_eles *e, int n_faces, const int *face_ele, const int *face_inter, int n_inters_per_ele,
                            const int *n_cubpts_per_inter, const double *const *opp_inters_cubpts,
                            const double *const *weight_inters_cubpts, const double *inter_detjac_inters_cubpts, double area,
                            double mdot0, int history_capacity)
{
  HFX_CHECK(e, "hfx_eles_set_body_force: NULL eles");
  HFX_CHECK(e->n_dims == 3 && e->n_fields == 5, "hfx_eles_set_body_force: the body force is built for three-dimensional Navier-Stokes "
                                                "blocks (n_dims 3, n_fields 5; src/solver.cpp:96), this block has n_dims %d, n_fields %d",
            e->n_dims, e->n_fields);
  HFX_CHECK(n_faces >= 0 && history_capacity >= 0, "hfx_eles_set_body_force: %d faces, history capacity %d", n_faces, history_capacity);
  HFX_CHECK(n_faces == 0 || (face_ele && face_inter && n_cubpts_per_inter && opp_inters_cubpts && weight_inters_cubpts &&
                             inter_detjac_inters_cubpts),
            "hfx_eles_set_body_force: NULL argument");
  HFX_CHECK(n_faces == 0 || n_inters_per_ele > 0, "hfx_eles_set_body_force: %d local faces per element", n_inters_per_ele);
  HFX_CHECK(area != 0.0 && area == area && mdot0 == mdot0, "hfx_eles_set_body_force: area %g, mdot0 %g", area, mdot0);
  for (int f = 0; f < n_faces; f++)
  {
    HFX_CHECK(face_ele[f] >= 0 && face_ele[f] < e->n_eles, "hfx_eles_set_body_force: face %d names element %d of %d", f, face_ele[f], e->n_eles);
    HFX_CHECK(face_inter[f] >= 0 && face_inter[f] < n_inters_per_ele, "hfx_eles_set_body_force: face %d names local face %d of %d", f,
              face_inter[f], n_inters_per_ele);
    const int l = face_inter[f];
    HFX_CHECK(n_cubpts_per_inter[l] > 0 && opp_inters_cubpts[l] && weight_inters_cubpts[l],
              "hfx_eles_set_body_force: local face %d has no surface cubature", l);
  }
  HFX_IMMEDIATE(e->ctx, 0);
  if (drop_body_force(e)) return 1;

  auto B = std::make_unique<BodyForce>();
  B->n_faces = n_faces;
  B->n_groups = (n_faces + BF_FACES_PER_GROUP - 1) / BF_FACES_PER_GROUP;
  B->capacity = history_capacity;
  B->area = area;
  B->mdot0 = mdot0;
  // c(k, face) = sum_j w_j detjac(j, face) opp(j, k), j ascending
  std::vector<double> c((size_t)e->n_upts * n_faces);
  const double *dj = inter_detjac_inters_cubpts;
  for (int f = 0; f < n_faces; f++)
  {
    const int l = face_inter[f], nc = n_cubpts_per_inter[l];
    const double *opp = opp_inters_cubpts[l], *w = weight_inters_cubpts[l];
    for (int k = 0; k < e->n_upts; k++)
    {
      double t = 0.0;
      for (int j = 0; j < nc; j++) t += w[j] * dj[j] * opp[j + (size_t)nc * k];
      c[k + (size_t)e->n_upts * f] = t;
    }
    dj += nc;
  }
  if (B->weights.upload(c)) return 1;
  if (B->face_ele.upload(face_ele, (size_t)n_faces)) return 1;
  if (B->partial.alloc_zeroed(2 * (size_t)B->n_groups)) return 1;
  if (B->ring.alloc_zeroed(3 * (size_t)history_capacity)) return 1;
  BodyForceRecord r{};
  r.fresh = 1;
  if (B->record.upload(&r, 1)) return 1;
  e->body_force = std::move(B);
  return 0;
}

int hfx_eles_clear_body_force(hfx_eles *e)
{
  HFX_CHECK(e, "hfx_eles_clear_body_force: NULL eles");
  HFX_IMMEDIATE(e->ctx, 0);
  return drop_body_force(e);
}

int hfx_eles_evaluate_body_force(hfx_eles *e)
{
  HFX_CHECK(e, "hfx_eles_evaluate_body_force: NULL eles");
  HFX_CHECK(e->body_force, "hfx_eles_evaluate_body_force: no body force registered (hfx_eles_set_body_force)");
  // (the stage that has been recorded leaves disu_upts(0) of the new state whichever way it runs)
  HFX_IMMEDIATE(e->ctx, 0);
  return evaluate_body_force(e, nullptr);
}

int hfx_time_body_force_kernels(hfx_eles *e, int reps, double ms[3])
{
  HFX_CHECK(e && ms && reps > 0, "hfx_time_body_force_kernels: bad argument");
  HFX_CHECK(e->body_force, "hfx_time_body_force_kernels: no body force registered (hfx_eles_set_body_force)");
  HFX_IMMEDIATE(e->ctx, 0);
  hipStream_t st = e->ctx->stream;
  hipEvent_t ev[4];
  for (auto &x : ev) HFX_HIP(hipEventCreate(&x));
  double acc[3] = {0.0, 0.0, 0.0};
  // 0 fine, 1 a launcher failed (its message stands), 2 an event call failed
  auto once = [&]() -> int {
    if (hipEventRecord(ev[0], st) != hipSuccess) return 2;
    if (integrate_inflow(e)) return 1;
    if (hipEventRecord(ev[1], st) != hipSuccess) return 2;
    if (launch_control(e, BF_SUM | BF_CONTROL)) return 1;
    if (hipEventRecord(ev[2], st) != hipSuccess) return 2;
    if (launch_add(e, e->body_force->record, 0.0, 0.0)) return 1;
    if (hipEventRecord(ev[3], st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return 2;
    for (int k = 0; k < 3; k++)
    {
      float t = 0.f;
      if (hipEventElapsedTime(&t, ev[k], ev[k + 1]) != hipSuccess) return 2;
      acc[k] += t;
    }
    return 0;
  };
  int rc = 0;
  for (int r = 0; r < reps && !rc; r++) rc = once();
  for (auto &x : ev) (void)hipEventDestroy(x);
  if (rc == 2) set_error("hfx_time_body_force_kernels: a HIP event call failed");
  if (rc) return 1;
  for (int k = 0; k < 3; k++) ms[k] = acc[k] / reps;
  return 0;
}

int hfx_eles_body_force_integrals(hfx_eles *e, double integral[2])
{
  HFX_CHECK(e && integral, "hfx_eles_body_force_integrals: NULL argument");
  HFX_CHECK(e->body_force, "hfx_eles_body_force_integrals: no body force registered (hfx_eles_set_body_force)");
  HFX_IMMEDIATE(e->ctx, 0);
  if (e->n_eles == 0)
  {
    integral[0] = integral[1] = 0.0;
    return 0;
  }
  return local_integrals(e, integral);
}

int hfx_eles_body_force_apply(hfx_eles *e, const double integral[2])
{
  HFX_CHECK(e && integral, "hfx_eles_body_force_apply: NULL argument");
  HFX_CHECK(e->body_force, "hfx_eles_body_force_apply: no body force registered (hfx_eles_set_body_force)");
  HFX_CHECK(e->ctx->params.dt_type != 2, "Not sure what value of timestep to use in body force term when using local timestepping.");
  HFX_CHECK(e->n_eles == 0 || e->arr[HFX_SRC_UPTS], "hfx_eles_body_force_apply: call hfx_eles_body_force_integrals first");
  HFX_IMMEDIATE(e->ctx, 0);
  if (e->n_eles == 0) return 0;
  return apply_integrals(e, integral);
}

int hfx_eles_body_force_state(hfx_eles *e, double *mass_flux, double *ubulk, double *body_force_x, double accumulated[2],
                              double integral[2], long *n_steps)
{
  HFX_CHECK(e, "hfx_eles_body_force_state: NULL eles");
  HFX_CHECK(e->body_force, "hfx_eles_body_force_state: no body force registered (hfx_eles_set_body_force)");
  HFX_IMMEDIATE(e->ctx, 0);
  BodyForceRecord r;
  if (read_record(e, r)) return 1;
  if (mass_flux) *mass_flux = r.mass_flux;
  if (ubulk) *ubulk = r.ubulk;
  if (body_force_x) *body_force_x = r.force[0];
  if (accumulated) { accumulated[0] = r.accumulated[0]; accumulated[1] = r.accumulated[1]; }
  if (integral) { integral[0] = r.integral[0]; integral[1] = r.integral[1]; }
  if (n_steps) *n_steps = (long)r.steps;
  HFX_CHECK(!r.nan, "ERROR: NaN body force, exiting"); /* src/eles.cpp:5457 */
  return 0;
}

int hfx_eles_body_force_history(hfx_eles *e, int max_rows, double *rows, int *n_rows)
{
  HFX_CHECK(e && n_rows && (max_rows == 0 || rows) && max_rows >= 0, "hfx_eles_body_force_history: bad argument");
  HFX_CHECK(e->body_force, "hfx_eles_body_force_history: no body force registered (hfx_eles_set_body_force)");
  HFX_IMMEDIATE(e->ctx, 0);
  BodyForce &B = *e->body_force;
  BodyForceRecord r;
  if (read_record(e, r)) return 1;
  const long kept = std::min<long>((long)r.steps, B.capacity);
  *n_rows = (int)kept;
  if (kept == 0 || max_rows == 0) return 0;
  std::vector<double> ring(3 * (size_t)B.capacity);
  HFX_HIP(hipMemcpy(ring.data(), B.ring, sizeof(double) * ring.size(), hipMemcpyDeviceToHost));
  // the newest min(max_rows, kept) rows, oldest first
  const long n = std::min<long>(kept, max_rows);
  for (long i = 0; i < n; i++)
  {
    const long step = (long)r.steps - n + i;
    std::copy(ring.begin() + 3 * (step % B.capacity), ring.begin() + 3 * (step % B.capacity) + 3, rows + 3 * i);
  }
  *n_rows = (int)n;
  return 0;
}

} // extern "C"
