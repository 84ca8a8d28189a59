// hfx_internal.hpp -- internal types of libhfx (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "../../include/hfx.h"
#include "physics.hpp"
#include "plot_point.hpp"

namespace hfx
{

void set_error(const char *fmt, ...);
struct FusedData;
struct GeneralData;
struct Simplex2dData;
struct TensorOps;
// (the four are complete in their own translation units only: fused_hex.hip, general.hip, simplex2d.hip, tensor_ops.hip)
struct FusedDelete { void operator()(FusedData *p) const; };
struct GeneralDelete { void operator()(GeneralData *p) const; };
struct Simplex2dDelete { void operator()(Simplex2dData *p) const; };
struct TensorOpsDelete { void operator()(TensorOps *p) const; };

#define HFX_HIP(call)                                                                          \
  do                                                                                           \
  {                                                                                            \
    hipError_t _e = (call);                                                                    \
    if (_e != hipSuccess)                                                                      \
    {                                                                                          \
      hfx::set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #call, hipGetErrorString(_e)); \
      return 1;                                                                                \
    }                                                                                          \
  } while (0)

#define HFX_CHECK(cond, ...)       \
  do                               \
  {                                \
    if (!(cond))                   \
    {                              \
      hfx::set_error(__VA_ARGS__); \
      return 1;                    \
    }                              \
  } while (0)

// the bytes all live DevBufs of the process hold (hfx_live_device_bytes_internal)
inline std::atomic<long> g_live_device_bytes{0};

// One device allocation and its owner (move-only): the only place of the library that allocates or frees device memory.
// At least one element is allocated, so a buffer of an empty block still has an address.  Converts to T*: kernel argument
// structs and the launchers read it as the plain pointer it holds.
template <class T>
class DevBuf
{
  T *p_ = nullptr;
  size_t n_ = 0; // elements allocated

public:
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept
  {
    if (this != &o)
    {
      reset();
      std::swap(p_, o.p_);
      std::swap(n_, o.n_);
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  void reset()
  {
    if (!p_) return;
    (void)hipFree(p_);
    g_live_device_bytes -= (long)(sizeof(T) * n_);
    p_ = nullptr;
    n_ = 0;
  }
  // what it held goes; a failed allocation leaves the buffer empty
  int alloc(size_t n)
  {
    reset();
    n = std::max<size_t>(n, 1);
    void *q = nullptr;
    HFX_HIP(hipMalloc(&q, sizeof(T) * n));
    p_ = (T *)q;
    n_ = n;
    g_live_device_bytes += (long)(sizeof(T) * n_);
    return 0;
  }
  int alloc_zeroed(size_t n)
  {
    if (alloc(n)) return 1;
    HFX_HIP(hipMemset(p_, 0, sizeof(T) * n_));
    return 0;
  }
  // allocated on first use
  int ensure(size_t n) { return p_ ? 0 : alloc(n); }
  int ensure_zeroed(size_t n) { return p_ ? 0 : alloc_zeroed(n); }
  int upload(const T *src, size_t n)
  {
    if ((!p_ || n_ != std::max<size_t>(n, 1)) && alloc(n)) return 1;
    if (n) HFX_HIP(hipMemcpy(p_, src, sizeof(T) * n, hipMemcpyHostToDevice));
    return 0;
  }
  int upload(const std::vector<T> &v) { return upload(v.data(), v.size()); }

  T *get() const { return p_; }
  size_t size() const { return n_; }
  explicit operator bool() const { return p_ != nullptr; }
  operator T *() const { return p_; }
};

// One registered operator matrix (m x k, column-major) on the device, in the
// forms the contraction kernels consume.
struct Operator
{
  int m = 0, k = 0;
  DevBuf<double> dense; // (m,k) column-major
  // the same zero-padded to whole MFMA tiles, (mpad, kpad) column-major with mpad = 16 ceil(m/16), kpad = 4 ceil(k/4): the
  // dense contraction kernels read operator fragments from it without bounds checks
  DevBuf<double> dense_pad;
  int mpad = 0, kpad = 0;
  // ELL form: exact non-zeros of every row in ASCENDING column order (the
  // reference dgemm sums l ascending, src/funcs.cpp:110-117), padded with
  // (val 0, col = first column of the row).  Row-interleaved: entry q of row r
  // at [r + m*q].
  int nnz_max = 0;
  DevBuf<double> ell_val;
  DevBuf<int> ell_idx;
  long nnz_total = 0;
  std::vector<double> h_val; // host copy of the ELL arrays (width max(nnz_max,1), row-interleaved)
  std::vector<int> h_idx;
  bool present() const { return (bool)dense; }
};

} // namespace hfx

struct hfx_inters;
struct hfx_comm;

namespace hfx
{
// ---- deferred execution (deferred.hip) -------------------------------------------------------------------------------
// With the option "deferred" the per-method entry points -- the calls CalcResidual (src/solver.cpp:59-221) and the RK loop
// (src/HiFiLES.cpp:201-217) make -- are RECORDED instead of launched.  When the record is complete (the next stage begins,
// or any other entry point needs the device state) it is compared with CalcResidual's canonical order: a whole stage runs as
// the split / general / partitioned fused stage, anything else is replayed call by call.
enum DeferMethod
{
  DM_CALC_SGS_TERMS = 0, DM_EXTRAPOLATE_SOLUTION, DM_MPI_SEND_SOLUTION, DM_CALCULATE_GRADIENT, DM_EVALUATE_INVFLUX,
  DM_INT_COMMON_INVFLUX, DM_BDY_INVFLUX, DM_MPI_RECEIVE_SOLUTION, DM_MPI_COMMON_INVFLUX, DM_CORRECT_GRADIENT,
  DM_MPI_SEND_GRADIENT, DM_EVALUATE_VISCFLUX, DM_EXTRAPOLATE_SGSFLUX, DM_MPI_SEND_SGSF, DM_EXTRAPOLATE_TOTALFLUX,
  DM_CALCULATE_DIVERGENCE, DM_INT_COMMON_VISCFLUX, DM_BDY_VISCFLUX, DM_MPI_RECEIVE_GRADIENT, DM_MPI_RECEIVE_SGSF,
  DM_MPI_COMMON_VISCFLUX, DM_CORRECTED_DIVERGENCE, DM_ADVANCE_SOLUTION, DM_SHOCK_CAPTURE, DM_N_METHODS,
  // not a method of the stage: `run_input.ramp_counter++` between two time steps (src/HiFiLES.cpp:224-225).  Recorded behind a
  // whole stage so that it does not force that stage to run before the caller has said what it wants of it; applied after it
  DM_SET_RAMP_COUNTER = DM_N_METHODS
};
struct DeferCall
{
  int method = 0;         // DeferMethod; the enumeration is in CalcResidual's order, so it doubles as the call's phase
  hfx_eles *e = nullptr;  // element-block methods
  hfx_inters *f = nullptr; // face-block methods
  hfx_comm *c = nullptr;  // send_* / receive_*
  int i0 = 0, i1 = 0;     // AdvanceSolution: in_step, adv_type; evaluate_invFlux: 1 = the over-integration form; ramp counter: value
};
struct DeferPlan
{
  std::vector<DeferCall> signature; // the record this plan was made for (methods and objects; stage number excluded)
  enum class Kind { replay, split, split_partitioned, general, general_partitioned }; // call by call, or as one of the fused stages
  Kind kind = Kind::replay;
  bool partitioned() const { return kind == Kind::split_partitioned || kind == Kind::general_partitioned; }
  std::string why;                  // Kind::replay: why the record is not run as a fused stage
  std::vector<hfx_eles *> eles;
  std::vector<hfx_inters *> faces, mpi_faces; // interior + boundary blocks | partition-face blocks
  hfx_comm *comm = nullptr;
  bool sgs_terms = false, shock = false;
};
struct Deferred
{
  bool on = false;   // option "deferred"
  bool busy = false; // a flush / replay / immediate entry point is running: calls execute at once
  std::vector<DeferCall> log;
  std::vector<DeferPlan> plans; // one per distinct record seen (a run has one or two)
  long n_fused = 0, n_replayed = 0; // stages run fused | records replayed call by call (hfx_ctx_deferred_stats)
  std::string last_why;
};
} // namespace hfx

struct hfx_ctx
{
  int device = 0;
  hipStream_t stream = nullptr;
  // a second stream for the boundary-face kernels of the fused stages, which then run BESIDE the pairwise interior-face kernel
  // (side_stream_fork: the side stream waits for what the main stream holds so far and boundary launches go there;
  // side_stream_join: launches go to the main stream again; side_stream_wait: the main stream waits for the side stream)
  hipStream_t side_stream = nullptr, bdy_stream = nullptr;
  hipEvent_t side_fork = nullptr, side_done = nullptr;
  hfx_params params{};
  bool have_params = false;
  int contract_mode = HFX_CONTRACT_AUTO;
  int fused_mode = 3; // which split variant hfx_time_fused_kernels / hfx_fused_kernel_bytes / hfx_stage_partitioned use (2 or 3)
  int n_cu = 256;
  // measurement knobs (hfx_ctx_set_option): kernel variants that give the same results; defaults are the product path
  struct Options
  {
    int split_grid_per_cu = 0;  // persistent workgroups per CU of the split element kernels; 0: as many as are resident
    int flux_grid_per_cu = 0;   // the same for the loader-wave flux kernel alone (0: split_grid_per_cu)
    int persistent_grid_cap = 0; // n > 0: no persistent element kernel is launched with more than n workgroups (persistent_grid); tests make small meshes loop with it
    int xcd_order = 1;          // workgroups of one XCD walk one contiguous eighth of the elements
    int dictionary_rows = 0;    // 1: the dictionary-row flux kernel even when the operators are tensor products
    int flux_waves = 2;         // waves per SIMD the sum-factorised flux kernel is launched for (2 or 3)
    int buffer_addressing = 1;  // buffer-descriptor addressing where every array is below 4 GiB
    int split_flux = 1;         // hfx_run_steps_partitioned: the flux kernel in three launches (half of the elements without partition-face points | those with | the other half)
    int split_update = 1;       // hfx_run_steps_partitioned: the update kernel in two launches, partition-face elements first (their exchange hidden behind the rest)
    int comm_stream_faces = 1;  // hfx_run_steps_partitioned: partition-face kernels on the communication stream, beside the interior ones
    int fold_general = 1;       // general fused stage: opp_3 norm_tdisf folded into the divergence operator (no norm_tdisf traffic)
    int gather_delta = 1;       // the loader-wave flux kernel forms the LDG corrections of interior points itself (no face_delta launch)
    int loader_wave = 1;        // the LDS-DMA loader wave of the flux kernel where the element size fits
    int simd_roles = 1;         // 1: the flux kernel deals its waves' parts by SIMD (one heavy wave per SIMD)
    int flux_stamps = 0;        // 1: phase time stamps of one workgroup of the flux kernel (printed by hfx_time_fused_kernels)
    int tensor_ops = 1;         // sum-factorised over-integration / shock capturing on tensor-product classes
    int dense_waves = 0;        // waves per workgroup of the dense MFMA contraction: 0 by the operator's rows, else 4 or 8
    int dense_split = 0;        // column groups per 16-row tile dealt to the waves: 0 by the operator's rows, else 1, 2 or 4
    int general_update_waves = 0; // waves per workgroup of the general stage's update kernel: 0 by the staging registers, else 4 or 8
    int over_int_fold = 1;      // 1: with the loader-wave flux kernel the over-integration kernel hands over its contribution to the divergence (n_fields values per point), not tdisf_upts
    int light_wave_short = 1;   // 1: a flux-kernel wave without solution points runs the flux-point physics alone (not the paired form)
    int bdy_beside = 0;         // 1: the fused stages' viscous boundary-face kernels run on a side stream beside the interior-face kernel (measured neutral: off)
    int les_flux_kernel = 1;    // 1: the LES closure is evaluated in the flux kernel of split variant 3 where its loader-wave form runs
    int affine_metrics = 1;     // 1: on an affine block (every element a parallelepiped) the split stage's flux and update kernels read a 34-double metric record per element in place of most per-point metric arrays
    int flux_two_wave = 1;      // 1: the affine flux kernel of P4 hexahedra as two-wave workgroups, four resident per CU (0: its loader-wave form)
    int fold_faces = 1;         // 1: with one-sided LDG (|ldg_beta| = 1/2; not with RoeM) the two-wave flux kernel forms the interior pairs' common flux itself and the stage launches no face_flux2_kernel on interior faces (0: the three-launch stage)
    int flux_two_wave_face = -1; // the local face that carries the two-wave flux kernel's left-over points: -1 the host's choice (two_wave_face), 0-5 forced (tests: reaches the left-over pass of phase B)
    int general_waves = 0;      // waves per workgroup of the general flux kernel: 0 by the LDS image (4 or 8), else 3, 4 or 8
    int fold_over_int = 1;      // 1: the 2-D simplex stage's element kernel carries a triangle block's over-integration (its OVERINT instantiation); 0: hfx_eles_evaluate_invFlux_over_int in front of the element kernel, which reads tdisf_upts
    int fold_shock = 1;         // 1: the 2-D simplex stage's update kernel carries a triangle block's shock filter (sensor of eles_tris::shock_det_persson); 0: the per-method filter behind the stage, as on tetrahedra and prisms
    int blocks_2d = 0;          // 1: the 2-D simplex stage (fused 4) takes several two-dimensional blocks -- a mixed quadrilateral / triangle mesh, several triangle blocks -- and a block of quadrilaterals of orders 1..4 (its plain kernels; cross blocks' LDG corrections by face_delta_kernel); 0: those calls are refused as ever
  } opt;
  hfx::Deferred defer;
  std::vector<hfx_comm *> comms; // the live communicators of this context (hfx_ctx_synchronize waits for their streams)
  double CFL = 0.0; // run_input.CFL (hfx_ctx_set_CFL); dt_type 1 / 2 only
  bool have_CFL = false;
  // the clock of the step loops (hfx_ctx_set_clock): FlowSol.time, i_steps and run_input.spinup_time of src/HiFiLES.cpp:221-243.
  // have_clock: the loops advance it and update the time averages after every step (hfx::end_of_step)
  double time = 0.0, spinup_time = 0.0;
  int i_steps = 0;
  bool have_clock = false;
  // point probes (hfx_ctx_set_probes): the fields of every block's samples, the sampling frequency in steps and the samples a
  // block's device history holds.  probe_epoch: counts the registrations; a block whose history was made for another one makes it anew
  int n_probe_fields = 0, probe_freq = 1, probe_capacity = 0;
  int probe_codes[HFX_MAX_PROBE_FIELDS] = {};
  unsigned long probe_epoch = 0;
  // the integral monitor (hfx_ctx_set_integral_monitor): run_input.integral_quantities as the ids of hfx_eles_CalcIntegralQuantities,
  // run_input.monitor_res_freq and the samples a block's device history holds.  iq_epoch: as probe_epoch
  int n_iq = 0, iq_freq = 1, iq_capacity = 0;
  int iq_ids[8] = {};
  unsigned long iq_epoch = 0;
  // the history monitor (hfx_ctx_set_history_monitor): run_input.res_norm_type, whether the rows carry the wall forces,
  // run_input.monitor_res_freq and the rows a block's device history holds.  hist_epoch: as probe_epoch
  bool hist_on = false, hist_forces = false;
  int hist_norm = 2, hist_freq = 1, hist_capacity = 0;
  unsigned long hist_epoch = 0;
  // the plot monitor (hfx_ctx_set_plot_monitor): run_input.diagnostic_fields as hfx_plot_field codes in the caller's order,
  // run_input.plot_freq and the snapshots a block's device history holds.  plot_epoch: as probe_epoch
  bool plot_on = false;
  int n_plot_diag = 0, plot_freq = 1, plot_capacity = 0;
  int plot_codes[16] = {};
  unsigned long plot_epoch = 0;
  // the exact solution of the error monitor (hfx_ctx_set_exact_solution): run_input.test_case and what eval_couette_flow takes
  hfx_exact exact{};
  bool have_exact = false;
  // the reference state of the wall-force monitor (hfx_ctx_set_force_reference) and what eles::compute_wall_forces forms from it
  // (src/eles.cpp:5733-5743): factor = 1 / (0.5 rho |u|^2), aoa = atan2(v, u), aos = atan2(w, u)
  hfx_force_ref force_ref{};
  double force_factor = 0.0, force_aoa = 0.0, force_aos = 0.0;
  bool have_force_ref = false;
  // the wall model (hfx_ctx_set_wall_model): run_input.wall_model (0 off, 1 Werner-Wengle, 2 Breuer-Rodi), prandtl_t, Kappa
  int wall_model = 0;
  double wm_prandtl_t = 0.9, wm_Kappa = 0.41;
  hfx::Phys phys() const
  {
    hfx::Phys P;
    P.gamma = params.gamma;
    P.prandtl = params.prandtl;
    P.rt_inf = params.rt_inf;
    P.mu_inf = params.mu_inf;
    P.c_sth = params.c_sth;
    P.fix_vis = params.fix_vis;
    P.ldg_beta = params.ldg_beta;
    P.ldg_tau = params.ldg_tau;
    P.riemann = params.riemann_solve_type;
    P.viscous = params.viscous;
    return P;
  }
};

namespace hfx
{
// The launches of the persistent element kernels since the block's last fused stage began (persistent_grid), in launch order
// (hfx_fused_launch_grids): the slot of hfx_time_fused_kernels, the grid, the elements or list entries the launch walks
struct LaunchLog
{
  static constexpr int MAX = 16;
  int n = 0;
  int slot[MAX] = {}, grid[MAX] = {};
  long work[MAX] = {};
};
} // namespace hfx

namespace hfx
{
// The controller of the mass-flux body force (forcing.hip; eles::evaluate_body_force, src/eles.cpp:5281-5482) as it lives on the
// device: what the three kernels of an evaluation hand to each other and what the state queries download
struct BodyForceRecord
{
  double integral[2];    // integral(0), integral(1) of the last evaluation (over all ranks)
  double mass_flux, ubulk;
  double force[2];       // body_force(1), body_force(4) of the last evaluation
  double accumulated[2]; // their sums since the registration: what src_upts holds of the controller
  long long steps;       // evaluations since the registration
  int nan;               // a body_force(1) was NaN (src/eles.cpp:5455)
  int fresh;             // no evaluation yet: mdot_old = mdot0 (src/eles.cpp:5398-5401)
};
struct BodyForce
{
  int n_faces = 0, n_groups = 0, capacity = 0;
  double area = 0.0, mdot0 = 0.0;
  bool own_src = false;            // HFX_SRC_UPTS was allocated by the first evaluation (the caller uploaded none)
  DevBuf<double> weights;          // c (n_upts, n_faces)
  DevBuf<int> face_ele;            // (n_faces)
  DevBuf<double> partial;          // (2, n_groups)
  DevBuf<BodyForceRecord> record;  // one
  DevBuf<double> ring;             // (3, capacity): mass_flux, ubulk, body_force(1) of the last `capacity` evaluations
  double h_integral[2] = {};       // several ranks: the integrals on their way through the all-reduce
};
} // namespace hfx

namespace hfx
{
// The point probes of one block (probes.hip), sorted by element: position i of the sorted order is probe dest[i] of the caller
struct Probes
{
  int n = 0;
  DevBuf<double> opp;     // (n_upts, n) operator rows, sorted order
  DevBuf<int> ele, dest;  // (n) element | the caller's index, sorted order
  // (n_fields, n, capacity + 1): the samples in the caller's order; the last slot is the scratch of hfx_time_probes
  DevBuf<double> history;
  int n_fields = 0, capacity = 0; // what `history` was made for
  unsigned long epoch = 0;        // ctx->probe_epoch it was made at
  std::vector<double> times;      // of the stored samples; their number is the number of stored samples
  std::vector<int> steps;
};
} // namespace hfx

namespace hfx
{
// The wall faces of one block (wall_force.hip), sorted by (local face, element): position s of the sorted order is face
// first[s] / n_cubpts of the caller's packed per-point arrays
struct WallForces
{
  int n_faces = 0, n_inters = 0, max_cubpts = 0;
  long n_points = 0;               // the sum of the faces' cubature points
  DevBuf<int> ele, inter, dual;    // (n_faces) sorted order: element | local face | 1 = SLIP_WALL_DUAL
  DevBuf<long> first;              // (n_faces) sorted order: where the face's points begin in detjac / norm / cp_cf
  DevBuf<int> n_cubpts;            // (n_inters) per local face
  DevBuf<long> opp_first, weight_first; // (n_inters) where local face l begins in opp / weight
  DevBuf<double> opp, weight;      // the local faces' (n_cubpts, n_upts) column-major operators | weights, one behind the other
  DevBuf<double> detjac, norm;     // the caller's packed arrays: (n_points) | per face (n_cubpts, n_dims) column-major
  DevBuf<double> cp_cf;            // (n_points, 2): Cp and Cf of the last call, the caller's order
  DevBuf<double> partial;          // (n_groups, 2 n_dims + 2) of the call that runs
};
} // namespace hfx

namespace hfx
{
// The integral-quantity history of one block (integrals.hip)
struct IntegralHistory
{
  // (n_quantities, capacity + 1): sample s at [n_quantities * s]; the last slot is the scratch of hfx_time_integral_quantities
  DevBuf<double> history;
  DevBuf<double> partial;         // (n_groups, n_quantities) of the sample that runs
  int n_quantities = 0, capacity = 0; // what `history` was made for
  unsigned long epoch = 0;        // ctx->iq_epoch it was made at
  std::vector<double> times;      // of the stored samples; their number is the number of stored samples
  std::vector<int> steps;
};
// The history rows of one block (history.hip): the residual of every field, then (the monitor with forces) the 2 n_dims + 2 values of
// hfx_eles_compute_wall_forces
struct HistoryRows
{
  // (n_res + n_force, capacity + 1): row s at [(n_res + n_force) * s]; the last slot is the scratch of hfx_time_history
  DevBuf<double> rows;
  DevBuf<double> partial;         // (n_groups, n_res) of the residual kernel of the sample that runs
  int n_res = 0, n_force = 0, capacity = 0; // what `rows` was made for
  unsigned long epoch = 0;        // ctx->hist_epoch it was made at
  std::vector<double> times;      // of the stored rows; their number is the number of stored rows
  std::vector<int> steps;
};
// The plot-file snapshots of one block (plot_fields.hip): per plot point the conserved fields, the registered average fields and the
// monitor's diagnostic fields, field planes apart as disu_ppts lies
struct PlotHistory
{
  DevBuf<double> history;         // (n_ppts, n_eles, n_out, capacity): snapshot s at [n_ppts * n_eles * n_out * s]
  DevBuf<double> scratch;         // one snapshot: hfx_eles_calc_plot_fields, hfx_time_plot_fields
  int n_ppts = 0, n_average = 0, n_out = 0, capacity = 0; // what `history` was made for
  unsigned long epoch = 0;        // ctx->plot_epoch it was made at
  std::vector<double> times;      // of the stored snapshots; their number is the number of stored snapshots
  std::vector<int> steps;
};
} // namespace hfx

struct hfx_eles
{
  hfx_ctx *ctx = nullptr;
  mutable hfx::LaunchLog launch_log;
  int n_eles = 0, n_upts = 0, n_fpts = 0, n_fields = 0, n_dims = 0, ele_type = 0, order = 0;
  bool viscous_ops = false;
  hfx::DevBuf<double> h_ref; // (n_eles) eles::h_ref for calc_dt_local
  // LES closure (hfx_eles_set_les)
  bool les_ready = false;
  unsigned les_serial = 0; // counts hfx_eles_set_les / hfx_eles_set_les_filter calls (the 2-D simplex stage's tables are one registration's)
  hfx::LesParams les{};
  hfx::DevBuf<double> wall_distance, Jacobian_fpts;
  // similarity-type closures (sgs_model 2, 3, 4): the filter matrix and the work arrays of calc_sgs_terms
  hfx::Operator filter_upts;
  hfx::DevBuf<double> sgs_uu, sgs_ue;
  // integral diagnostics (hfx_eles_set_volume_cubpts)
  int n_vol_cubpts = 0;
  hfx::Operator opp_volume_cubpts;
  hfx::DevBuf<double> weight_volume_cubpts, vol_detjac_vol_cubpts, iq_u, iq_g;
  hfx::DevBuf<int> iq_ids; // the quantity ids of the call that runs
  // the samples of the context's integral monitor (hfx_ctx_set_integral_monitor)
  hfx::IntegralHistory integrals;
  // the rows of the context's history monitor (hfx_ctx_set_history_monitor)
  hfx::HistoryRows history_rows;
  // the snapshots of the context's plot monitor (hfx_ctx_set_plot_monitor)
  hfx::PlotHistory plot;
  // exact-solution error norms (error_norm.hip): pos_volume_cubpts (n_vol_cubpts, n_eles, n_dims) of hfx_eles_set_error_points,
  // the cubature size it was registered for, and one partial per workgroup and quantity of the call that runs
  hfx::DevBuf<double> pos_volume_cubpts, err_partial;
  int n_err_cubpts = 0;
  // plot-point interpolation (hfx_eles_set_opp_p)
  int n_ppts = 0;
  hfx::Operator opp_p;
  hfx::DevBuf<double> disu_ppts;
  // time-averaged fields (hfx_eles_set_average_fields): disu_average_upts (n_upts, n_eles, n_average_fields)
  int n_average_fields = 0;
  int average_codes[HFX_MAX_AVERAGE_FIELDS] = {};
  hfx::DevBuf<double> disu_average_upts, disu_average_ppts;
  // point probes (hfx_eles_set_probes)
  hfx::Probes probes;
  // mass-flux body force (hfx_eles_set_body_force); null: none registered
  std::unique_ptr<hfx::BodyForce> body_force;
  // wall faces of the force monitor (hfx_eles_set_wall_faces); null: none registered
  std::unique_ptr<hfx::WallForces> wall_forces;
  // over-integration (hfx_eles_set_over_int)
  bool over_int_ready = false;
  int n_cubpts = 0;
  unsigned over_int_serial = 0; // counts hfx_eles_set_over_int calls (the 2-D simplex stage's tables are one registration's)
  hfx::Operator opp_over_int_cubpts, over_int_filter;
  hfx::DevBuf<double> JGinv_over_int_cubpts, u_cub, t_cub;
  // shock capturing (hfx_eles_set_shock_capture)
  bool shock_ready = false;
  hfx::Operator inv_vandermonde, exp_filter;
  hfx::DevBuf<double> persson_num, persson_den; // (n_upts) weights of the sensor's two sums
  // the same as registered, on the host (the 2-D simplex stage checks the sensor's form without a download), and the number of
  // the registration (0: none yet; tables made from an earlier one are rebuilt)
  std::vector<double> h_persson_num, h_persson_den;
  unsigned shock_serial = 0;
  double s0 = 0.0;
  int shock_det_field = 0;
  hfx::Operator opp_0, opp_1[3], opp_2[3], opp_3, opp_4[3], opp_5[3], opp_6;
  // metrics
  hfx::DevBuf<double> detjac_upts, JGinv_upts, detjac_fpts, JGinv_fpts, tdA_fpts, norm_fpts;
  // state / work arrays, indexed by hfx_array_id
  hfx::DevBuf<double> arr[HFX_N_ARRAYS];
  long arr_len[HFX_N_ARRAYS] = {};
  bool src_nonzero = false;
  // deferred execution: disu_fpts holds opp_0 . disu_upts(0) of the CURRENT state (the fused stages leave it so; anything
  // else that changes the state clears it), and on a partitioned block that flux-point solution is already on its way to
  // the neighbours; stale: bit i = array i was not refreshed by the last fused stage (its contents are older)
  bool fpts_valid = false, fpts_sent = false;
  unsigned long sent_on = 0; // fpts_sent: the serial number of the communicator that message travels on,
  int sent_blocks = 0;       // and the partition-face blocks of this element block it carries
  unsigned stale = 0;
  hfx::DevBuf<unsigned long long> nan_flag; // device: smallest flat index of a NaN in div_tconf, or ~0
  hfx::DevBuf<double> red_buf;            // device partial sums for reductions
  int red_blocks = 0;
  std::unique_ptr<hfx::TensorOps, hfx::TensorOpsDelete> tensor_ops; // 1-D factors of the over-integration / shock-capturing matrices
  // the form the last over-integration / shock capturing of this block ran (hfx_eles_tensor_ops_plan): 1 sum-factorised, 0 dense,
  // -1 none yet
  int over_int_form_run = -1, shock_form_run = -1;
  // fused-path private data (built lazily)
  std::unique_ptr<hfx::FusedData, hfx::FusedDelete> fused;
  std::unique_ptr<hfx::GeneralData, hfx::GeneralDelete> general; // the general (non-tensor-product) fused stage (general.hip)
  std::unique_ptr<hfx::Simplex2dData, hfx::Simplex2dDelete> simplex2d; // the 2-D simplex fused stage (simplex2d.hip)
  std::vector<hfx_inters *> faces_attached;
};

namespace hfx
{
// Slots of the persistent element kernels in hfx_fused_launch_grids: those of hfx_time_fused_kernels, and one each for the
// over-integration and the shock-capturing kernel
enum : int { SLOT_ELEMENT = 1, SLOT_UPDATE = 3, SLOT_OVER_INT = 4, SLOT_SHOCK = 5 };

// The grid of EVERY persistent element kernel: `most`, the workgroups its launcher would start for `work` elements (or list
// entries), and no more than the persistent_grid_cap option when that is set.  Notes the launch in the block's log.
inline int persistent_grid(const hfx_eles *e, int slot, long work, long most)
{
  const int cap = e->ctx->opt.persistent_grid_cap;
  const int grid = (int)(cap > 0 ? std::min<long>(most, cap) : most);
  hfx::LaunchLog &g = e->launch_log;
  // a stage launches its over-integration and flux (gradient) kernels, then its update (residual) kernels, then the shock filter: the
  // first of the former behind one of the latter begins the next stage (a partitioned stage is driven step by step, each its own call)
  const bool opens = slot == SLOT_OVER_INT || slot == SLOT_ELEMENT;
  if (opens && g.n > 0 && (g.slot[g.n - 1] == SLOT_UPDATE || g.slot[g.n - 1] == SLOT_SHOCK)) g.n = 0;
  if (g.n < hfx::LaunchLog::MAX)
  {
    g.slot[g.n] = slot; g.grid[g.n] = grid; g.work[g.n] = work;
    g.n++;
  }
  return grid;
}
} // namespace hfx

struct hfx_inters
{
  hfx_ctx *ctx = nullptr;
  hfx_eles *left = nullptr, *right = nullptr;
  int n_inters = 0, n_fpts_per_inter = 0;
  hfx::DevBuf<int> L, R;          // device (n_fpts_per_inter, n_inters)
  std::vector<int> hL, hR;        // host copies (for building per-element tables)
  // partition faces (is_mpi): R holds the received-record slot lut(j); buffers are owned here
  bool is_mpi = false;
  hfx::DevBuf<double> out_disu, in_disu, out_grad, in_grad;
  hfx::DevBuf<double> out_sgsf, in_sgsf; // LES: physical SGS flux records (allocated when the left block has a closure)
  // neighbour segments (hfx_mpi_inters_set_neighbours): faces [send[s], send[s]+count[s]) go to peer[s], its faces arrive at recv[s]
  std::vector<int> seg_peer, seg_send, seg_recv, seg_count;
  // boundary faces (is_bdy): left side only
  bool is_bdy = false;
  hfx::DevBuf<int> boundary_id; // device (n_inters)
  hfx::DevBuf<hfx_bc> bcs;      // device (n_bcs)
  int n_bcs = 0, ramp_counter = 0;
  bool any_ramp = false; // a group of this block ramps its total pressure: run_input.pressure_ramp (src/input.cpp:374-377)
  double R_ref = 0.0;
  // wall-model faces (a no-slip wall group with use_wm under a context with a wall model): their indices in the block, and
  // per face of the block the input point and its wall distance (hfx_bdy_inters_set_wall_model_points)
  int n_wm_faces = 0;
  bool wm_points = false;
  std::vector<int> h_wm_face;
  hfx::DevBuf<int> wm_face, wm_upt;
  hfx::DevBuf<double> wm_dist;
};

namespace hfx
{
// what every step loop and residual asks before its first launch: do the wall-model faces of a viscous run have their input points?
inline int wall_model_check_points(hfx_inters *const *faces, int nfb)
{
  for (int b = 0; b < nfb; b++)
  {
    const hfx_inters *f = faces[b];
    if (!f || !f->is_bdy || f->n_wm_faces == 0 || !f->ctx->params.viscous) continue;
    HFX_CHECK(f->wm_points, "face block %d has %d wall-model faces and no input points (hfx_bdy_inters_set_wall_model_points)", b,
              f->n_wm_faces);
  }
  return 0;
}
} // namespace hfx

// RCCL transport of the partition-face buffers (comm.hip)
struct hfx_comm
{
  hfx_ctx *ctx = nullptr;
  void *nccl = nullptr;         // ncclComm_t
  hipStream_t stream = nullptr; // communication stream
  int nranks = 1, rank = 0;
  hipEvent_t packed[3] = {nullptr, nullptr, nullptr};   // compute -> comm: buffers of kind 0 / 1 / 2 are packed
  hipEvent_t received[3] = {nullptr, nullptr, nullptr}; // comm -> compute: exchange of kind 0 / 1 / 2 complete
  hfx::DevBuf<double> scratch;                 // device scratch of the small all-reduces
  // exchange accounting (hfx_comm_exchange_stats): messages of kind 0 / 1 / 2 posted and waited for, one per partition-face
  // block -- what the per-method send_* / receive_* calls of those blocks would have posted -- and how many solution messages
  // of partition-face blocks are posted and not consumed yet
  long posted[3] = {0, 0, 0}, waited[3] = {0, 0, 0};
  int in_flight = 0;
  unsigned long serial = 0; // unique over the process (a block remembers the communicator of its message by it)
};

namespace hfx
{
// (wall_force.hip) the wall forces of a history row: _prepare is everything that refuses hfx_eles_compute_wall_forces on a block with wall
// faces and the arrays its launch needs; _launch the kernel alone, whose per-workgroup partials stay in wall_forces->partial
int wall_force_partials_prepare(hfx_eles *e, const char *who);
int wall_force_partials_launch(hfx_eles *e, int *n_groups);
// ---- deferred execution (deferred.hip) ----
int defer_record(hfx_ctx *ctx, int method, hfx_eles *e, hfx_inters *f, hfx_comm *c, int i0, int i1);
// run what has been recorded.  need: bit i = array i (hfx_array_id) must hold the reference's values afterwards -- a record
// that a fused stage would leave without them is replayed call by call
int defer_flush(hfx_ctx *ctx, unsigned need = 0);
struct DeferBusy
{
  hfx_ctx *c;
  bool prev;
  explicit DeferBusy(hfx_ctx *ctx) : c(ctx), prev(ctx->defer.busy) { c->defer.busy = true; }
  ~DeferBusy() { c->defer.busy = prev; }
};
// the state of e is about to change (or may be changed through a device pointer): disu_fpts no longer holds it.  A solution
// message of e still on its way is taken off first -- the compute stream waits for it -- so that nothing the caller writes
// next races the communication stream (comm.hip)
int invalidate_fpts(hfx_eles *e);
int side_stream_fork(hfx_ctx *ctx);
int side_stream_join(hfx_ctx *ctx);
int side_stream_wait(hfx_ctx *ctx);
// (hfx.hip) the squared length scale of the eddy-viscosity closures at every solution point, for the fused stages' flux kernels
int les_len2_upload(hfx_eles *e, DevBuf<double> &dst);
} // namespace hfx
// a per-method entry point: recorded while the context defers (and is not replaying)
#define HFX_DEFER(ctx_, method_, e_, f_, c_, i0_, i1_)  \
  if ((ctx_)->defer.on && !(ctx_)->defer.busy) return hfx::defer_record(ctx_, method_, e_, f_, c_, i0_, i1_)
// any other entry point that reads or changes device state: what has been recorded runs first
#define HFX_IMMEDIATE(ctx_, need_)                \
  if (hfx::defer_flush(ctx_, need_)) return 1;    \
  hfx::DeferBusy _defer_busy(ctx_)

// an entry point that reads array id_ of e_: refused when the fused stage that ran last left it with older contents
#define HFX_CHECK_CURRENT(e_, id_, who_)                                                                                        \
  HFX_CHECK(!((e_)->stale & (1u << (id_))),                                                                                    \
            "%s: array %d was not materialised by the fused stage that ran last (deferred execution): read it before the "      \
            "next stage begins", who_, id_)

namespace hfx
{
// The corrected gradients after a fused stage that ran OUTSIDE the deferred scheduler (which keeps the account of every array itself,
// deferred.hip).  A stage that keeps them on chip -- split variant 3, the general stage -- leaves an older stage's values in
// grad_disu_upts / grad_disu_fpts: they are marked, and hfx_eles_download and the error monitor refuse them until something writes
// them again.  Split variant 2 has just written them: the mark goes.  Every loop and stage entry point that runs such a stage calls this
inline void note_gradients(hfx_eles *e, bool materialised)
{
  if (!e->ctx->params.viscous) return;
  const unsigned grads = (1u << HFX_GRAD_DISU_UPTS) | (1u << HFX_GRAD_DISU_FPTS);
  e->stale = materialised ? (e->stale & ~grads) : (e->stale | grads);
}
} // namespace hfx

// boundary-face kernels (hfx.hip); visc 0: inviscid sweep (+ LDG common solution), 1: viscous sweep;
// fast: the fused paths' reciprocal-multiply physics
extern "C" int hfx_bdy_launch_internal(hfx_inters *f, int visc, int fast);
// LES: sgsf_upts = JGinv * F_sgs from disu_upts(0) and grad_disu_upts (hfx.hip)
extern "C" int hfx_mpi_sgsf_buffers_internal(hfx_inters *f); // allocates out / in_sgsf when the left block has a closure
extern "C" int hfx_les_sgsf_upts_internal(hfx_eles *e);
extern "C" int hfx_les_extrapolate_reference_internal(hfx_eles *e); // sgsf_fpts = opp_0 * sgsf_upts, not yet back-transformed
// the bytes of device memory the library holds now (all contexts of the process): what a create / destroy cycle must give back
extern "C" long hfx_live_device_bytes_internal(void);
