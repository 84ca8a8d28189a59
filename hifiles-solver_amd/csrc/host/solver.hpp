// solver.hpp -- `struct solution`, the stage scheduler CalcResidual and the box-mesh setup.
//
// struct solution mirrors /root/reference/include/solution.h:44-96; CalcResidual has the
// call order of /root/reference/src/solver.cpp:50-223 (RANS off)
// and calls only the public eles / int_inters methods, like the reference's.
#pragma once
#include <string>
#include <vector>

#include "eles.hpp"
#include "inters.hpp"

struct solution
{
  int rank = 0, nproc = 1;
  double time = 0.0;
  int i_steps = 0; // time steps of this run (src/HiFiLES.cpp:99,223): step 1 sets run_input.spinup_time; a restart read resets it
  int n_ele_types = 5; // 0 tri, 1 quad, 2 tet, 3 pri, 4 hex (src/geometry.cpp:135)
  int n_dims = 0;
  int num_cells_global = 0, ini_iter = 0;
  hf_array<eles *> mesh_eles; // entries of classes this build does not carry are NULL
  eles_quads mesh_eles_quads;
  eles_hexas mesh_eles_hexas;
  int n_int_inter_types = 3;
  hf_array<int_inters> mesh_int_inters;
  int n_bdy_inter_types = 3;
  hf_array<bdy_inters> mesh_bdy_inters; // include/solution.h:84-86
  // partition faces (include/solution.h:88-94, _MPI only in the reference)
  int n_mpi_inter_types = 3;
  hf_array<mpi_inters> mesh_mpi_inters;
  int n_mpi_inters = 0;
  input run_input;
  hfx_ctx *ctx = nullptr;
  hfxh_exchange_fn exchange = nullptr;
  void *exchange_user = nullptr;
  double (*reduce_min)(void *user, double v) = nullptr; // MPI_Allreduce(MIN) of calc_time_step, supplied by the caller
  void *reduce_user = nullptr;
  void (*reduce_sum)(void *user, double *v, int n) = nullptr; // MPI_Allreduce(SUM) of the body force's integrals, supplied by the caller
  void *reduce_sum_user = nullptr;
  hfx_comm *comm = nullptr; // the library's RCCL transport (SetComm); takes the place of `exchange` and `reduce_min`
  // deferred execution (include/hfx.h): the method calls of CalcResidual + AdvanceSolution below are recorded by libhfx and
  // a whole stage runs as one fused stage -- the call sequence itself is the reference's, unchanged.  On by default.
  bool deferred = true;
  int history_freq = 0; // the monitor_res_freq the context's history monitor is registered with; 0: none (RegisterHistoryMonitor)
  std::string err;
  ~solution();
};

// periodic box [0,length]^dims of n[0] x n[1] (x n[2]) quads / hexes, optional smooth periodic
// deformation (same formula as oracle/gen_neu_mesh.py) or caller-supplied vertices
// xv[v + nv*d], v = ix + (nx+1)*(iy + (ny+1)*iz).
struct box_mesh
{
  int dims = 3, n[3] = {1, 1, 1}; // cells of THIS rank's block
  double length = 0.0, amp = 0.0; // edge of the GLOBAL periodic box
  // block decomposition of the structured box: pgrid ranks per direction, this rank's coordinates.
  // The reference partitions with ParMETIS (src/mesh.cpp:72-314), which is not available; the
  // structured block split is the documented stand-in.
  int pgrid[3] = {1, 1, 1}, pcoord[3] = {0, 0, 0};
  int rank_of(int px, int py, int pz) const { return px + pgrid[0] * (py + pgrid[1] * pz); }
  // a periodic direction that is NOT split (pgrid 1) whose wrap-around faces are nevertheless made partition faces, with
  // this rank as its own neighbour: the whole partition-face path (pack, exchange, one-sided kernels) then runs on one
  // rank -- how the RCCL transport is exercised on a one-GPU box
  int self_partition[3] = {0, 0, 0};
  // boundary group of each side of the GLOBAL box, indexed by the element-local face number (hex: z- y- x+ y+ x-
  // z+, quad: y- x+ y+ x-): index into run_input.bc_specs; -1 or a cyclic group = periodic.  A direction is
  // periodic when both of its sides are.
  int side_bc[6] = {-1, -1, -1, -1, -1, -1};
  std::vector<double> xv; // (nv, dims) column-major
  int nv() const { return (n[0] + 1) * (n[1] + 1) * (dims == 3 ? n[2] + 1 : 1); }
  int ne() const { return n[0] * n[1] * (dims == 3 ? n[2] : 1); }
  void generate();
};

// the part of GeoPreprocess + InitSolution the hot path needs (src/geometry.cpp:106-915,
// src/solver.cpp:321): elements, shapes, transforms, interior (periodic) faces, initial state
int GeoPreprocess_box(solution *FlowSol, const box_mesh &mesh);
int InitSolution(solution *FlowSol);
// move everything to the device (the reference's mv_all_cpu_gpu calls, src/geometry.cpp:310-320,552-557)
int MoveToDevice(solution *FlowSol, int device);
// point probes: run_input's probe fields -> the context (hfx_ctx_set_probes); one sample of every element class at the solution's
// time and step (always, or under the reference's condition i_steps % probe_freq == 0)
int RegisterProbeFields(solution *S);
void SampleProbes(solution *FlowSol, bool always);
// run_input's test case -> the context (hfx_ctx_set_exact_solution), with the walls of Couette flow from the boundary groups
int RegisterExactSolution(solution *S);
// output::compute_error (src/output.cpp:2052-2110) without the file: error (2, n_fields) summed over the element classes and the
// ranks (one SUM reduction of 2 n_fields values), then the square root for error_norm_type 2, at the solution's time
int ComputeError(solution *FlowSol, double *error);
// output::CalcIntegralQuantities (src/output.cpp:2017-2038): run_input's integral quantities over the classes and the ranks
int CalcIntegralQuantities(solution *FlowSol, double *integral_quantities);
// the integral monitor (hfx_ctx_set_integral_monitor): run_input's quantities, monitor_res_freq and history size -> the context;
// one sample of every class at the solution's clock (always, or under the reference's condition i_steps == 1 || i_steps %
// monitor_res_freq == 0, src/HiFiLES.cpp:247); the stored samples; the rows of history.plt over classes and ranks
int RegisterIntegralMonitor(solution *FlowSol);
int SampleIntegralQuantities(solution *FlowSol, bool always);
int IntegralCount(solution *FlowSol, int *n_samples);
int ReadIntegralHistory(solution *FlowSol, int max_samples, double *times, int *steps, double *values, int *n_samples);
// the history monitor (hfx_ctx_set_history_monitor): run_input's res_norm_type, calc_force, monitor_res_freq and history size -> the
// context; one row of every class at the solution's clock (always, or under the reference's condition); the stored rows
int RegisterHistoryMonitor(solution *FlowSol);
int SampleHistory(solution *FlowSol, bool always);
int HistoryCount(solution *FlowSol, int *n_rows);
// the plot monitor (hfx_ctx_set_plot_monitor): run_input's diagnostic_fields, plot_freq and history size -> the context; one snapshot
// of every class at the solution's clock (always, or under the reference's condition i_steps % plot_freq == 0, src/HiFiLES.cpp:273);
// the stored snapshots; the columns of a row (n_dims + n_fields + n_average_fields + n_diagnostic_fields) and the rows of a snapshot
// (the plot points of every class); the rows as write_tec prints them (src/output.cpp:366-427), the histories emptied: per snapshot,
// classes in their order, per element and plot point the position, the conserved fields, the averages, the diagnostic fields.  A NaN
// is the reference's error ("Nan in tecplot file, exiting", src/output.cpp:397; "NaN", src/eles.cpp:3999)
int RegisterPlotMonitor(solution *FlowSol);
int SamplePlot(solution *FlowSol, bool always);
int PlotCount(solution *FlowSol, int *n_snapshots);
int PlotColumns(const solution *FlowSol);
long PlotPoints(const solution *FlowSol);
int ReadPlotRows(solution *FlowSol, int max_snapshots, double *times, int *steps, double *rows, int *n_snapshots);
// the finish of output::CalcNormResidual (src/output.cpp:2236-2246) on what the classes and ranks gave: sum[n_fields] -- the max for
// norm type 0, the sums for 1 and 2 -- and n_upts -> sum, sum / n_upts or sqrt(sum) / n_upts; a NaN norm is the reference's error
int NormResidual(int res_norm_type, int n_fields, const double *sum, long n_upts, double *norm_residual, std::string &err);
// output::CalcNormResidual (src/output.cpp:2166-2248) now, through eles::compute_res_upts of every class: norm_residual[n_fields]
int CalcNormResidual(solution *FlowSol, double *norm_residual);
// the rows as HistoryOutput writes them (src/output.cpp:2375-2402) without the computing time, the histories (the integral monitor's
// too) emptied: per row log10(norm_residual) per field, with calc_force inv + vis force per dimension, CL, CD, the integral
// quantities where that monitor is registered, the time (x time_ref on a viscous case)
int HistoryColumns(const solution *FlowSol);
int ReadHistory(solution *FlowSol, int max_rows, int *steps, double *rows, int *n_cols, int *n_rows);
// run_input's reference state -> the context (hfx_ctx_set_force_reference): rho_c_ic, u_c_ic, v_c_ic, w_c_ic, p_c_ic, area_ref
int RegisterForceReference(solution *S);
// output::CalcForces (src/output.cpp:1915-2014) without the file: eles::compute_wall_forces of every element class, summed, then
// summed over the ranks (one SUM reduction of 2 n_dims + 2 values; every rank gets the sums, where the reference's MPI_Reduce
// gives them to rank 0)
int CalcForces(solution *FlowSol, double *inv_force, double *vis_force, double *cl, double *cd);
// switch deferred execution on / off (before or after MoveToDevice)
int SetDeferred(solution *FlowSol, bool on);

void CalcResidual(int in_file_num, int in_rk_stage, solution *FlowSol);
// RK loop of src/HiFiLES.cpp:194-221 through the mirrored class methods
int calc_time_step(solution *FlowSol); // src/solver.cpp:484-549
// ASCII restart files "Rest_%09d_p%04d.dat" (host arrays; sync with the device before / after)
int write_restart_ascii(solution *FlowSol, const std::string &dir, int in_file_num);             // src/output.cpp:1753
int read_restart_ascii(solution *FlowSol, const std::string &dir, int in_file_num, int n_files); // src/solver.cpp:377
int RunSteps(solution *FlowSol, int n_steps);
// the same RK loop through the split fused kernels on a partitioned block, exchanging between the
// phases of hfx_stage_partitioned
int RunStepsPartitionedFused(solution *FlowSol, int n_steps);
void SetExchange(solution *FlowSol, hfxh_exchange_fn fn, void *user);
void SetReduceMin(solution *FlowSol, double (*fn)(void *user, double v), void *user);
void SetReduceSum(solution *FlowSol, void (*fn)(void *user, double *v, int n), void *user);
// collective: the library's communicator for this rank (id from hfx_comm_get_unique_id on rank 0)
int SetComm(solution *FlowSol, const char *unique_id);
// per-phase / per-exchange times of the partitioned fused stage (hfx_time_partitioned)
int TimePartitioned(solution *FlowSol, int reps, double ms[8]);
// what RCCL reports for the communicator (hfx_comm_info)
int CommInfo(solution *FlowSol, int *nranks, int *rank, int *device, char pci_bus_id[32]);
