// input.hpp -- the frozen subset of the reference's run_input that the hot path and its
// setup read (/root/reference/include/input.h; keys of src/input.cpp:62-327), plus the
// non-dimensionalisation of input::setup_params (src/input.cpp:527-720).
// Not a global: each `solution` owns one.
#pragma once
#include <string>
#include <vector>

#include "../../../include/hfx.h"
#include "hf_array.hpp"

// one boundary group as the input file gives it: `bc_<name>_type` and the type's parameters, DIMENSIONAL
// (/root/reference/src/input.cpp:328-437)
struct bc_spec
{
  int flag = HFX_BC_CYCLIC; // src/bc.cpp:36-48
  double rho = 0, u = 0, v = 0, w = 0, p_static = 0, T_static = 0, p_total = 0, T_total = 0;
  double nx = 1., ny = 0., nz = 0., mach = 0;
  int pressure_ramp = 0;
  double p_ramp_coeff = 0, T_ramp_coeff = 0, p_total_old = 0, T_total_old = 0;
  bool T_total_given = false, T_total_old_given = false;
  int use_wm = 0; // bc_<name>_use_wm: read for isotherm_wall / adiabat_wall groups, and only when wall_model != 0 (src/input.cpp:413,433)
};

struct input
{
  // ---- solver
  int equation = 0, viscous = 1, order = 4;
  int riemann_solve_type = 3, vis_riemann_solve_type = 0;
  int ic_form = 7, adv_type = 3, dt_type = 0, n_steps = 1;
  double dt = 0.0, CFL = 0.0;
  double ldg_tau = 0.0, ldg_beta = 0.5;
  // ---- polynomial de-aliasing and shock capturing (src/input.cpp:248-263)
  int over_int = 0, over_int_order = 0;
  int shock_cap = 0, shock_det = 0, shock_det_field = 0;
  double s0 = 0.0, expf_fac = 36.0;
  int expf_order = 4, expf_cutoff = 0;
  // ---- LES closure (src/input.cpp:167-182,666): SGS_model 0 Smagorinsky (needs the wall distance: meshes without walls
  // only here), 1 WALE, 2 WALE + similarity, 3 spectral vanishing viscosity, 4 similarity; the last three filter the
  // solution with filter_upts built from filter_type / filter_ratio
  int LES = 0, SGS_model = 1, filter_type = 0;
  double C_s = 0.0, filter_ratio = 1.0, Kappa = 0.41, prandtl_t = 0.9;
  // ---- wall model (src/input.cpp:176): 0 none, 1 Werner-Wengle, 2 Breuer-Rodi; reads prandtl_t and Kappa above
  int wall_model = 0;
  // ---- plotting: points per edge (src/input.cpp:110; the reference's default is 2)
  int p_res = 2;
  // ---- time-averaged fields (src/input.cpp:115-133): names of rho_average, u_average, v_average, w_average, e_average, lower-cased;
  // spinup_time: the time of the first step of the run, where the averages begin (src/HiFiLES.cpp:242-243)
  std::vector<std::string> average_fields;
  int n_average_fields = 0;
  double spinup_time = 0.0;
  // the names -> average_fields (lower-cased as src/input.cpp:130-133 does) and n_average_fields.  A name outside the five is refused
  // (the reference's CalcTimeAverageQuantities would average an uninitialised value, src/eles.cpp:5632-5674), and so is
  // w_average when n_dims is 2; a refusal leaves the fields as they were
  int set_average_fields(const std::vector<std::string> &names, int n_dims, std::string &err);
  // HFX_AVG_* of average_fields(i)
  int average_code(int i) const;
  // ---- point probes (run_input.probe, src/probe_input.cpp): the field names of rho, u, v, w, specific_total_energy, pressure,
  // lower-cased as probe_input::read_probe_input does; probe_freq in steps; probe_capacity: the samples the device history holds
  // (a key of this mirror: the reference writes every sample to a file at once)
  std::vector<std::string> probe_fields;
  int n_probe_fields = 0, probe_freq = 1, probe_capacity = 0;
  // a name outside the six, w in a two-dimensional run, probe_freq < 1 and capacity < 1 are refused and leave everything as it was
  int set_probe_fields(const std::vector<std::string> &names, int n_dims, int freq, int capacity, std::string &err);
  int probe_code(int i) const; // HFX_PROBE_* of probe_fields(i)
  // ---- exact-solution error norms (src/input.cpp:108-109): test_case 0 none, 1 isentropic vortex, 5 Couette flow (2, 3, 4 belong to
  // the advection-diffusion equation); error_norm_type 1 L1, 2 L2.  Refusals leave both as they were
  int test_case = 0, error_norm_type = 2;
  int set_test_case(int in_test_case, int in_error_norm_type, std::string &err);
  // test case 5: velocity(0) of the moving isothermal wall and T_static of the one at rest, from bc_list by the reference's rule
  // (src/eles.cpp:5219-5230).  The reference reads what it did not find uninitialised; here a missing wall is refused by name
  int couette_walls(double &u_wall, double &T_wall, std::string &err) const;
  // ---- integral diagnostics (src/input.cpp:134-149): names out of kineticenergy, enstropy, pressuredilatation, straincolonproduct,
  // devstraincolonproduct (the reference's spelling), lower-cased; another name is refused with the reference's words
  std::vector<std::string> integral_quantities;
  int n_integral_quantities = 0;
  int set_integral_quantities(const std::vector<std::string> &names, std::string &err);
  int integral_quantity_code(int i) const; // the quantity id of hfx_eles_CalcIntegralQuantities
  // the frequency in steps of the history rows, default 100, 0 means 1000 (src/input.cpp:101,534-535).  integral_capacity: the samples
  // the device history of the integral monitor holds; 0: the quantities are not sampled in the loops (the caller asks for them with
  // CalcIntegralQuantities, as before).  A negative frequency or capacity is refused and leaves both as they were
  int monitor_res_freq = 100, integral_capacity = 0;
  int set_monitor_res_freq(int freq, int capacity, std::string &err);
  bool integral_monitor_on() const { return n_integral_quantities > 0 && integral_capacity > 0; }
  bool integral_sample_step(int i_steps) const { return i_steps == 1 || i_steps % monitor_res_freq == 0; } /* src/HiFiLES.cpp:247 */
  // ---- the residual and force columns of a history row: res_norm_type 0 infinity, 1 L1, 2 L2 norm (default 2, src/input.cpp:108);
  // anything else is refused with the reference's words (src/output.cpp:2241).  history_capacity: the rows the device history of the
  // history monitor holds; 0: no rows are taken in the loops.  The forces of a row follow calc_force
  int res_norm_type = 2, history_capacity = 0;
  int set_history(int norm_type, int capacity, std::string &err);
  bool history_monitor_on() const { return history_capacity > 0; }
  // ---- the plot file (src/input.cpp:98,114,125-129): run_input.diagnostic_fields out of u, v, w, energy, mach, pressure, vorticity,
  // q_criterion, scaled_q_criterion, sensor, lower-cased; another name is refused with the reference's words (src/eles.cpp:3994).
  // plot_freq in steps (the reference's default is INT32_MAX: never); plot_capacity: the snapshots the device history of the plot
  // monitor holds; 0: no snapshots are taken in the loops.  Refusals leave everything as it was
  std::vector<std::string> diagnostic_fields;
  int n_diagnostic_fields = 0;
  int set_diagnostic_fields(const std::vector<std::string> &names, std::string &err);
  int diagnostic_code(int i) const; // HFX_PLOT_* of diagnostic_fields(i)
  int plot_freq = 2147483647, plot_capacity = 0;
  int set_plot(int freq, int capacity, std::string &err);
  bool plot_monitor_on() const { return plot_capacity > 0; }
  bool plot_sample_step(int i_steps) const { return i_steps % plot_freq == 0; } /* src/HiFiLES.cpp:273 */
  // ---- mass-flux body force of periodic channels (`body_forcing`, src/input.cpp:312).  forcing_area and forcing_mdot0 are keys of
  // this mirror: the inflow area and the target mass flux, which the reference hard-codes to 9.162 both (src/eles.cpp:5393-5395);
  // forcing_history: evaluations whose massflux.dat columns the device keeps
  int forcing = 0;
  double forcing_area = 9.162, forcing_mdot0 = 9.162;
  int forcing_history = 4096;
  // ---- wall forces (src/input.cpp:102-107): calc_force 1 makes output::CalcForces available; area_ref DIMENSIONAL on input (a
  // viscous run divides it by L_ref^2, src/input.cpp:621-622); monitor_cp_freq 0 means never (src/input.cpp:536-537)
  int calc_force = 0, monitor_cp_freq = 2147483647;
  double area_ref = 0.0;
  // ---- element parameters
  int upts_type_hexa = 0, vcjh_scheme_hexa = 1;
  double eta_hexa = 0.0;
  // tetrahedra and prisms (src/input.cpp:264-300)
  int upts_type_tet = 0, fpts_type_tet = 0, vcjh_scheme_tet = 1;
  int upts_type_pri_tri = 0, upts_type_pri_1d = 0, vcjh_scheme_pri_1d = 1, vcjh_scheme_tri = 1;
  double eta_pri = 0.0;
  double c_tet = 0.0, c_tri = 0.0; // vcjh_scheme_tet / _tri 0: the filter's c given (src/input.cpp:289,299)
  int upts_type_quad = 0, vcjh_scheme_quad = 1;
  double eta_quad = 0.0;
  // ---- gas
  double gamma = 1.4, prandtl = 0.72, S_gas = 120.0, T_gas = 291.15, R_gas = 286.9, mu_gas = 1.827e-5;
  int fix_vis = 1;
  double Mach_free_stream = 1.0, L_free_stream = 1.0, T_free_stream = 300.0, rho_free_stream = 1.17723946;
  // ---- initial condition (dimensional on input, like the reference)
  double Mach_c_ic = 0.0, nx_c_ic = 1.0, ny_c_ic = 0.0, nz_c_ic = 0.0, T_c_ic = 0.0, rho_c_ic = 0.0;
  double u_c_ic = 0.0, v_c_ic = 0.0, w_c_ic = 0.0, p_c_ic = 0.0; // inviscid inputs
  // optional override of the 1-D solution points (order+1 values); empty: computed
  hf_array<double> loc_1d_upts_override;
  // ---- periodic box
  double dx_cyclic = 0.0, dy_cyclic = 0.0, dz_cyclic = 0.0;

  // ---- derived by setup_params()
  double T_ref = 0, L_ref = 0, rho_ref = 0, uvw_ref = 0, p_ref = 0, mu_ref = 0, time_ref = 0, R_ref = 0;
  double c_sth = 0, mu_inf = 0, rt_inf = 0, uvw_c_ic = 0, mu_c_ic = 0;
  hf_array<double> RK_a, RK_b, RK_c;
  double time = 0.0;

  // ---- boundary groups: bc_specs in, bc_list (non-dimensional records for the device) out
  std::vector<bc_spec> bc_specs;
  std::vector<hfx_bc> bc_list;
  int ramp_counter = 0;
  int pressure_ramp = 0; // 1 when a group ramps its total pressure (src/input.cpp:374-377)
  // input::read_boundary_param (src/input.cpp:328-525) after setup_params()
  int read_boundary_param(std::string &err);
  double bc_R_ref() const { return viscous ? R_ref : R_gas; } // src/bdy_inters.cpp:368-369

  // returns 0 or sets err (the reference's FatalError texts)
  int setup_params(std::string &err);
  int n_rk_stages() const { return adv_type == 0 ? 1 : (adv_type <= 2 ? 4 : (adv_type == 3 ? 5 : 14)); }
  void fill(hfx_params &p) const;
};
