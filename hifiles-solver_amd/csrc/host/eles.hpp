// eles.hpp -- host-side mirror of the reference's element classes for the hot path.
//
// Same public method names, argument meaning and array layouts as
// /root/reference/include/eles.h:55-125 (eles), eles_hexas.h, eles_quads.h, so that a
// CalcResidual written against the reference's interface (src/solver.cpp:50-223) drives
// this implementation unchanged.  The per-stage methods do no arithmetic on the host:
// they call the C ABI of libhfx (include/hfx.h), which owns the device copy of every array.
// The setup methods (operators, metrics, initial condition) are host code, as in the reference.
#pragma once
#include <iostream>
#include <string>
#include <vector>

#include "../../../include/hfx.h"
#include "hf_array.hpp"
#include "input.hpp"

class eles
{
public:
  eles();
  virtual ~eles();

  // ---- setup (reference: eles::setup src/eles.cpp:66-235) -------------------------
  // returns 0 or non-zero with last_error() set (the reference calls FatalError)
  int setup(int in_n_eles, int in_max_n_spts_per_ele, input *in_run_input);
  void set_shape_node(int in_spt, int in_ele, const hf_array<double> &in_pos); // src/eles.cpp set_shape_node
  int set_transforms();                                                          // src/eles.cpp:4015
  int set_ics(double &time);                                                     // src/eles.cpp:237

  // ---- device residency (replaces mv_all_cpu_gpu / cp_*_gpu_cpu, src/eles.cpp:930-1062)
  int mv_all_cpu_gpu(hfx_ctx *ctx);
  void free_device();
  int cp_disu_upts_gpu_cpu();
  int cp_disu_upts_cpu_gpu();
  int cp_div_tconf_upts_gpu_cpu();
  int cp_grad_disu_upts_gpu_cpu();
  int cp_array_gpu_cpu(int hfx_id, hf_array<double> &dst);

  // ---- the per-stage methods CalcResidual calls (src/solver.cpp:65-216) -------------
  void extrapolate_solution();
  void calculate_gradient();
  void evaluate_invFlux();
  void evaluate_invFlux_over_int(); // src/eles.cpp:1480 (run_input.over_int)
  void shock_capture();             // src/eles.cpp:2918 (run_input.shock_cap), after AdvanceSolution
  void correct_gradient();
  void evaluate_viscFlux();
  void extrapolate_sgsFlux(); // src/eles.cpp:2817 (run_input.LES)
  void calc_sgs_terms();      // src/eles.cpp:2058 (SGS_model 2, 3, 4: at the first RK stage of a step)
  void extrapolate_totalFlux();
  void calculate_divergence();
  void calculate_corrected_divergence();
  void AdvanceSolution(int in_step, int adv_type);
  double calc_dt_local(int in_ele); // host evaluation on the host copy of disu_upts(0), src/eles.cpp:1267
  // ---- time-averaged fields (run_input->average_fields; registered by mv_all_cpu_gpu)
  void CalcTimeAverageQuantities(double &time); // src/eles.cpp:5630: one update on the device, spin-up time from run_input
  int register_average_fields();                // run_input->average_fields -> the device block (zeroed averages)
  int cp_disu_average_upts_gpu_cpu();           // -> disu_average_upts (n_upts, n_eles, n_average_fields)
  int calc_time_average_ppts_all();             // every element at once, on the device -> disu_average_ppts
  void calc_time_average_ppts(int in_ele, hf_array<double> &out_disu_average_ppts); // src/eles.cpp:3820, the per-element accessor
  hf_array<double> disu_average_upts, disu_average_ppts;
  double compute_res_upts(int in_norm_type, int in_field);
  // ---- surface cubature and the mass-flux body force (run_input->forcing; csrc/host/eles_forcing.cpp).  Built by set_transforms
  // only when forcing or calc_force is on, like the reference (src/eles.cpp:4023); for EVERY element, where the reference keeps them for its
  // boundary elements only (bdy_ele2ele): the second index of the per-element arrays is the element
  hf_array<int> n_cubpts_per_inter;
  hf_array<hf_array<double>> loc_inters_cubpts, weight_inters_cubpts, tnorm_inters_cubpts; // (n_dims, n_cubpts) | (n_cubpts) | (n_dims, n_cubpts)
  hf_array<hf_array<double>> opp_inters_cubpts;                                            // (n_cubpts, n_upts)
  hf_array<hf_array<double>> inter_detjac_inters_cubpts, norm_inters_cubpts;               // (n_cubpts, n_eles) | (n_cubpts, n_eles, n_dims)
  virtual int set_inters_cubpts();                // the class's face cubature rule (src/eles_hexas.cpp:284-373, src/eles_quads.cpp:251-315); quadrilaterals and hexahedra here
  void set_opp_inters_cubpts();                   // src/eles.cpp:3635-3665
  void set_transforms_inters_cubpts();            // src/eles.cpp:4480-4595
  virtual double compute_inter_detjac_inters_cubpts(int in_inter, const hf_array<double> &d_pos) { return 0.0; }
  // cyclic_inter(ele, l) = 1: local face l of the element lies on a cyclic boundary group of the mesh (set by the mesh setup: the
  // reference asks run_input.bc_list(bcid(ele, l)), src/eles.cpp:5322)
  hf_array<int> cyclic_inter;
  // the reference's inflow rule (src/eles.cpp:5312-5338): cyclic, and the x-component of the unit normal at the first cubature
  // point == -1 exactly -> inflow_ele / inflow_inter, elements ascending, local faces ascending
  void set_inflow_inters();
  std::vector<int> inflow_ele, inflow_inter;
  int register_body_force();                 // -> hfx_eles_set_body_force with run_input's forcing_area / forcing_mdot0 (resets the controller)
  void evaluate_body_force(int in_file_num); // src/eles.cpp:5281: one evaluation on the device
  // its two halves around the sum over the ranks (src/eles.cpp:5375-5385), for the transports of solution::comm / reduce_sum
  int body_force_integrals(double integral[2]);
  int body_force_apply(const double integral[2]);

  // ---- wall forces (run_input->calc_force; csrc/host/eles_forces.cpp; output::CalcForces, src/output.cpp:1915-2014).  The surface
  // cubature above is then built for quadrilaterals and hexahedra (src/eles.cpp:4023).
  // bcid(ele, l): the boundary group of local face l of the element, -1 none (set by the mesh setup; src/geometry.cpp:292)
  hf_array<int> bcid;
  // the wall faces in the reference's order (src/eles.cpp:5746-5769): elements with a boundary face ascending, local faces
  // ascending -- those whose bcid names a slip, isothermal, adiabatic or dual-consistent slip wall, and ONLY those (the
  // reference also reads bc_list(-1)); per face the bc flag and the number of cubature points; wall_pos (n_dims, points): calc_pos
  // of every point, faces as walked, inside a face j DESCENDING, the row order of cp_*.dat
  void set_wall_inters();
  std::vector<int> wall_ele, wall_inter, wall_flag, wall_n_points;
  std::vector<double> wall_pos;
  int register_wall_forces(); // -> hfx_eles_set_wall_faces
  // src/eles.cpp:5704 on the device: this class's sums; Cp and Cf of every point -> wall_cp, wall_cf in the order of wall_pos
  int compute_wall_forces(hf_array<double> &inv_force, hf_array<double> &vis_force, double &temp_cl, double &temp_cd);
  std::vector<double> wall_cp, wall_cf;

  // ---- point probes (csrc/host/eles_probes.cpp; run_input.probe, src/probe_input.cpp, src/output.cpp:1440-1545)
  int calc_p2c(const hf_array<double> &in_pos); // the class's calc_p2c: the element that holds in_pos, -1 none, -2 shape not implemented (probe_error)
  int pos_to_loc(const hf_array<double> &in_pos, int in_ele, hf_array<double> &out_loc); // src/eles.cpp:5992; non-zero: no convergence
  void set_opp_probe(const hf_array<double> &in_loc);                                    // src/eles.cpp:3625 -> opp_probe (n_upts)
  void calc_pos_probe(const hf_array<double> &in_loc, int in_ele, hf_array<double> &out_pos); // calc_pos, for callers outside the class
  hf_array<double> opp_probe;
  // the located probes of this class: element (run_probe.p2c), index in the caller's list, reference location (n_dims each),
  // operator rows (n_upts each)
  std::vector<int> probe_p2c, probe_global;
  std::vector<double> probe_loc, probe_opp;
  int locate_probes(int n, const double *positions); // locate positions (n_dims, n), keep what lies in this class (host only)
  std::string probe_error;                           // why calc_p2c / pos_to_loc / locate_probes refused (the block itself stays usable)
  int register_probes();                          // -> hfx_eles_set_probes (empties the device history)
  void sample_probes(double time, int step);      // one sample on the device
  // the shape nodes that span the plane of local face in_face (calc_p2c); returns the number of faces, -1: shape not implemented
  virtual int face_plane_vertices(int in_n_spts, int in_face, int v[3]) const = 0;

  // ---- volume cubature and the monitors over it (csrc/host/eles_error.cpp): run_input->test_case, n_integral_quantities.
  // loc (n_dims, n_cubpts), weight (n_cubpts), opp (n_cubpts, n_upts), vol_detjac (n_cubpts, n_eles), pos (n_cubpts, n_eles, n_dims;
  // a test case only).  Quadrilaterals and hexahedra; empty while neither monitor is asked for
  hf_array<double> loc_volume_cubpts, weight_volume_cubpts, opp_volume_cubpts, vol_detjac_vol_cubpts, pos_volume_cubpts;
  int set_volume_cubature();      // builds or drops the five arrays by run_input (host only)
  int register_volume_cubature(); // -> hfx_eles_set_volume_cubpts, hfx_eles_set_error_points
  int compute_error(int in_norm_type, double &time, hf_array<double> &error); // src/eles.cpp:5076 on the device: error (2, n_fields)
  int CalcIntegralQuantities(int n_integral_quantities, hf_array<double> &integral_quantities); // src/eles.cpp:5485: adds to them

  // ---- getters used by face wiring (src/eles.cpp:4638-4949 return pointers; here: offsets)
  int get_n_eles() const { return n_eles; }
  int get_n_dims() const { return n_dims; }
  int get_n_fields() const { return n_fields; }
  int get_n_fpts_per_inter(int f) const { return n_fpts_per_inter(f); }
  // offset `fpt + n_fpts*ele` of local flux point `in_fpt` of local face `in_inter` of element `in_ele`
  int get_fpt_offset(int in_ele, int in_inter, int in_fpt) const;
  // eles::calc_wm_upts_dist (src/eles.cpp:4873-4903): the wall model's input point of local face in_local_inter -- the FIRST solution
  // point with the strictly largest minimum, over the face's flux points, of (pos_fpt - pos_upt) . n_fpt -- and that distance.  On a
  // mesh where several points tie (a Cartesian one: the whole far row) the pick is the first strictly larger in this arithmetic
  double calc_wm_upts_dist(int in_ele, int in_local_inter, int &out_upt) const;
  hfx_eles *device() { return dev; }
  const std::string &last_error() const { return err; }
  bool failed() const { return !err.empty(); }

  // ---- data (public here; protected in the reference: include/eles.h:470-935) --------
  input *run_input = nullptr;
  int n_eles = 0, n_dims = 0, n_fields = 0, order = 0, ele_type = -1, viscous = 0;
  int n_upts_per_ele = 0, n_fpts_per_ele = 0, n_inters_per_ele = 0, upts_type = 0;
  hf_array<int> n_fpts_per_inter, n_spts_per_ele;
  hf_array<double> loc_1d_upts, loc_upts, tloc_fpts, tnorm_fpts;
  hf_array<double> shape; // (n_dims, max_n_spts, n_eles)
  hf_array<double> opp_0, opp_3, opp_6;
  hf_array<hf_array<double>> opp_1, opp_2, opp_4, opp_5;
  hf_array<double> detjac_upts, JGinv_upts, detjac_fpts, JGinv_fpts, tdA_fpts, norm_fpts, pos_upts, pos_fpts;
  hf_array<hf_array<double>> disu_upts;      // host copies, valid after cp_*_gpu_cpu
  hf_array<hf_array<double>> div_tconf_upts;
  hf_array<double> grad_disu_upts;
  hf_array<double> h_ref, dt_local;
  hf_array<double> Jacobian_fpts; // (n_dims,n_dims,n_fpts,n_eles) d(pos)/d(loc) at the flux points, LES only (src/eles.cpp:4231)
  // eles::calc_wall_distance (src/eles.cpp:2701-2810): for every solution point the vector from the nearest flux point of a no-slip
  // wall face (brute force; loc_noslip_bdy: (n_dims, n_points) column-major, faces in the mesh's order); the damped Smagorinsky closure
  // uses its length
  void calc_wall_distance(const std::vector<double> &loc_noslip_bdy);
  hf_array<double> wall_distance; // (n_upts,n_eles,n_dims)
  // ---- modal operators of the tensor-product classes (eles_modal.cpp): shock capturing and over-integration
  // (include/eles.h:926-935; eles_hexas.h / eles_quads.h: vandermonde, inv_vandermonde, norm_basis_persson)
  hf_array<double> vandermonde, inv_vandermonde, exp_filter, norm_basis_persson;
  hf_array<int> persson_high_modes; // 1: a mode with a degree == order in some direction
  hf_array<double> loc_over_int_cubpts, weight_over_int_cubpts, opp_over_int_cubpts, over_int_filter, JGinv_over_int_cubpts;
  // ---- plot points (src/eles_hexas.cpp:498-521 set_loc_ppts, src/eles.cpp:3600 set_opp_p, :3757 calc_disu_ppts)
  int p_res = 0, n_ppts_per_ele = 0;
  hf_array<double> loc_ppts, opp_p, disu_ppts; // disu_ppts (n_ppts, n_eles, n_fields): filled by calc_disu_ppts_all
  void set_loc_ppts();
  void set_opp_p();
  void calc_pos_ppts(int in_ele, hf_array<double> &out_pos_ppts);   // src/eles.cpp:3714: (n_ppts_per_ele, n_dims) through calc_pos
  int calc_disu_ppts_all();                                         // every element at once, on the device
  void calc_disu_ppts(int in_ele, hf_array<double> &out_disu_ppts); // the reference's per-element accessor
  virtual int set_shock_capture_operators(); // set_vandermonde1D/3D, calc_norm_basis, set_exp_filter; eles_tets / eles_pris override it
  virtual int compute_filter_upts(); // src/eles_hexas.cpp:583, src/eles_quads.cpp:428 (LES_filter); eles_tets overrides it
  // reference length of an element for the CFL time step (calc_h_ref_specific of the class); the box meshes of hexes / quads set
  // h_ref themselves (solver.cpp), the simplex classes here
  virtual double calc_h_ref_specific(int) { return 0.0; }
  hf_array<double> filter_upts_1D, filter_upts;
  int set_over_int();                // set_over_int (cubature points, interpolation, L2-projection filter)
  void tensor_modes(hf_array<int> &deg) const;
  // ---- ASCII restart (src/eles.cpp:655-760,845-870; info blocks src/eles_hexas.cpp:799-890, eles_quads.cpp)
  hf_array<int> ele2global_ele;
  int order_rest = 0, n_upts_per_ele_rest = 0;
  hf_array<double> loc_1d_upts_rest, opp_r;
  void write_restart_info_ascii(std::ostream &restart_file);
  void write_restart_data_ascii(std::ostream &restart_file);
  int read_restart_info_ascii(std::istream &restart_file); // 1 found, 0 not in the file
  int read_restart_data_ascii(std::istream &restart_file); // fills disu_upts(0); returns 0 or fails
  void set_opp_r();

protected:
  virtual int setup_ele_type_specific() = 0;
  virtual double eval_nodal_basis(int in_index, const hf_array<double> &in_loc) = 0;
  virtual double eval_d_nodal_basis(int in_index, int in_cpnt, const hf_array<double> &in_loc) = 0;
  virtual void fill_opp_3(hf_array<double> &opp_3) = 0;
  virtual double eval_nodal_s_basis(int in_index, const hf_array<double> &in_loc, int in_n_spts) = 0;
  virtual void eval_d_nodal_s_basis(hf_array<double> &d_nodal_s_basis, const hf_array<double> &in_loc, int in_n_spts) = 0;

  void set_opp_0();
  void set_opp_1();
  void set_opp_2();
  void set_opp_3();
  void set_opp_4();
  void set_opp_5();
  void set_opp_6();
  void calc_pos(const hf_array<double> &in_loc, int in_ele, hf_array<double> &out_pos);
  void calc_d_pos(const hf_array<double> &in_loc, int in_ele, hf_array<double> &out_d_pos);
  int set_transforms_pts(int which); // 0 solution points, 1 flux points, 2 over-integration cubature points
  void fail(const std::string &msg);

  hfx_eles *dev = nullptr;
  std::string err;
  int max_n_spts_per_ele = 0;
};

class eles_hexas : public eles
{
public:
  int face_plane_vertices(int in_n_spts, int in_face, int v[3]) const override;
  int set_inters_cubpts() override;
  double compute_inter_detjac_inters_cubpts(int in_inter, const hf_array<double> &d_pos) override; // src/eles_hexas.cpp:395

protected:
  int setup_ele_type_specific() override;
  double eval_nodal_basis(int in_index, const hf_array<double> &in_loc) override;
  double eval_d_nodal_basis(int in_index, int in_cpnt, const hf_array<double> &in_loc) override;
  void fill_opp_3(hf_array<double> &opp_3) override;
  double eval_nodal_s_basis(int in_index, const hf_array<double> &in_loc, int in_n_spts) override;
  void eval_d_nodal_s_basis(hf_array<double> &d, const hf_array<double> &in_loc, int in_n_spts) override;
};

class eles_quads : public eles
{
public:
  int face_plane_vertices(int in_n_spts, int in_face, int v[3]) const override;
  int set_inters_cubpts() override;                                                                // src/eles_quads.cpp:251-315
  double compute_inter_detjac_inters_cubpts(int in_inter, const hf_array<double> &d_pos) override; // src/eles_quads.cpp:333

protected:
  int setup_ele_type_specific() override;
  double eval_nodal_basis(int in_index, const hf_array<double> &in_loc) override;
  double eval_d_nodal_basis(int in_index, int in_cpnt, const hf_array<double> &in_loc) override;
  void fill_opp_3(hf_array<double> &opp_3) override;
  double eval_nodal_s_basis(int in_index, const hf_array<double> &in_loc, int in_n_spts) override;
  void eval_d_nodal_s_basis(hf_array<double> &d, const hf_array<double> &in_loc, int in_n_spts) override;
};

// Tetrahedra and triangular prisms (src/eles_tets.cpp, src/eles_pris.cpp) as producers of the dense operators and the
// metrics: csrc/host/eles_simplex.cpp.  4-node / 6-node (straight-sided) shapes.
class eles_tets : public eles
{
public:
  int face_plane_vertices(int in_n_spts, int in_face, int v[3]) const override;

protected:
  int setup_ele_type_specific() override;
  double eval_nodal_basis(int in_index, const hf_array<double> &in_loc) override;
  double eval_d_nodal_basis(int in_index, int in_cpnt, const hf_array<double> &in_loc) override;
  void fill_opp_3(hf_array<double> &opp_3) override;
  double eval_nodal_s_basis(int in_index, const hf_array<double> &in_loc, int in_n_spts) override;
  void eval_d_nodal_s_basis(hf_array<double> &d, const hf_array<double> &in_loc, int in_n_spts) override;
  int compute_filter_upts() override; // src/eles_tets.cpp:576-690 (modal filter, element average)
  double calc_h_ref_specific(int in_ele) override; // src/eles_tets.cpp:1599-1633: the insphere diameter
  int set_shock_capture_operators() override; // src/eles_tets.cpp:705-797 (set_vandermonde, set_exp_filter, shock_det_persson's mode set)
  std::vector<int> mode_i, mode_j, mode_k; // the orthonormal modal basis the nodal one is computed through
  std::vector<double> vinv;                // inverse Vandermonde matrix, row-major
};

class eles_pris : public eles
{
public:
  int face_plane_vertices(int in_n_spts, int in_face, int v[3]) const override;
  eles_pris();
  ~eles_pris() override;
  int n_upts_tri = 0;

protected:
  int setup_ele_type_specific() override;
  double eval_nodal_basis(int in_index, const hf_array<double> &in_loc) override;
  double eval_d_nodal_basis(int in_index, int in_cpnt, const hf_array<double> &in_loc) override;
  void fill_opp_3(hf_array<double> &opp_3) override;
  double eval_nodal_s_basis(int in_index, const hf_array<double> &in_loc, int in_n_spts) override;
  void eval_d_nodal_s_basis(hf_array<double> &d, const hf_array<double> &in_loc, int in_n_spts) override;
  int set_shock_capture_operators() override; // src/eles_pris.cpp:609-730 (set_vandermonde3D, set_exp_filter, calc_norm_basis)
  double calc_h_ref_specific(int in_ele) override; // src/eles_pris.cpp:1535-1557: shortest vertical edge or triangle incircle diameter
  struct Impl;
  Impl *impl;
};
