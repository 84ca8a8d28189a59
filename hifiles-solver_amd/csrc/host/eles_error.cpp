// eles_error.cpp -- the volume cubature of the tensor-product classes and the two monitors that integrate over it: the
// exact-solution error norms (eles::compute_error, src/eles.cpp:5076-5277) and the integral diagnostics
// (eles::CalcIntegralQuantities, src/eles.cpp:5485-5627).  The host builds the rule, the operator, the determinants and the
// positions, as the reference's setup does when run_input.test_case != 0 or n_integral_quantities != 0 (src/eles_hexas.cpp:87,
// src/eles_quads.cpp:97); the sums run on the device (csrc/error_norm.hip, hfx_eles_CalcIntegralQuantities).
#include <cmath>

#include "basis.hpp"
#include "eles.hpp"

// set_volume_cubpts (src/eles_hexas.cpp:376, src/eles_quads.cpp:317): the tensor Gauss rule with order + 1 points per direction,
// first direction fastest; set_opp_volume_cubpts (src/eles.cpp:3667); set_transforms_vol_cubpts (src/eles.cpp:4600-4633); and for a
// test case the positions compute_error takes from calc_pos on every call (src/eles.cpp:5095-5097).  Neither monitor asked for:
// none of the five arrays exists.
int eles::set_volume_cubature()
{
  const bool on = run_input->test_case != 0 || run_input->n_integral_quantities != 0;
  loc_volume_cubpts.setup(0); weight_volume_cubpts.setup(0); opp_volume_cubpts.setup(0); vol_detjac_vol_cubpts.setup(0);
  pos_volume_cubpts.setup(0);
  if (!on || n_eles == 0) return 0;
  if (ele_type != 1 && ele_type != 4)
  {
    fail("volume cubature: quadrilaterals and hexahedra only in this mirror");
    return 1;
  }
  const int Nc = order + 1;
  hf_array<double> c1, w1;
  cubature_1d_nodes(0, Nc, c1, w1);
  int n_cub = 1;
  for (int d = 0; d < n_dims; d++) n_cub *= Nc;
  loc_volume_cubpts.setup(n_dims, n_cub);
  weight_volume_cubpts.setup(n_cub);
  for (int q = 0; q < n_cub; q++)
  {
    int r = q;
    double w = 1.0;
    for (int d = 0; d < n_dims; d++)
    {
      loc_volume_cubpts(d, q) = c1(r % Nc);
      w *= w1(r % Nc);
      r /= Nc;
    }
    weight_volume_cubpts(q) = w;
  }
  hf_array<double> loc(n_dims), d_pos(n_dims, n_dims), pos(n_dims);
  opp_volume_cubpts.setup(n_cub, n_upts_per_ele);
  for (int i = 0; i < n_upts_per_ele; i++)
    for (int j = 0; j < n_cub; j++)
    {
      for (int k = 0; k < n_dims; k++) loc(k) = loc_volume_cubpts(k, j);
      opp_volume_cubpts(j, i) = eval_nodal_basis(i, loc);
    }
  // (the reference keeps one array of n_eles values per cubature point; here the point is the first index of one array)
  vol_detjac_vol_cubpts.setup(n_cub, n_eles);
  if (run_input->test_case != 0) pos_volume_cubpts.setup(n_cub, n_eles, n_dims);
  for (int i = 0; i < n_eles; i++)
    for (int j = 0; j < n_cub; j++)
    {
      for (int m = 0; m < n_dims; m++) loc(m) = loc_volume_cubpts(m, j);
      calc_d_pos(loc, i, d_pos);
      if (n_dims == 2)
        vol_detjac_vol_cubpts(j, i) = d_pos(0, 0) * d_pos(1, 1) - d_pos(0, 1) * d_pos(1, 0);
      else
        vol_detjac_vol_cubpts(j, i) = d_pos(0, 0) * (d_pos(1, 1) * d_pos(2, 2) - d_pos(1, 2) * d_pos(2, 1)) -
                                      d_pos(0, 1) * (d_pos(1, 0) * d_pos(2, 2) - d_pos(1, 2) * d_pos(2, 0)) +
                                      d_pos(0, 2) * (d_pos(1, 0) * d_pos(2, 1) - d_pos(1, 1) * d_pos(2, 0));
      if (run_input->test_case != 0)
      {
        calc_pos(loc, i, pos);
        for (int m = 0; m < n_dims; m++) pos_volume_cubpts(j, i, m) = pos(m);
      }
    }
  return 0;
}

int eles::register_volume_cubature()
{
  if (!dev || weight_volume_cubpts.get_dim(0) == 0) return 0; // (mv_all_cpu_gpu registers it | nothing to register)
  if (hfx_eles_set_volume_cubpts(dev, weight_volume_cubpts.get_dim(0), opp_volume_cubpts.get_ptr_cpu(), weight_volume_cubpts.get_ptr_cpu(),
                                 vol_detjac_vol_cubpts.get_ptr_cpu()))
  {
    fail(hfx_last_error());
    return 1;
  }
  if (pos_volume_cubpts.get_dim(0) != 0 && hfx_eles_set_error_points(dev, pos_volume_cubpts.get_ptr_cpu()))
  {
    fail(hfx_last_error());
    return 1;
  }
  return 0;
}

int eles::compute_error(int in_norm_type, double &time, hf_array<double> &error)
{
  if (!dev) { fail("element block is not on the device"); return 1; }
  error.setup(2, n_fields);
  if (hfx_eles_compute_error(dev, in_norm_type, time, error.get_ptr_cpu())) { fail(hfx_last_error()); return 1; }
  return 0;
}

int eles::CalcIntegralQuantities(int n_integral_quantities, hf_array<double> &integral_quantities)
{
  if (!dev) { fail("element block is not on the device"); return 1; }
  int ids[8];
  for (int m = 0; m < n_integral_quantities; m++) ids[m] = run_input->integral_quantity_code(m);
  if (hfx_eles_CalcIntegralQuantities(dev, n_integral_quantities, ids, integral_quantities.get_ptr_cpu())) { fail(hfx_last_error()); return 1; }
  return 0;
}
