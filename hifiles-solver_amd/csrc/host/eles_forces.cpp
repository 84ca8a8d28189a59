// eles_forces.cpp -- what the host builds for the wall-force monitor (run_input->calc_force; output::CalcForces,
// src/output.cpp:1915-2014): the surface cubature of the quadrilaterals (the hexahedra's is in eles_forcing.cpp), the wall faces,
// the positions of their cubature points, and the registration with libhfx.  The forces themselves
// (eles::compute_wall_forces, src/eles.cpp:5704-5990) are computed on the device (csrc/wall_force.hip).
//
// The wall faces: the reference walks bdy_ele2ele -- the elements with at least one face in a boundary group, ascending
// (src/eles.cpp:4396-4433) -- and every local face of each, and asks run_input.bc_list(bcid(ele, l)) for its kind.  bcid is -1 on
// the local faces that belong to no group (src/geometry.cpp:292), so that read is out of bounds and the reference's totals take
// in whatever interior faces the stray flag happens to call a wall.  Here a face is taken when its bcid names a group of one of
// the four wall kinds, and only then.
#include <cmath>

#include "basis.hpp"
#include "eles.hpp"

// src/eles_quads.cpp:251-315: the 1-D Gauss rule of `order` (order + 1 points) along every side; sides 2 and 3 run backwards
int eles_quads::set_inters_cubpts()
{
  const int N = order + 1;
  hf_array<double> x1, w1;
  cubature_1d_nodes(0, N, x1, w1);
  n_cubpts_per_inter.setup(n_inters_per_ele);
  loc_inters_cubpts.setup(n_inters_per_ele);
  weight_inters_cubpts.setup(n_inters_per_ele);
  tnorm_inters_cubpts.setup(n_inters_per_ele);
  static const double TN[4][2] = {{0., -1.}, {1., 0.}, {0., 1.}, {-1., 0.}};
  for (int i = 0; i < n_inters_per_ele; i++)
  {
    n_cubpts_per_inter(i) = N;
    loc_inters_cubpts(i).setup(n_dims, N);
    weight_inters_cubpts(i).setup(N);
    tnorm_inters_cubpts(i).setup(n_dims, N);
    for (int j = 0; j < N; j++)
    {
      if (i == 0) { loc_inters_cubpts(i)(0, j) = x1(j); loc_inters_cubpts(i)(1, j) = -1.; }
      else if (i == 1) { loc_inters_cubpts(i)(0, j) = 1.; loc_inters_cubpts(i)(1, j) = x1(j); }
      else if (i == 2) { loc_inters_cubpts(i)(0, j) = x1(N - j - 1); loc_inters_cubpts(i)(1, j) = 1.0; }
      else { loc_inters_cubpts(i)(0, j) = -1.0; loc_inters_cubpts(i)(1, j) = x1(N - j - 1); }
      weight_inters_cubpts(i)(j) = w1(j);
      tnorm_inters_cubpts(i)(0, j) = TN[i][0];
      tnorm_inters_cubpts(i)(1, j) = TN[i][1];
    }
  }
  set_opp_inters_cubpts();
  return 0;
}

// src/eles_quads.cpp:333-363: the length of the side's tangent
double eles_quads::compute_inter_detjac_inters_cubpts(int in_inter, const hf_array<double> &d_pos)
{
  const double xr = d_pos(0, 0), xs = d_pos(0, 1), yr = d_pos(1, 0), ys = d_pos(1, 1);
  return (in_inter == 0 || in_inter == 2) ? std::sqrt(xr * xr + yr * yr) : std::sqrt(xs * xs + ys * ys);
}

static bool is_wall(int flag)
{
  return flag == HFX_BC_SLIP_WALL || flag == HFX_BC_ISOTHERM_WALL || flag == HFX_BC_ADIABAT_WALL || flag == HFX_BC_SLIP_WALL_DUAL;
}

void eles::set_wall_inters()
{
  wall_ele.clear(); wall_inter.clear(); wall_flag.clear(); wall_n_points.clear(); wall_pos.clear();
  wall_cp.clear(); wall_cf.clear();
  if (n_cubpts_per_inter.get_dim(0) != n_inters_per_ele || bcid.get_dim(0) != n_eles) return;
  hf_array<double> loc(n_dims), pos(n_dims);
  for (int i = 0; i < n_eles; i++)
    for (int l = 0; l < n_inters_per_ele; l++)
    {
      const int g = bcid(i, l);
      if (g < 0 || g >= (int)run_input->bc_list.size() || !is_wall(run_input->bc_list[g].flag)) continue;
      wall_ele.push_back(i);
      wall_inter.push_back(l);
      wall_flag.push_back(run_input->bc_list[g].flag);
      wall_n_points.push_back(n_cubpts_per_inter(l));
      // the rows of the cp file: j descending (src/eles.cpp:5773), the position through calc_pos (:5782-5785), once
      for (int j = n_cubpts_per_inter(l) - 1; j >= 0; j--)
      {
        for (int m = 0; m < n_dims; m++) loc(m) = loc_inters_cubpts(l)(m, j);
        calc_pos(loc, i, pos);
        for (int m = 0; m < n_dims; m++) wall_pos.push_back(pos(m));
      }
    }
}

int eles::register_wall_forces()
{
  if (!dev) return 0; // (mv_all_cpu_gpu registers them)
  std::vector<const double *> opp(n_inters_per_ele), wgt(n_inters_per_ele);
  for (int l = 0; l < n_inters_per_ele; l++)
  {
    opp[l] = opp_inters_cubpts(l).get_ptr_cpu();
    wgt[l] = weight_inters_cubpts(l).get_ptr_cpu();
  }
  // per listed face: detjac (n_cubpts), norm (n_cubpts, n_dims)
  std::vector<double> detjac, norm;
  for (size_t f = 0; f < wall_ele.size(); f++)
  {
    const int l = wall_inter[f], i = wall_ele[f], nc = n_cubpts_per_inter(l);
    for (int j = 0; j < nc; j++) detjac.push_back(inter_detjac_inters_cubpts(l)(j, i));
    for (int m = 0; m < n_dims; m++)
      for (int j = 0; j < nc; j++) norm.push_back(norm_inters_cubpts(l)(j, i, m));
  }
  if (hfx_eles_set_wall_faces(dev, (int)wall_ele.size(), wall_ele.data(), wall_inter.data(), wall_flag.data(), n_inters_per_ele,
                              n_cubpts_per_inter.get_ptr_cpu(), opp.data(), wgt.data(), detjac.data(), norm.data()))
  {
    fail(hfx_last_error());
    return 1;
  }
  return 0;
}

int eles::compute_wall_forces(hf_array<double> &inv_force, hf_array<double> &vis_force, double &temp_cl, double &temp_cd)
{
  if (!dev) { fail("element block is not on the device"); return 1; }
  inv_force.setup(n_dims);
  vis_force.setup(n_dims);
  size_t np = 0;
  for (int n : wall_n_points) np += (size_t)n;
  std::vector<double> cp(np + 1), cf(np + 1);
  if (hfx_eles_compute_wall_forces(dev, inv_force.get_ptr_cpu(), vis_force.get_ptr_cpu(), &temp_cl, &temp_cd, cp.data(), cf.data()))
  {
    fail(hfx_last_error());
    return 1;
  }
  // into the order of the cp file: inside a face j descending
  wall_cp.assign(np, 0.0);
  wall_cf.assign(np, 0.0);
  size_t first = 0;
  for (int n : wall_n_points)
  {
    for (int r = 0; r < n; r++)
    {
      wall_cp[first + r] = cp[first + (n - 1 - r)];
      wall_cf[first + r] = cf[first + (n - 1 - r)];
    }
    first += (size_t)n;
  }
  return 0;
}
