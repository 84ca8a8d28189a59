// eles_forcing.cpp -- what the host builds for the mass-flux body force of periodic channels (run_input->forcing): the cubature of
// the element faces, the surface metrics at its points, the inflow faces, and the registration with libhfx.  The evaluation
// itself (eles::evaluate_body_force, src/eles.cpp:5281-5482) runs on the device (csrc/forcing.hip).
//
// Definitions follow the reference:
//   face rule     tensor Gauss rule with order + 1 points per direction, first direction fastest (src/eles_hexas.cpp:284-373,
//                 src/cubature_quad.cpp:49-72)
//   opp           opp_inters_cubpts(l)(j, k) = l_k(cubature point j of face l)          (src/eles.cpp:3635-3665)
//   metrics       unit normal = the transformed normal taken through det(J) J^-1, normalised; surface Jacobian = |x_u x x_v| of the
//                 two reference directions u, v that span the face                      (src/eles.cpp:4480-4595, src/eles_hexas.cpp:395)
#include <cmath>

#include "basis.hpp"
#include "eles.hpp"

int eles::set_inters_cubpts()
{
  fail("surface cubature: built for quadrilaterals and hexahedra (register the arrays of other classes with hfx_eles_set_body_force / "
       "hfx_eles_set_wall_faces)");
  return 1;
}

// hexahedra: the reference coordinate that is fixed on local face l and its value there; the other two span the face, ascending
static const int HEX_FIXED[6] = {2, 1, 0, 1, 0, 2};
static const double HEX_AT[6] = {-1.0, -1.0, 1.0, 1.0, -1.0, 1.0};

int eles_hexas::set_inters_cubpts()
{
  const int N = order + 1, nq = N * N;
  hf_array<double> x1, w1;
  cubature_1d_nodes(0, N, x1, w1);
  n_cubpts_per_inter.setup(n_inters_per_ele);
  loc_inters_cubpts.setup(n_inters_per_ele);
  weight_inters_cubpts.setup(n_inters_per_ele);
  tnorm_inters_cubpts.setup(n_inters_per_ele);
  for (int l = 0; l < n_inters_per_ele; l++)
  {
    n_cubpts_per_inter(l) = nq;
    loc_inters_cubpts(l).setup(n_dims, nq);
    weight_inters_cubpts(l).setup(nq);
    tnorm_inters_cubpts(l).setup(n_dims, nq);
    const int fx = HEX_FIXED[l], u = (fx == 0) ? 1 : 0, v = (fx == 2) ? 1 : 2;
    for (int b = 0; b < N; b++)
      for (int a = 0; a < N; a++)
      {
        const int j = a + N * b;
        loc_inters_cubpts(l)(u, j) = x1(a);
        loc_inters_cubpts(l)(v, j) = x1(b);
        loc_inters_cubpts(l)(fx, j) = HEX_AT[l];
        weight_inters_cubpts(l)(j) = w1(a) * w1(b);
        for (int d = 0; d < n_dims; d++) tnorm_inters_cubpts(l)(d, j) = (d == fx) ? HEX_AT[l] : 0.0;
      }
  }
  set_opp_inters_cubpts();
  return 0;
}

void eles::set_opp_inters_cubpts()
{
  hf_array<double> loc(n_dims);
  opp_inters_cubpts.setup(n_inters_per_ele);
  for (int l = 0; l < n_inters_per_ele; l++)
  {
    opp_inters_cubpts(l).setup(n_cubpts_per_inter(l), n_upts_per_ele);
    for (int j = 0; j < n_cubpts_per_inter(l); j++)
    {
      for (int d = 0; d < n_dims; d++) loc(d) = loc_inters_cubpts(l)(d, j);
      for (int k = 0; k < n_upts_per_ele; k++) opp_inters_cubpts(l)(j, k) = eval_nodal_basis(k, loc);
    }
  }
}

double eles_hexas::compute_inter_detjac_inters_cubpts(int in_inter, const hf_array<double> &d_pos)
{
  const int fx = HEX_FIXED[in_inter], u = (fx == 0) ? 1 : 0, v = (fx == 2) ? 1 : 2;
  const double xu = d_pos(0, u), yu = d_pos(1, u), zu = d_pos(2, u);
  const double xv = d_pos(0, v), yv = d_pos(1, v), zv = d_pos(2, v);
  const double c0 = yu * zv - zu * yv, c1 = zu * xv - xu * zv, c2 = xu * yv - yu * xv;
  return std::sqrt(c0 * c0 + c1 * c1 + c2 * c2);
}

void eles::set_transforms_inters_cubpts()
{
  hf_array<double> loc(n_dims), d_pos(n_dims, n_dims);
  inter_detjac_inters_cubpts.setup(n_inters_per_ele);
  norm_inters_cubpts.setup(n_inters_per_ele);
  for (int l = 0; l < n_inters_per_ele; l++)
  {
    inter_detjac_inters_cubpts(l).setup(n_cubpts_per_inter(l), n_eles);
    norm_inters_cubpts(l).setup(n_cubpts_per_inter(l), n_eles, n_dims);
  }
  const bool trilinear = ele_type == 4 && max_n_spts_per_ele == 8;
  hf_array<double> d_s_basis(max_n_spts_per_ele, n_dims);
  for (int i = 0; i < n_eles; i++)
    for (int l = 0; l < n_inters_per_ele; l++)
      for (int j = 0; j < n_cubpts_per_inter(l); j++)
      {
        for (int d = 0; d < n_dims; d++) loc(d) = loc_inters_cubpts(l)(d, j);
        if (trilinear)
        {
          // d(pos)/d(loc) of a trilinear hexahedron as sums over its four edges along each reference direction.  The difference
          // of an edge's two nodes is taken first, so a direction in which the element does not extend contributes exactly
          // nothing: on a box of parallel cells the normals are the axis directions to the last bit, which the inflow rule's
          // `== -1` reads.  (calc_d_pos adds the eight nodes one by one and leaves rounding noise of 1e-17 there.)
          eval_d_nodal_s_basis(d_s_basis, loc, 8);
          for (int d = 0; d < 3; d++)
            for (int k = 0; k < 3; k++)
            {
              double q = 0.0;
              for (int s = 0; s < 8; s++)
                if (s & (1 << k)) q += d_s_basis(s, k) * (shape(d, s, i) - shape(d, s ^ (1 << k), i));
              d_pos(d, k) = q;
            }
        }
        else
          calc_d_pos(loc, i, d_pos);
        if (n_dims == 2)
        {
          // src/eles.cpp:4529-4554
          const double t0 = tnorm_inters_cubpts(l)(0, j), t1 = tnorm_inters_cubpts(l)(1, j);
          const double v0 = (t0 * d_pos(1, 1)) - (t1 * d_pos(1, 0));
          const double v1 = -(t0 * d_pos(0, 1)) + (t1 * d_pos(0, 0));
          const double mag = std::sqrt(v0 * v0 + v1 * v1);
          norm_inters_cubpts(l)(j, i, 0) = v0 / mag;
          norm_inters_cubpts(l)(j, i, 1) = v1 / mag;
          inter_detjac_inters_cubpts(l)(j, i) = compute_inter_detjac_inters_cubpts(l, d_pos);
          continue;
        }
        const double xr = d_pos(0, 0), xs = d_pos(0, 1), xt = d_pos(0, 2);
        const double yr = d_pos(1, 0), ys = d_pos(1, 1), yt = d_pos(1, 2);
        const double zr = d_pos(2, 0), zs = d_pos(2, 1), zt = d_pos(2, 2);
        // the transformed normal through det(J) J^-1 (the cofactors, as at the flux points), then its length
        const double t0 = tnorm_inters_cubpts(l)(0, j), t1 = tnorm_inters_cubpts(l)(1, j), t2 = tnorm_inters_cubpts(l)(2, j);
        const double v0 = (t0 * (ys * zt - yt * zs)) + (t1 * (yt * zr - yr * zt)) + (t2 * (yr * zs - ys * zr));
        const double v1 = (t0 * (xt * zs - xs * zt)) + (t1 * (xr * zt - xt * zr)) + (t2 * (xs * zr - xr * zs));
        const double v2 = (t0 * (xs * yt - xt * ys)) + (t1 * (xt * yr - xr * yt)) + (t2 * (xr * ys - xs * yr));
        const double mag = std::sqrt(v0 * v0 + v1 * v1 + v2 * v2);
        norm_inters_cubpts(l)(j, i, 0) = v0 / mag;
        norm_inters_cubpts(l)(j, i, 1) = v1 / mag;
        norm_inters_cubpts(l)(j, i, 2) = v2 / mag;
        inter_detjac_inters_cubpts(l)(j, i) = compute_inter_detjac_inters_cubpts(l, d_pos);
      }
}

void eles::set_inflow_inters()
{
  inflow_ele.clear();
  inflow_inter.clear();
  if (n_cubpts_per_inter.get_dim(0) != n_inters_per_ele || cyclic_inter.get_dim(0) != n_eles) return;
  for (int i = 0; i < n_eles; i++)
    for (int l = 0; l < n_inters_per_ele; l++)
      if (cyclic_inter(i, l) && norm_inters_cubpts(l)(0, i, 0) == -1) // the inflow plane's normal is -x, exactly
      {
        inflow_ele.push_back(i);
        inflow_inter.push_back(l);
      }
}

int eles::register_body_force()
{
  if (!dev) return 0; // (mv_all_cpu_gpu registers it)
  std::vector<const double *> opp(n_inters_per_ele), wgt(n_inters_per_ele);
  for (int l = 0; l < n_inters_per_ele; l++)
  {
    opp[l] = opp_inters_cubpts(l).get_ptr_cpu();
    wgt[l] = weight_inters_cubpts(l).get_ptr_cpu();
  }
  std::vector<double> detjac;
  for (size_t f = 0; f < inflow_ele.size(); f++)
    for (int j = 0; j < n_cubpts_per_inter(inflow_inter[f]); j++)
      detjac.push_back(inter_detjac_inters_cubpts(inflow_inter[f])(j, inflow_ele[f]));
  if (hfx_eles_set_body_force(dev, (int)inflow_ele.size(), inflow_ele.data(), inflow_inter.data(), n_inters_per_ele,
                              n_cubpts_per_inter.get_ptr_cpu(), opp.data(), wgt.data(), detjac.data(), run_input->forcing_area,
                              run_input->forcing_mdot0, run_input->forcing_history))
  {
    fail(hfx_last_error());
    return 1;
  }
  return 0;
}

int eles::body_force_integrals(double integral[2])
{
  integral[0] = integral[1] = 0.0;
  if (n_eles != 0 && hfx_eles_body_force_integrals(dev, integral) != 0) { fail(hfx_last_error()); return 1; }
  return 0;
}

int eles::body_force_apply(const double integral[2])
{
  if (n_eles != 0 && hfx_eles_body_force_apply(dev, integral) != 0) { fail(hfx_last_error()); return 1; }
  return 0;
}

void eles::evaluate_body_force(int /*in_file_num*/)
{
  // (the device's record knows its first evaluation, where the reference compares in_file_num, src/eles.cpp:5398-5401)
  if (n_eles != 0 && hfx_eles_evaluate_body_force(dev) != 0) fail(hfx_last_error());
}
