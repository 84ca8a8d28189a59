// eles_probes.cpp -- point probes of the host mirror: locating a physical point (calc_p2c of the four element classes,
// /root/reference/src/eles_hexas.cpp:1573, eles_quads.cpp:1303, eles_tets.cpp:1636, eles_pris.cpp:1559; eles::pos_to_loc,
// src/eles.cpp:5992-6020), its operator row (eles::set_opp_probe, src/eles.cpp:3625-3631) and the registration of the located
// probes with the device block, which samples them (hfx_eles_set_probes / hfx_eles_sample_probes).
#include <cmath>

#include "eles.hpp"

// ---- the vertices that span the plane (3-D: three, 2-D: the line's two) of local face `in_face`, for the linear shapes --------
// returns the number of faces of the class, or -1 for a shape this build does not locate in
int eles_hexas::face_plane_vertices(int in_n_spts, int in_face, int v[3]) const
{
  if (in_n_spts != 8) return -1;
  // shape node = r + 2 s + 4 t; faces z- y- x+ y+ x- z+
  static const int T[6][3] = {{1, 0, 2}, {0, 1, 5}, {1, 3, 7}, {3, 2, 6}, {2, 0, 4}, {4, 5, 7}};
  for (int k = 0; k < 3; k++) v[k] = T[in_face][k];
  return 6;
}

int eles_quads::face_plane_vertices(int in_n_spts, int in_face, int v[3]) const
{
  if (in_n_spts != 4) return -1;
  // shape node = r + 2 s; faces y- x+ y+ x-
  static const int T[4][2] = {{0, 1}, {1, 3}, {3, 2}, {2, 0}};
  v[0] = T[in_face][0]; v[1] = T[in_face][1]; v[2] = 0;
  return 4;
}

int eles_tets::face_plane_vertices(int, int in_face, int v[3]) const
{
  // (the quadratic tetrahedron keeps its vertices in nodes 0-3: the planes through them, as the reference takes them)
  static const int T[4][3] = {{1, 2, 3}, {0, 3, 2}, {0, 1, 3}, {0, 2, 1}};
  for (int k = 0; k < 3; k++) v[k] = T[in_face][k];
  return 4;
}

int eles_pris::face_plane_vertices(int, int in_face, int v[3]) const
{
  static const int T[5][3] = {{0, 2, 1}, {3, 4, 5}, {0, 1, 4}, {1, 2, 5}, {2, 0, 3}};
  for (int k = 0; k < 3; k++) v[k] = T[in_face][k];
  return 5;
}

// The first element for which in_pos and the centroid of the shape nodes lie on the same side of every face plane (product of
// the two plane values >= 0), or -1.  -2: a shape that is not implemented (probe_error says so, in the reference's words)
int eles::calc_p2c(const hf_array<double> &in_pos)
{
  for (int i = 0; i < n_eles; i++)
  {
    const int ns = n_spts_per_ele(i);
    int v[3];
    const int n_faces = face_plane_vertices(ns, 0, v);
    if (n_faces < 0)
    {
      probe_error = n_dims == 3 ? "elemment type not implemented" : "cell type not implemented";
      return -2;
    }
    double centroid[3] = {0.0, 0.0, 0.0};
    for (int d = 0; d < n_dims; d++)
    {
      for (int j = 0; j < ns; j++) centroid[d] += shape(d, j, i);
      centroid[d] /= (double)ns;
    }
    bool inside = true;
    for (int f = 0; f < n_faces && inside; f++)
    {
      face_plane_vertices(ns, f, v);
      double c[4]; // c0 x + c1 y (+ c2 z) + c3 = 0
      if (n_dims == 3)
      {
        double a[3], b[3];
        for (int d = 0; d < 3; d++)
        {
          a[d] = shape(d, v[1], i) - shape(d, v[0], i);
          b[d] = shape(d, v[2], i) - shape(d, v[0], i);
        }
        c[0] = a[1] * b[2] - a[2] * b[1];
        c[1] = a[2] * b[0] - a[0] * b[2];
        c[2] = a[0] * b[1] - a[1] * b[0];
        c[3] = 0. - (c[0] * shape(0, v[0], i) + c[1] * shape(1, v[0], i) + c[2] * shape(2, v[0], i));
        const double at_pos = c[0] * in_pos(0) + c[1] * in_pos(1) + c[2] * in_pos(2) + c[3];
        const double at_centroid = c[0] * centroid[0] + c[1] * centroid[1] + c[2] * centroid[2] + c[3];
        inside = at_pos * at_centroid >= 0;
      }
      else
      {
        c[0] = shape(1, v[1], i) - shape(1, v[0], i);
        c[1] = shape(0, v[0], i) - shape(0, v[1], i);
        c[2] = 0. - (c[0] * shape(0, v[0], i) + c[1] * shape(1, v[0], i));
        const double at_pos = c[0] * in_pos(0) + c[1] * in_pos(1) + c[2];
        const double at_centroid = c[0] * centroid[0] + c[1] * centroid[1] + c[2];
        inside = at_pos * at_centroid >= 0;
      }
    }
    if (inside) return i;
  }
  return -1;
}

// dx = J^-1 b for the 2 x 2 / 3 x 3 Jacobian J(i, j) = d pos_i / d loc_j, by cofactors
static bool solve_small(int n, const hf_array<double> &J, const double *b, double *dx)
{
  if (n == 2)
  {
    const double det = J(0, 0) * J(1, 1) - J(0, 1) * J(1, 0);
    if (det == 0.0 || !std::isfinite(det)) return false;
    dx[0] = (J(1, 1) * b[0] - J(0, 1) * b[1]) / det;
    dx[1] = (-J(1, 0) * b[0] + J(0, 0) * b[1]) / det;
    return true;
  }
  double co[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
    {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      co[i][j] = J(i1, j1) * J(i2, j2) - J(i1, j2) * J(i2, j1);
    }
  const double det = J(0, 0) * co[0][0] + J(0, 1) * co[0][1] + J(0, 2) * co[0][2];
  if (det == 0.0 || !std::isfinite(det)) return false;
  for (int i = 0; i < 3; i++) dx[i] = (co[0][i] * b[0] + co[1][i] * b[1] + co[2][i] * b[2]) / det; // (J^-1 = adj / det, adj = co^T)
  return true;
}

// Newton's method from loc = 0, until the step is no longer than 1e-6 (src/eles.cpp:5992-6020).  The reference iterates for ever
// on a point that does not converge; here the iteration count is capped and the failure reported
int eles::pos_to_loc(const hf_array<double> &in_pos, int in_ele, hf_array<double> &out_loc)
{
  const int max_iterations = 50;
  hf_array<double> d_pos(n_dims, n_dims), pos(n_dims);
  double rhs[3], dx[3];
  for (int i = 0; i < n_dims; i++) out_loc(i) = 0.0;
  for (int it = 0; it < max_iterations; it++)
  {
    calc_d_pos(out_loc, in_ele, d_pos);
    calc_pos(out_loc, in_ele, pos);
    for (int i = 0; i < n_dims; i++) rhs[i] = -pos(i) + in_pos(i);
    if (!solve_small(n_dims, d_pos, rhs, dx)) break;
    double len2 = 0.;
    for (int i = 0; i < n_dims; i++)
    {
      out_loc(i) += dx[i];
      len2 += dx[i] * dx[i];
    }
    if (!std::isfinite(len2)) break;
    if (!(std::sqrt(len2) > 1.e-6)) return 0;
  }
  probe_error = "pos_to_loc: Newton's method did not converge in element " + std::to_string(in_ele);
  return 1;
}

void eles::set_opp_probe(const hf_array<double> &in_loc)
{
  opp_probe.setup(n_upts_per_ele);
  for (int i = 0; i < n_upts_per_ele; i++) opp_probe(i) = eval_nodal_basis(i, in_loc);
}

void eles::calc_pos_probe(const hf_array<double> &in_loc, int in_ele, hf_array<double> &out_pos) { calc_pos(in_loc, in_ele, out_pos); }

// Locates positions (n_dims, n) column-major: every point found in an element of this class becomes a probe of it, a point
// found in none is not this rank's (as in the reference).  A refusal (probe_error) leaves the probes as they were.  Host only:
// register_probes hands them to the device block
int eles::locate_probes(int n, const double *positions)
{
  std::vector<int> p2c, global;
  std::vector<double> loc, opp;
  hf_array<double> pos(n_dims), l(n_dims);
  for (int i = 0; i < n; i++)
  {
    for (int d = 0; d < n_dims; d++) pos(d) = positions[d + (size_t)n_dims * i];
    const int ele = calc_p2c(pos);
    if (ele == -2) return 1;
    if (ele < 0) continue;
    if (pos_to_loc(pos, ele, l)) return 1;
    set_opp_probe(l);
    p2c.push_back(ele);
    global.push_back(i);
    for (int d = 0; d < n_dims; d++) loc.push_back(l(d));
    for (int k = 0; k < n_upts_per_ele; k++) opp.push_back(opp_probe(k));
  }
  probe_p2c.swap(p2c);
  probe_global.swap(global);
  probe_loc.swap(loc);
  probe_opp.swap(opp);
  return 0;
}

int eles::register_probes()
{
  if (!dev) return 0; // (mv_all_cpu_gpu registers them)
  if (hfx_eles_set_probes(dev, (int)probe_p2c.size(), probe_p2c.data(), probe_opp.data())) { fail(hfx_last_error()); return 1; }
  return 0;
}

void eles::sample_probes(double time, int step)
{
  if (n_eles == 0 || probe_p2c.empty()) return;
  if (!dev) { fail("element block is not on the device"); return; }
  if (hfx_eles_sample_probes(dev, time, step)) fail(hfx_last_error());
}
