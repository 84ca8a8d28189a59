// Stand-alone host program around hfx::wall_stress (hifiles-solver_amd/csrc/wall_model.hpp): TEST INFRASTRUCTURE.
// Compiled by tests/test_wall_model_host.py with the system compiler; no device, no HIP header.
//
//   wall_model_host_main <cases> : one case per line
//     nd model gamma prandtl rt_inf mu_inf c_sth fix_vis prandtl_t Kappa dist  u_wm[nd+2]  u_w[nd+2]  n[nd]
//   (numbers in any form strtod reads, hexadecimal floats included) -> one line per case: fn[nd+2] as hexadecimal floats, then the
//   Newton iterations model 2 took (0 for model 1)
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

#include "wall_model.hpp"

template <int ND>
static void run(int model, const hfx::WallModelPhys &P, double prandtl_t, double Kappa, double dist, const std::vector<double> &v)
{
  double u_wm[ND + 2], u_w[ND + 2], n[ND], fn[ND + 2];
  for (int k = 0; k < ND + 2; k++) u_wm[k] = v[k];
  for (int k = 0; k < ND + 2; k++) u_w[k] = v[ND + 2 + k];
  for (int k = 0; k < ND; k++) n[k] = v[2 * (ND + 2) + k];
  int it = 0;
  hfx::wall_stress<ND>(model, P, prandtl_t, Kappa, u_wm, u_w, dist, n, fn, &it);
  for (int k = 0; k < ND + 2; k++) std::printf("%a ", fn[k]);
  std::printf("%d\n", it);
}

int main(int argc, char **argv)
{
  if (argc != 2) return 2;
  std::FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char line[4096];
  while (std::fgets(line, sizeof line, f))
  {
    std::vector<double> t;
    char *p = line, *end = nullptr;
    for (;;)
    {
      const double x = std::strtod(p, &end);
      if (end == p) break;
      t.push_back(x);
      p = end;
    }
    if (t.empty()) continue;
    const int nd = (int)t[0], model = (int)t[1];
    if ((nd != 2 && nd != 3) || t.size() != (size_t)(11 + 2 * (nd + 2) + nd)) return 3;
    const hfx::WallModelPhys P{t[2], t[3], t[4], t[5], t[6], t[7]};
    const std::vector<double> v(t.begin() + 11, t.end());
    if (nd == 2)
      run<2>(model, P, t[8], t[9], t[10], v);
    else
      run<3>(model, P, t[8], t[9], t[10], v);
  }
  std::fclose(f);
  return 0;
}
