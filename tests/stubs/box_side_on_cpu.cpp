// gaussianvi_amd/csrc/box_moments.hpp -- the functions the HINGE_BOX kernels call -- compiled for the CPU and run on a grid.
// Built with AddressSanitizer and UBSan by tests/test_box_host.py, which compares the printed values with tests/box_ref.py.
//   side <sigma> <sd> <gap> <sgn> <e0> <e1> <e2>          box_side, hex floats
//   coord <case> <e0> <e1> <e2>                           box_coordinate on a d = 4 block with every combination of sides
//   point <case> <psi> <margin>                           psi_hinge_box / box_margin of that block
#include <cstdio>
#include <limits>
#include <vector>

#include "box_moments.hpp"

int main() {
  const double ts[] = {-40.0, -9.0, -6.0, -4.0, -2.5, -1.5, -1.0, -0.3, 0.0, 1e-9, 0.3, 1.0, 1.5, 2.5, 4.0, 6.0, 9.0, 40.0};
  for (double sigma : {0.5, 3.0})
    for (double sd : {0.05, 0.7, 0.0})
      for (double t : ts)
        for (double sgn : {1.0, -1.0}) {
          const double gap = sd > 0.0 ? t * sd : t * 0.01;
          const gvi::BoxSide r = gvi::box_side(sigma, sd, gap, sgn);
          std::printf("side %a %a %a %a %a %a %a\n", sigma, sd, gap, sgn, r.e0, r.e1, r.e2);
        }
  const double inf = std::numeric_limits<double>::infinity();
  const int d = 4;
  // [sigma | eps | lo | hi]: coordinate 0 upper side only, 1 without limits, 2 both sides, 3 lower side only
  const std::vector<double> p = {1.5, 2.0, 2.5, 3.0, 0.1, 0.1, 0.2, 0.0, -inf, -inf, -1.0, -0.5, 1.0, inf, 1.0, inf};
  const double ms[3][4] = {{0.95, 7.0, -0.9, -0.45}, {0.0, -3.0, 0.0, 1.0}, {2.0, 0.0, 1.2, -2.0}};
  for (int c = 0; c < 3; ++c) {
    for (int i = 0; i < d; ++i) {
      const gvi::BoxSide r = gvi::box_coordinate(p.data(), d, i, ms[c][i], 0.3);
      std::printf("coord %d %d %a %a %a\n", c, i, r.e0, r.e1, r.e2);
    }
    std::printf("point %d %a %a\n", c, gvi::psi_hinge_box(p.data(), ms[c], d), gvi::box_margin(p.data(), ms[c], d));
  }
  std::printf("ALL OK\n");
  return 0;
}
