// gaussianvi_amd/csrc/halfspace_moments.hpp -- the functions the HINGE_HALFSPACE kernels call -- compiled for the CPU and run on
// the cases of a file.  Built with AddressSanitizer and UBSan by tests/test_halfspace_host.py, which writes the cases and compares
// the printed values with tests/halfspace_ref.py.  Every buffer is a std::vector of exactly the size the functions may touch, so
// a read or write past a parameter block, a root or a v_j is reported.
//   input   <ncases>, then per case: <d> <J> | p [J (d + 3)] | mu [d] | S [d d] (row-major root, x = mu + S z) | x [d]
//   row <case> <j> <e0> <e1> <e2>                          halfspace_row, hex floats
//   mom <case> <m0> <m1 [d]> <M2 [d d]>                    E[psi], E[z psi], E[z z^T psi] assembled in ascending j
//   point <case> <psi> <margin>                            psi_hinge_halfspace / halfspace_margin at x
#include <cstdio>
#include <vector>

#include "halfspace_moments.hpp"

static bool read(std::FILE* f, std::vector<double>& v, size_t n) {
  v.assign(n, 0.0);
  for (size_t i = 0; i < n; ++i)
    if (std::fscanf(f, "%lf", &v[i]) != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "r");
  int ncases = 0;
  if (!f || std::fscanf(f, "%d", &ncases) != 1) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  for (int c = 0; c < ncases; ++c) {
    int d = 0, J = 0;
    std::vector<double> p, mu, S, x;
    if (std::fscanf(f, "%d %d", &d, &J) != 2 || !read(f, p, (size_t)J * (d + 3)) || !read(f, mu, d) || !read(f, S, (size_t)d * d) ||
        !read(f, x, d)) {
      std::fprintf(stderr, "case %d: short input\n", c);
      return 2;
    }
    std::vector<double> v(d), m1(d, 0.0), M2((size_t)d * d, 0.0);
    double m0 = 0.0;
    for (int j = 0; j < J; ++j) {
      v.assign(d, 0.0);                         // an off row writes nothing: it then adds exact zeros
      const gvi::BoxSide r = gvi::halfspace_row(p.data(), d, J, j, mu.data(), S.data(), v.data());
      std::printf("row %d %d %a %a %a\n", c, j, r.e0, r.e1, r.e2);
      m0 += r.e0;
      for (int a = 0; a < d; ++a) {
        m1[a] += v[a] * r.e1;
        for (int b = 0; b < d; ++b) M2[(size_t)a * d + b] += v[a] * v[b] * r.e2;
      }
    }
    for (int a = 0; a < d; ++a) M2[(size_t)a * d + a] += m0;
    std::printf("mom %d %a", c, m0);
    for (double t : m1) std::printf(" %a", t);
    for (double t : M2) std::printf(" %a", t);
    std::printf("\npoint %d %a %a\n", c, gvi::psi_hinge_halfspace(p.data(), x.data(), d, J), gvi::halfspace_margin(p.data(), x.data(), d, J));
  }
  std::fclose(f);
  std::printf("ALL OK\n");
  return 0;
}
