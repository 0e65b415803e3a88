// Host-side print of the per-coordinate second moments that build_orbits (gaussianvi_amd/csrc/orbits.hpp) derives from a
// table for the odd part of psi: tau2[c] = 2 sum_k w_k z_kc^2.
// usage: orbit_tau file d N   -- file: N x d doubles Z (row-major) followed by N doubles w, little endian;
// prints "tau2 c <hex float>" per coordinate and "ok d N smax", exit code 1 on any failure
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../gaussianvi_amd/csrc/orbits.hpp"

using namespace gvi;

int main(int argc, char** argv) {
  if (argc != 4) { std::printf("FAIL usage\n"); return 1; }
  const int d = std::atoi(argv[2]);
  const long long N = std::atoll(argv[3]);
  if (d < 1 || N < 1) { std::printf("FAIL arguments\n"); return 1; }
  std::vector<double> Z((size_t)N * d), w((size_t)N);
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::printf("FAIL open\n"); return 1; }
  const bool read = std::fread(Z.data(), 8, Z.size(), f) == Z.size() && std::fread(w.data(), 8, w.size(), f) == w.size();
  std::fclose(f);
  if (!read) { std::printf("FAIL read\n"); return 1; }
  const OrbitHost o = build_orbits(d, N, Z.data(), w.data(), true);
  if (!o.ok || (int)o.tau2.size() != d) { std::printf("FAIL build_orbits\n"); return 1; }
  for (int c = 0; c < d; ++c) std::printf("tau2 %d %a\n", c, o.tau2[(size_t)c]);
  std::printf("ok %d %lld %d\n", d, N, o.smax);
  return 0;
}
