// gaussianvi_amd/csrc/psi_point.hpp -- psi_point and hinge_psi_clearance, the chain from a psi kind to its psi at one state that
// the generic and the sample-cost kernels run -- compiled for the CPU on a FactorDev of host pointers and run on the cases of a
// file.  Built plain and with AddressSanitizer / UBSan by tests/test_psi_point_host.py, which writes the cases and compares the
// printed values with the oracle and the numpy references.  Every buffer (parameter block, grid, arm model, each state) is a
// std::vector of exactly the size the code may touch, so a look-up or a walk that leaves one is reported.
//   input   <ncases>, then per case
//     <kind> <d> <J> <raw_stride> <N> | <rows> <cols> <nz> <ox> <oy> <oz> <cell> | field [rows cols max(nz, 1)] (r + c rows + z rows
//     cols; rows = 0: no grid) | <narm> | arm [narm] (the packed model of gvi_factors_set_arm) | raw [raw_stride] | X [N][d]
//   output  psi <case> <N values>, clr <case> <N values> (hex floats)
#include <cstdio>
#include <vector>

#include "psi_point.hpp"

static bool read(std::FILE* f, std::vector<double>& v, size_t n) {
  v.assign(n, 0.0);
  for (size_t i = 0; i < n; ++i)
    if (std::fscanf(f, "%lf", &v[i]) != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
  std::FILE* in = std::fopen(argv[1], "r");
  int ncases = 0;
  if (!in || std::fscanf(in, "%d", &ncases) != 1) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  for (int c = 0; c < ncases; ++c) {
    gvi::FactorDev f{};
    int N = 0, narm = 0;
    std::vector<double> field, arm, raw, x;
    bool ok = std::fscanf(in, "%d %d %d %d %d", &f.kind, &f.d, &f.seg_J, &f.raw_stride, &N) == 5 && f.d >= 1 && N >= 0 && f.raw_stride >= 0 &&
              std::fscanf(in, "%d %d %d %lf %lf %lf %lf", &f.sdf_rows, &f.sdf_cols, &f.sdf_nz, &f.sdf_ox, &f.sdf_oy, &f.sdf_oz, &f.sdf_cell) == 7;
    ok = ok && read(in, field, (size_t)f.sdf_rows * f.sdf_cols * (f.sdf_nz > 0 ? f.sdf_nz : 1));
    ok = ok && std::fscanf(in, "%d", &narm) == 1 && narm >= 0 && read(in, arm, narm) && read(in, raw, f.raw_stride);
    if (!ok) { std::fprintf(stderr, "case %d: bad or short input\n", c); return 2; }
    f.K = 1;
    f.sdf_inv_cell = 1.0 / f.sdf_cell;
    f.sdf = field.empty() ? nullptr : field.data();
    f.arm = arm.empty() ? nullptr : arm.data();
    f.raw = raw.data();
    std::vector<double> psi(N), clr(N);
    for (int i = 0; i < N; ++i) {
      if (!read(in, x, f.d)) { std::fprintf(stderr, "case %d: short state %d\n", c, i); return 2; }
      double both_psi = 0.0, only_clr = 0.0;
      psi[i] = gvi::psi_point(f, 0, x.data());
      gvi::hinge_psi_clearance(f, 0, x.data(), true, true, both_psi, clr[i]);
      gvi::hinge_psi_clearance(f, 0, x.data(), false, true, both_psi, only_clr);
      // the two entry points and the two ways of asking are the same bits (NaN alike)
      const bool same_psi = both_psi == psi[i] || (both_psi != both_psi && psi[i] != psi[i]);
      const bool same_clr = only_clr == clr[i] || (only_clr != only_clr && clr[i] != clr[i]);
      if (!same_psi || !same_clr) { std::fprintf(stderr, "case %d state %d: psi_point and hinge_psi_clearance disagree\n", c, i); return 1; }
    }
    std::printf("psi %d", c);
    for (double v : psi) std::printf(" %a", v);
    std::printf("\nclr %d", c);
    for (double v : clr) std::printf(" %a", v);
    std::printf("\n");
  }
  std::fclose(in);
  std::printf("ALL OK\n");
  return 0;
}
