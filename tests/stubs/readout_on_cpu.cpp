// gaussianvi_amd/csrc/readout_moments.hpp -- the functions moments_readout_kernel calls -- compiled for the CPU and run on the cases
// of a file.  Built plain and with AddressSanitizer / UBSan by tests/test_readout_host.py, which writes the cases and compares the
// printed values with tests/readout_ref.py.  Every buffer is a std::vector of exactly the size the functions may touch, so a read or
// write past a parameter block, a root or a Gam_j is reported.
//   input   <ncases>, then per case one of
//     mom <P> <cls> <d> <J> <order> | cls 0 (LEAD, J = 1) and 1 (SEG): <rows> <cols> <nz> <ox> <oy> <oz> <cell> | field [rows cols
//                               max(nz, 1)] (r + c rows + z rows cols) | p: the factor's block, [3] (LEAD), [3 + J P (d + 1)] (SEG) or
//                               [3 + J (P (d + 1) + 1) + 8 (2 P + 1)] (cls 2, BALLS) | mu [d] | S [d d] (row-major root, x = mu + S z) |
//                               nodes [order] | weights [order]
//     chol <P> | C [P P]
//   mom <case> <ok> <m0> <m1 [d]> <M2 [d d]>      E[psi], E[z psi], E[z z^T psi] assembled in ascending j (hex floats)
//   chol <case> <ok> <keep [P]> <L [P P]>         readout_chol
#include <cstdio>
#include <cstring>
#include <vector>

#include "psi_point.hpp"
#include "readout_moments.hpp"

static bool read(std::FILE* f, std::vector<double>& v, size_t n) {
  v.assign(n, 0.0);
  for (size_t i = 0; i < n; ++i)
    if (std::fscanf(f, "%lf", &v[i]) != 1) return false;
  return true;
}

template <int P>
static bool run_chol(std::FILE* f, int c) {
  std::vector<double> C;
  if (!read(f, C, P * P)) return false;
  const gvi::ReadoutChol<P> ch = gvi::readout_chol<P>(C.data());
  std::printf("chol %d %d", c, ch.ok ? 1 : 0);
  for (int k = 0; k < P; ++k) std::printf(" %d", ch.keep[k] ? 1 : 0);
  for (int e = 0; e < P * P; ++e) std::printf(" %a", ch.L[e]);
  std::printf("\n");
  return true;
}

template <int P>
static bool run_mom(std::FILE* f, int c, int cls, int d, int J, int order) {
  gvi::FactorDev fd{};
  std::vector<double> field, p, mu, S, nodes, weights;
  if (cls != gvi::READOUT_BALLS) {
    if (std::fscanf(f, "%d %d %d %lf %lf %lf %lf", &fd.sdf_rows, &fd.sdf_cols, &fd.sdf_nz, &fd.sdf_ox, &fd.sdf_oy, &fd.sdf_oz, &fd.sdf_cell) != 7 ||
        !read(f, field, (size_t)fd.sdf_rows * fd.sdf_cols * (fd.sdf_nz > 0 ? fd.sdf_nz : 1)))
      return false;
    fd.sdf = field.data();
    fd.sdf_inv_cell = 1.0 / fd.sdf_cell;
  }
  const size_t np = 3 + (size_t)J * (cls == gvi::READOUT_LEAD ? 0 : gvi::readout_stride(cls, P, d)) +
                    (cls == gvi::READOUT_BALLS ? gvi::BALLS_SLOTS * gvi::balls_slot_stride(P) : 0);
  if (!read(f, p, np) || !read(f, mu, d) || !read(f, S, (size_t)d * d) || !read(f, nodes, order) || !read(f, weights, order)) return false;
  const gvi::ReadoutView view{p.data(), P, d, J, cls};
  std::vector<double> Gam((size_t)P * d), m1(d, 0.0), M2((size_t)d * d, 0.0);
  double m0 = 0.0;
  bool ok = true;
  for (int j = 0; j < J && ok; ++j) {
    gvi::ReadoutSums<P> s;
    // f_j at a read-out point: the hinge on the balls' distance, or on the grid's as moments_readout_kernel forms it
    auto fj = [&](const double* q) {
      if (cls == gvi::READOUT_BALLS) return gvi::readout_f_balls<P>(p.data(), view.balls(), view.tau(j), q);
      const double sd = P == 2 ? gvi::sdf2d_lookup(fd, q[0], q[1]) : gvi::sdf3d_lookup(fd, q[0], q[1], q[P - 1]);
      return gvi::hinge_sq(sd, p[1] + p[2], 1.0, p[0]);
    };
    ok = gvi::readout_check_point<P>(d, view.W(j), view.c(j), mu.data(), S.data(), order, nodes.data(), weights.data(), fj, Gam.data(), &s);
    if (!ok) break;
    double Hs[P * P];
    int e = 0;
    for (int k = 0; k < P; ++k)
      for (int l = k; l < P; ++l, ++e) Hs[k * P + l] = Hs[l * P + k] = s.H[e];
    m0 += s.e0;
    for (int a = 0; a < d; ++a) {
      for (int k = 0; k < P; ++k) m1[a] += Gam[(size_t)k * d + a] * s.h[k];
      for (int b = 0; b < d; ++b)
        for (int k = 0; k < P; ++k)
          for (int l = 0; l < P; ++l) M2[(size_t)a * d + b] += Gam[(size_t)k * d + a] * Hs[k * P + l] * Gam[(size_t)l * d + b];
    }
  }
  for (int a = 0; a < d; ++a) M2[(size_t)a * d + a] += m0;
  std::printf("mom %d %d %a", c, ok ? 1 : 0, m0);
  for (double t : m1) std::printf(" %a", t);
  for (double t : M2) std::printf(" %a", t);
  std::printf("\n");
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "r");
  int ncases = 0;
  if (!f || std::fscanf(f, "%d", &ncases) != 1) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  for (int c = 0; c < ncases; ++c) {
    char what[8] = {0};
    int P = 0, cls = 0, d = 0, J = 0, order = 0;
    bool ok = std::fscanf(f, "%7s %d", what, &P) == 2 && (P == 2 || P == 3);
    if (ok && !std::strcmp(what, "chol")) {
      ok = P == 2 ? run_chol<2>(f, c) : run_chol<3>(f, c);
    } else if (ok && !std::strcmp(what, "mom")) {
      ok = std::fscanf(f, "%d %d %d %d", &cls, &d, &J, &order) == 4 && cls >= gvi::READOUT_LEAD && cls <= gvi::READOUT_BALLS && d >= P && J >= 1 &&
           (cls != gvi::READOUT_LEAD || J == 1) && gvi::readout_order_ok(order, P);
      if (ok) ok = P == 2 ? run_mom<2>(f, c, cls, d, J, order) : run_mom<3>(f, c, cls, d, J, order);
    } else {
      ok = false;
    }
    if (!ok) { std::fprintf(stderr, "case %d: bad or short input\n", c); return 2; }
  }
  std::fclose(f);
  std::printf("ALL OK\n");
  return 0;
}
