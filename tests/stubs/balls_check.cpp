// Stand-alone driver of the moving-ball kinds on the CPU for tests/test_balls_host.py (plain and -fsanitize=address,undefined
// builds): the rows of gaussianvi_amd/csrc/psi_kinds.hpp for GVI_PSI_HINGE_BALLS_2D / _3D and the arithmetic of
// gaussianvi_amd/csrc/balls_psi.hpp.  Reads one command per line from the file argv[1] and answers each with one line:
//   layout KIND D PPF             -> layout STATUS M J NEED | MESSAGE
//   params KIND D PPF K V...      -> params STATUS | MESSAGE      (psi_kind_layout first for J; the K blocks are the V)
//   flags KIND                    -> flags KIND NAME...           (the flags the table gives the kind)
//   numbers                       -> numbers BALLS_2D BALLS_3D BALLS_MAX_M SEG_MAX_J KIND_COUNT
//   eval P D J N V...             -> eval PSI_0 CLR_0 ... PSI_{N-1} CLR_{N-1}   (V: one block, then N states of D; %.17g)
// Blocks and states live in heap buffers of exactly their size, so a read past either is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../gaussianvi_amd/csrc/balls_psi.hpp"
#include "../../gaussianvi_amd/csrc/psi_kinds.hpp"

using namespace gvi;

template <unsigned FLAG>
static void name_flag(int kind, const char* name, std::string& out) {
  if (psi_kind_is<FLAG>(kind)) { out += ' '; out += name; }
}

static std::vector<double> values(std::istringstream& ls) {
  std::vector<double> v;
  for (std::string tok; ls >> tok;) v.push_back(std::strtod(tok.c_str(), nullptr));
  return v;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string cmd;
    ls >> cmd;
    if (cmd == "layout") {
      int kind = 0, d = 0, m = -1, J = -1;
      long long ppf = 0;
      int64_t need = -1;
      const char* msg = nullptr;
      ls >> kind >> d >> ppf;
      const gvi_status rc = psi_kind_layout(kind, d, ppf, &m, &J, &need, &msg);
      std::printf("layout %d %d %d %lld | %s\n", (int)rc, m, J, (long long)need, msg ? msg : "");
    } else if (cmd == "params") {
      int kind = 0, d = 0, m = 0, J = 0;
      long long ppf = 0, K = 0;
      int64_t need = 0;
      const char* msg = nullptr;
      ls >> kind >> d >> ppf >> K;
      const std::vector<double> v = values(ls);
      if (psi_kind_layout(kind, d, ppf, &m, &J, &need, &msg) != GVI_OK) { std::printf("params layout-refused | %s\n", msg); continue; }
      if ((long long)v.size() != K * ppf) { std::printf("params bad-command | %zu values\n", v.size()); continue; }
      double* blocks = new double[v.size()];
      for (size_t i = 0; i < v.size(); ++i) blocks[i] = v[i];
      const gvi_status rc = psi_kind_check_params(kind, d, J, ppf, K, blocks, &msg);
      std::printf("params %d | %s\n", (int)rc, msg ? msg : "");
      delete[] blocks;
    } else if (cmd == "flags") {
      int kind = 0;
      ls >> kind;
      std::string out;
      name_flag<PSI_RAW>(kind, "raw", out);
      name_flag<PSI_SDF_2D>(kind, "sdf2d", out);
      name_flag<PSI_SDF_3D>(kind, "sdf3d", out);
      name_flag<PSI_SDF>(kind, "sdf", out);
      name_flag<PSI_ARM>(kind, "arm", out);
      name_flag<PSI_CLEARANCE>(kind, "clearance", out);
      name_flag<PSI_CLOSED>(kind, "closed", out);
      name_flag<PSI_CLOSED_DEFAULT>(kind, "closed_default", out);
      name_flag<PSI_SUMSQ>(kind, "sumsq", out);
      name_flag<PSI_NO_DEVICE>(kind, "no_device", out);
      std::printf("flags %d%s\n", kind, out.c_str());
    } else if (cmd == "numbers") {
      std::printf("numbers %d %d %d %d %d\n", (int)GVI_PSI_HINGE_BALLS_2D, (int)GVI_PSI_HINGE_BALLS_3D, (int)GVI_BALLS_MAX_M, (int)GVI_SEG_MAX_J,
                  (int)KIND_COUNT);
    } else if (cmd == "eval") {
      int P = 0, d = 0, J = 0, N = 0;
      ls >> P >> d >> J >> N;
      const std::vector<double> v = values(ls);
      const size_t nb = 3 + (size_t)J * balls_point_stride(P, d) + (size_t)BALLS_SLOTS * balls_slot_stride(P);
      if ((P != 2 && P != 3) || v.size() != nb + (size_t)N * d) { std::printf("eval bad-command | %zu values\n", v.size()); continue; }
      double* block = new double[nb];
      for (size_t i = 0; i < nb; ++i) block[i] = v[i];
      std::printf("eval");
      for (int i = 0; i < N; ++i) {
        double* x = new double[d];
        for (int c = 0; c < d; ++c) x[c] = v[nb + (size_t)i * d + c];
        const double psi = P == 2 ? psi_hinge_balls<2>(block, x, d, J) : psi_hinge_balls<3>(block, x, d, J);
        const double clr = P == 2 ? balls_clearance<2>(block, x, d, J) : balls_clearance<3>(block, x, d, J);
        std::printf(" %.17g %.17g", psi, clr);
        delete[] x;
      }
      std::printf("\n");
      delete[] block;
    } else if (!cmd.empty()) {
      std::printf("unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
