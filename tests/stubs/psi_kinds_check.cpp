// Stand-alone driver of gaussianvi_amd/csrc/psi_kinds.hpp for tests/test_psi_kinds_host.py (plain and -fsanitize=address,undefined
// builds).  Reads one command per line from the file argv[1] and answers each with one line:
//   layout KIND D PPF             -> layout STATUS M J NEED | MESSAGE
//   params KIND D PPF K V...      -> params STATUS | MESSAGE      (psi_kind_layout first for J; the K blocks are the V, "null" = no pointer)
//   flags KIND                    -> flags KIND NAME...           (the flags the table gives the kind)
// The parameter blocks live in a heap buffer of exactly K * PPF doubles, so a read past a block is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../gaussianvi_amd/csrc/psi_kinds.hpp"

using namespace gvi;

template <unsigned FLAG>
static void name_flag(int kind, const char* name, std::string& out) {
  if (psi_kind_is<FLAG>(kind)) { out += ' '; out += name; }
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
      std::vector<double> v;
      bool null = false;
      for (std::string tok; ls >> tok;) {
        if (tok == "null") null = true; else v.push_back(std::strtod(tok.c_str(), nullptr));
      }
      if (psi_kind_layout(kind, d, ppf, &m, &J, &need, &msg) != GVI_OK) { std::printf("params layout-refused | %s\n", msg); continue; }
      if (!null && (long long)v.size() != K * ppf) { std::printf("params bad-command | %zu values\n", v.size()); continue; }
      double* blocks = null ? nullptr : new double[v.size()];
      for (size_t i = 0; i < v.size() && blocks; ++i) blocks[i] = v[i];
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
    } else if (!cmd.empty()) {
      std::printf("unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
