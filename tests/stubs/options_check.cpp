// Stand-alone driver of gaussianvi_amd/csrc/options.hpp for tests/test_options_host.py (plain and -fsanitize=address,undefined
// builds).  Reads one command per line from the file argv[1]; every command starts from fresh defaults and answers with one line:
//   rows                 -> rows NAME:ENV ...              ("-" where a row has none)
//   defaults             -> ok | FIELD=VALUE ...
//   env NAME VALUE       -> ok | FIELD=VALUE ...           (options_from_env with a lookup that knows NAME alone)
//   set NAME VALUE       -> ok | FIELD=VALUE ...   or   refused MESSAGE
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "../../gaussianvi_amd/csrc/options.hpp"

using namespace gvi;

static void dump(const Options& o) {
  std::printf("ok | warm_start=%d fuse_trial=%d target_waves=%d mirror=%d split_flush=%d sreg_pipe=%d no_scost=%d orbit=%d fused=%d "
              "orbit_waves=%d jacobi_tol=%a chol_sqrt=%d chol_rowb=%d trust_table_degree=%d orbit_min_tiles=%d orbit_copies=%d "
              "pair_fuse=%d fuse_gather=%d side_solve=%d asm_on_load=%d chain_merge=%d chain_merge_fault=%d pipeline=%d spin_ms=%d "
              "safe_publish=%d sample_sweep=%d solve_lds=%d chain_wave=%d asm_dense=%d chain_pair=%d\n",
              o.warm_start, o.fuse_trial, o.target_waves, o.mirror, o.split_flush, o.sreg_pipe, o.no_scost, o.orbit, o.fused,
              o.orbit_waves, o.jacobi_tol, o.chol_sqrt, o.chol_rowb, o.trust_table_degree, o.orbit_min_tiles, o.orbit_copies,
              o.pair_fuse, o.fuse_gather, o.side_solve, o.asm_on_load, o.chain_merge, o.chain_merge_fault, o.pipeline, o.spin_ms,
              o.safe_publish, o.sample_sweep, o.solve_lds, o.chain_wave, o.asm_dense, o.chain_pair);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string cmd, name, value;
    ls >> cmd >> name >> value;
    Options o;
    if (cmd == "rows") {
      std::printf("rows");
      for (const OptionRow& r : OPTION_ROWS) std::printf(" %s:%s", r.name ? r.name : "-", r.env ? r.env : "-");
      std::printf("\n");
    } else if (cmd == "defaults") {
      dump(o);
    } else if (cmd == "env") {
      options_from_env(o, [&](const char* asked) -> const char* { return name == asked ? value.c_str() : nullptr; });
      dump(o);
    } else if (cmd == "set") {
      std::string msg;
      if (option_set(o, name.c_str(), std::atoi(value.c_str()), &msg)) dump(o);
      else std::printf("refused %s\n", msg.c_str());
    } else if (!cmd.empty()) {
      std::printf("unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
