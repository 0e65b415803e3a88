// Stand-alone driver of gaussianvi_amd/csrc/factor_lds.hpp for tests/test_factor_lds_host.py (plain and
// -fsanitize=address,undefined builds).  Reads one command per line from the file argv[1] and answers each with one line of
// NAME=VALUE pairs (offsets and sizes in doubles unless the name ends in _bytes):
//   products D        -> the Jacobi view, the Cholesky view (chol_end at m = D), the area, the staging, both host sizes
//   chol D M          -> chol_end of the Cholesky view for M rows of A
//   epilogue D        -> the epilogue view, its `last` word, the tree and the size of epilogue_all_kernel at dmax = D
//   item D            -> the item area of the one-launch passes
//   helper D M        -> the helper wave's view
//   fused DMAX WALK KEEP ITEMS -> region = fused_region_of(WALK, DMAX) and the launch 4 region + ITEMS (KEEP + 4 npairs(DMAX)),
//                        as kernels_fused.hpp composes them (WALK = orbit_lds_doubles, KEEP = fused_keep_doubles: kernels_orbit.hpp
//                        and kernels_fused.hpp are HIP headers, their two values come from the caller)
//   generic D M       -> the generic kernel's view, its bytes, and whether the launch is refused
//   jko D             -> jko_half_kernel's view and bytes
//   fixed D           -> box (doubles, refused), half-space (doubles per wave), split (doubles), block3 (doubles per wave)
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "../../gaussianvi_amd/csrc/factor_lds.hpp"

using namespace gvi;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string cmd;
    ls >> cmd;
    int d = 0, m = 0;
    if (cmd == "products") {
      ls >> d;
      const ProductsLds L{d};
      std::printf("A0=%d A1=%d V0=%d V1=%d al=%d be=%d lam=%d pa=%d jacobi_end=%d Ll=%d Xl=%d Al=%d chol_end=%d doubles=%d Sl=%d ml=%d staged_end=%d "
                  "prep_bytes=%zu prep_all_bytes=%zu\n",
                  L.A0(), L.A1(), L.V0(), L.V1(), L.al(), L.be(), L.lam(), L.pa(), L.jacobi_end(), L.Ll(), L.Xl(), L.Al(), L.chol_end(d), L.doubles(),
                  L.Sl(), L.ml(), L.staged_end(), prep_lds_bytes(d), prep_all_lds_bytes(d));
    } else if (cmd == "chol") {
      ls >> d >> m;
      std::printf("chol_end=%d\n", ProductsLds{d}.chol_end(m));
    } else if (cmd == "epilogue") {
      ls >> d;
      const EpilogueLds E{d};
      std::printf("Ms=%d M2=%d Tm=%d Sv=%d Lv=%d end=%d last=%zu doubles=%zu tree=%zu all_doubles=%zu\n", E.Ms(), E.M2(), E.Tm(), E.Sv(), E.Lv(), E.end(),
                  E.last(), epilogue_lds_doubles(d), epilogue_all_tree(d), epilogue_all_lds_doubles(d));
    } else if (cmd == "item") {
      ls >> d;
      std::printf("item=%zu products=%zu\n", item_lds_doubles(d), item_products_doubles(d));
    } else if (cmd == "helper") {
      ls >> d >> m;
      const HelperLds H{d, m};
      std::printf("Al=%zu mh=%zu end=%zu\n", H.Al(), H.mh(), H.end());
    } else if (cmd == "fused") {
      int dmax = 0, items = 0;
      size_t walk = 0, keep = 0;
      ls >> dmax >> walk >> keep >> items;
      const size_t region = fused_region_of(walk, dmax);
      std::printf("region=%zu lds=%zu\n", region, 4 * region + (size_t)items * (keep + 4 * (size_t)npairs(dmax)));
    } else if (cmd == "generic") {
      ls >> d >> m;
      const GenericLds G{d, m};
      std::printf("zs=%d xs=%d cs=%d Ssh=%d mush=%d Ash=%d bsh=%d gsh=%d end=%d bytes=%zu refused=%d\n", G.zs(), G.xs(), G.cs(), G.Ssh(), G.mush(), G.Ash(),
                  G.bsh(), G.gsh(), G.end(), generic_lds_bytes(d, m), (int)(generic_lds_bytes(d, m) > GENERIC_LDS_LIMIT));
    } else if (cmd == "jko") {
      ls >> d;
      const JkoLds K{d};
      std::printf("M=%d Sg=%d Tm=%d end=%d bytes=%zu\n", K.M(), K.Sg(), K.Tm(), K.end(), jko_half_lds_bytes(d));
    } else if (cmd == "fixed") {
      ls >> d;
      std::printf("box=%zu box_refused=%d halfspace=%zu split=%d block3=%zu\n", box_closed_lds_doubles(d), (int)(box_closed_lds_doubles(d) * 8 > BOX_CLOSED_LDS_LIMIT),
                  halfspace_closed_lds_doubles(d), SPLIT_LDS_DOUBLES(d), block3_lds_doubles());
    } else if (!cmd.empty()) {
      std::printf("unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
