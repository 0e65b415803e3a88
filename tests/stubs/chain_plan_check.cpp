// Stand-alone driver of gaussianvi_amd/csrc/chain_plan.hpp for tests/test_chain_plan_host.py (plain and
// -fsanitize=address,undefined builds).  Reads one command per line from the file argv[1] and answers each with one line:
//   shape T n                       -> shape PADDED SUPPORTED LEVELS THREADS LP_ENTRIES WS_DOUBLES     (threads, workspace: at PADDED)
//   fwd HAS_E HAS_Y TOP N S ROWB    -> fwd DOUBLES
//   bwd HAS_E N S                   -> bwd DOUBLES
//   dense N ; K D NSP DATA ; ...    -> dense 0|1                  (chain_asm_dense on the sets that follow, one per ';')
//   plan KEY=VALUE...               -> plan STATUS ASSEMBLE THREADS NPASS | LAUNCH | LAUNCH ...
//        LAUNCH = KERNEL FORM nb0 nb nbt nb0c lds : level0 m S top first par lp_off blocks [: the same of the carried pass]
// Keys of plan: T n on0 back0 on1 list shape (facts), wave asm_dense pair merge (rules); a key that is not given keeps the
// default of the struct (facts: off).
#include <cstdio>
#include <fstream>
#include <map>
#include <sstream>
#include <string>

#include "../../gaussianvi_amd/csrc/chain_plan.hpp"

using namespace gvi;

static const char* KERNELS[] = {"Wave", "Forward", "TopBack", "Backward"};
static const char* FORMS[] = {"Own", "TwoRow", "Readlane"};
static const char* ASMS[] = {"Off", "Generic", "Dense"};
static const char* STATUS[] = {"Ok", "BlockSize", "Lds"};

static void print_pass(const ChainPass& q) {
  std::printf(" : %d %d %d %d %d %d %d %d", q.level0, q.m, q.S, q.top, q.first, q.par, q.lp_off, q.blocks);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string cmd;
    ls >> cmd;
    if (cmd == "shape") {
      int T = 0, n = 0;
      ls >> T >> n;
      const int N = chain_padded(n);
      std::printf("shape %d %d %d %d %zu %zu\n", N, (int)chain_supported(n), chain_levels(T), N ? chain_threads(N) : 0, chain_lp_entries(T),
                  chain_ws_doubles(T, N));
    } else if (cmd == "fwd") {
      int e = 0, y = 0, top = 0, N = 0, S = 0, rowb = 0;
      ls >> e >> y >> top >> N >> S >> rowb;
      std::printf("fwd %zu\n", chain::fwd_lds_doubles(e != 0, y != 0, top != 0, N, S, rowb != 0));
    } else if (cmd == "bwd") {
      int e = 0, N = 0, S = 0;
      ls >> e >> N >> S;
      std::printf("bwd %zu\n", chain::bwd_lds_doubles(e != 0, N, S));
    } else if (cmd == "dense") {
      int n = 0, nsets = 0;
      ls >> n;
      AsmSetFacts sets[8] = {};
      for (std::string sep; nsets < 8 && ls >> sep;) {
        int data = 0;
        ls >> sets[nsets].K >> sets[nsets].d >> sets[nsets].nsp >> data;
        sets[nsets++].data = data != 0;
      }
      std::printf("dense %d\n", (int)chain_asm_dense(sets, nsets, n));
    } else if (cmd == "plan") {
      std::map<std::string, long long> kv;
      for (std::string tok; ls >> tok;) {
        const size_t eq = tok.find('=');
        if (eq != std::string::npos) kv[tok.substr(0, eq)] = std::stoll(tok.substr(eq + 1));
      }
      auto get = [&](const char* key, long long def) { return kv.count(key) ? kv[key] : def; };
      ChainFacts f{};
      ChainRules r;
      f.T = (int)get("T", 0); f.n = (int)get("n", 0);
      f.on0 = get("on0", 0); f.back0 = get("back0", 0); f.on1 = get("on1", 0);
      f.asm_list = get("list", 0); f.asm_dense_shape = get("shape", 0);
      r.wave = get("wave", r.wave); r.asm_dense = get("asm_dense", r.asm_dense); r.pair = get("pair", r.pair); r.merge = get("merge", r.merge);
      const ChainLaunchPlan p = chain_decide(f, r);
      std::printf("plan %s %s %d %d", STATUS[(int)p.status], ASMS[(int)p.assemble], p.threads, p.npass);
      for (int i = 0; i < p.nlaunch; ++i) {
        const ChainLaunch& l = p.launch[i];
        std::printf(" | %s %s %d %d %d %d %u", KERNELS[(int)l.kernel], FORMS[(int)l.form], l.nb0, l.nb, l.nbt, l.nb0c, l.lds);
        if (l.kernel != ChainKernel::Wave) print_pass(p.pass[l.pass]);
        if (l.carried >= 0) print_pass(p.pass[l.carried]);
      }
      std::printf("\n");
    } else if (!cmd.empty()) {
      std::printf("unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
