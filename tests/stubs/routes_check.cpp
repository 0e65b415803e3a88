// Stand-alone driver of gaussianvi_amd/csrc/routes.hpp for tests/test_routes_host.py (plain and -fsanitize=address,undefined
// builds).  Reads one command per line from the file argv[1] and answers each with one line:
//   reg KIND D M | sreg KIND D M | scost KIND D M | split D M | orbit M SMAX | opsi KIND | fused M SMAX D0 D1 | closed KIND
//   | prep D
//                                  -> NAME 0, or NAME 1 and the template arguments of the instance the list hands out
//   variant V                      -> variant 0, or variant 1 and what the predicates say of the force: reg must_reg sgpr orbit opsi
//   route KEY=VALUE...             -> route STATUS ROUTE NCHUNK CHUNK MCHUNK GX GY PIPE | REFUSAL
//   fuse KEY=VALUE... ; SET ; SET  -> fuse NAME       (moments / cost launch; every SET is the KEY=VALUE facts of one set)
//   full KEY=VALUE... ; SET ; SET  -> full NAME       (full pass; per set also resident=0|1)
//   geo ROUTE FUSED CLOSED         -> geo CODE
// Keys of the facts and rules: see facts_of / rules_of below; a key that is not given keeps the default of the struct.
#include <cstdio>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../gaussianvi_amd/csrc/routes.hpp"

using namespace gvi;
using KV = std::map<std::string, long long>;

template <class T> struct PsiName;
template <> struct PsiName<PsiRange1D> { static std::string get() { return "range"; } };
template <int D, int M> struct PsiName<PsiQuad<D, M>> { static std::string get() { return "quad " + std::to_string(D) + " " + std::to_string(M); } };
template <int D, int KIND> struct PsiName<PsiHingeSdf<D, KIND>> { static std::string get() { return "sdf " + std::to_string(D) + " " + std::to_string(KIND); } };
template <int D, int P> struct PsiName<PsiHingeSeg<D, P>> { static std::string get() { return "seg " + std::to_string(D) + " " + std::to_string(P); } };
template <int D> struct PsiName<PsiBoxHinge<D>> { static std::string get() { return "box " + std::to_string(D); } };

template <int D, class Psi> std::string describe(RegInst<D, Psi>) { return std::to_string(D) + " " + PsiName<Psi>::get(); }
template <int D, int M, bool PIPE> std::string describe(SregInst<D, M, PIPE> t) { return std::to_string(D) + " " + std::to_string(M) + " " + std::to_string((int)t.pipe); }
template <int D, int M> std::string describe(ScostInst<D, M>) { return std::to_string(D) + " " + std::to_string(M); }
template <int D, int R> std::string describe(SplitInst<D, R>) { return std::to_string(D) + " " + std::to_string(R); }
template <int M, int SMAX, int WAVES, bool PAIR> std::string describe(OrbitInst<M, SMAX, WAVES, PAIR> t) {
  return std::to_string(M) + " " + std::to_string(SMAX) + " " + std::to_string(t.waves) + " " + std::to_string((int)t.pair);
}
template <int KIND> std::string describe(OrbitPsiInst<KIND>) { return std::to_string(KIND); }
template <int M, int SMAX, int WAVES, int D0, int D1> std::string describe(FusedInst<M, SMAX, WAVES, D0, D1>) {
  return std::to_string(M) + " " + std::to_string(SMAX) + " " + std::to_string(WAVES) + " " + std::to_string(D0) + " " + std::to_string(D1);
}
inline std::string describe(ClosedSumsq) { return "sumsq"; }
inline std::string describe(ClosedBox) { return "box"; }
inline std::string describe(ClosedHalfspace) { return "halfspace"; }
template <int EPLP> std::string describe(PrepInst<EPLP>) { return std::to_string(EPLP); }

static const char* ROUTE_NAMES[] = {"Empty", "Closed", "Orbit", "OrbitPsi", "Split", "Sreg", "Scost", "Reg", "Generic"};

static KV parse(const std::string& text) {
  KV kv;
  std::istringstream ls(text);
  for (std::string tok; ls >> tok;) {
    const size_t eq = tok.find('=');
    if (eq != std::string::npos) kv[tok.substr(0, eq)] = std::stoll(tok.substr(eq + 1));
  }
  return kv;
}
template <class T> void take(const KV& kv, const char* key, T& field) {
  auto it = kv.find(key);
  if (it != kv.end()) field = (T)it->second;
}
static RouteFacts facts_of(const KV& kv) {
  RouteFacts f;
  take(kv, "kind", f.kind); take(kv, "d", f.d); take(kv, "m", f.m); take(kv, "K", f.K);
  take(kv, "closed", f.closed_form); take(kv, "all_pos", f.all_pos); take(kv, "psi_ext", f.psi_ext);
  take(kv, "arm", f.has_arm); take(kv, "sdf", f.has_sdf); take(kv, "ndof", f.arm_ndof); take(kv, "J", f.seg_J);
  take(kv, "rows", f.opsi_rows);
  take(kv, "Np", f.Np); take(kv, "Nmp", f.Nmp); take(kv, "p", f.p); take(kv, "coded", f.coded); take(kv, "Zq", f.has_Zq);
  take(kv, "orb", f.orb_ok); take(kv, "smax", f.orb_smax); take(kv, "tiles", f.orb_tiles);
  return f;
}
static bool rules_of(const KV& kv, RouteRules* out) {
  RouteRules r;
  int variant = 0;
  take(kv, "variant", variant);
  if (!route_force_of_variant(variant, &r.force)) return false;
  take(kv, "orbit", r.orbit); take(kv, "no_scost", r.no_scost); take(kv, "sreg_pipe", r.sreg_pipe);
  take(kv, "tw", r.target_waves); take(kv, "ow", r.orbit_waves); take(kv, "omt", r.orbit_min_tiles);
  take(kv, "pair_fuse", r.pair_fuse); take(kv, "fused", r.fused); take(kv, "chol_sqrt", r.chol_sqrt);
  *out = r;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string cmd;
    ls >> cmd;
    int a = 0, b = 0, c = 0, d = 0;
    std::string got;
    auto say = [&](auto inst) { got = describe(inst); };
    auto answer = [&](bool hit) { std::printf("%s %d%s%s\n", cmd.c_str(), (int)hit, hit ? " " : "", got.c_str()); };
    if (cmd == "reg") { ls >> a >> b >> c; answer(with_reg_instance(a, b, c, say)); }
    else if (cmd == "sreg") { ls >> a >> b >> c; answer(with_sreg_instance(a, b, c, say)); }
    else if (cmd == "scost") { ls >> a >> b >> c; answer(with_scost_instance(a, b, c, say)); }
    else if (cmd == "split") { ls >> a >> b; answer(with_split_instance(a, b, say)); }
    else if (cmd == "orbit") { ls >> a >> b; answer(with_orbit_instance(a, b, say)); }
    else if (cmd == "opsi") { ls >> a; answer(with_orbit_psi_instance(a, say)); }
    else if (cmd == "fused") { ls >> a >> b >> c >> d; answer(with_fused_instance(a, b, c, d, say)); }
    else if (cmd == "closed") { ls >> a; answer(with_closed_instance(a, say)); }
    else if (cmd == "prep") { ls >> a; answer(with_prep_instance(a, say)); }
    else if (cmd == "variant") {
      ls >> a;
      RouteForce f;
      if (!route_force_of_variant(a, &f)) { std::printf("variant 0\n"); continue; }
      std::printf("variant 1 %d %d %d %d %d\n", (int)may_take_reg(f), (int)must_take_reg(f), (int)may_take_sgpr(f), (int)may_take_orbit(f),
                  (int)prefers_orbit_psi(f));
    } else if (cmd == "route") {
      const KV kv = parse(line);
      RouteRules r;
      if (!rules_of(kv, &r)) { std::printf("route bad-variant\n"); continue; }
      int full = 1;
      take(kv, "full", full);
      const RouteDecision o = decide_route(facts_of(kv), r, full);
      std::printf("route %d %s %d %lld %lld %u %u %d | %s\n", (int)o.status, ROUTE_NAMES[(int)o.route], o.nchunk, (long long)o.chunk,
                  (long long)o.mchunk, o.gx, o.gy, (int)o.pipe, o.why ? o.why : "");
    } else if (cmd == "fuse" || cmd == "full") {
      std::vector<std::string> parts;
      std::istringstream ps(line);
      for (std::string part; std::getline(ps, part, ';');) parts.push_back(part);
      const KV head = parse(parts[0]);
      RouteRules r;
      if (!rules_of(head, &r)) { std::printf("%s bad-variant\n", cmd.c_str()); continue; }
      int full = 1, profile_all = 0, ngd = 1, max_items = 4;
      take(head, "full", full); take(head, "profile_all", profile_all); take(head, "ngd", ngd); take(head, "max_items", max_items);
      const int ns = (int)parts.size() - 1;
      // heap arrays of exactly ns entries: a read past the sets is the sanitizer's to report
      RouteFacts* F = new RouteFacts[ns];
      RouteDecision* D = new RouteDecision[ns];
      bool* resident = new bool[ns];
      bool refused = false;
      for (int i = 0; i < ns; ++i) {
        const KV kv = parse(parts[i + 1]);
        F[i] = facts_of(kv);
        D[i] = decide_route(F[i], r, cmd == "full" ? 1 : full);
        refused = refused || D[i].status != GVI_OK;
        resident[i] = false;
        take(kv, "resident", resident[i]);
      }
      if (refused) std::printf("%s refused\n", cmd.c_str());
      else if (cmd == "fuse") {
        static const char* names[] = {"None", "OrbitPair", "SregPair", "ScostPair", "Planar3"};
        std::printf("fuse %s\n", names[(int)decide_fuse(ns, F, D, r, profile_all != 0, full)]);
      } else {
        static const char* names[] = {"Fused", "Block3", "Separate"};
        std::printf("full %s\n", names[(int)decide_full(ns, F, D, resident, r, profile_all != 0, ngd != 0, max_items)]);
      }
      delete[] F;
      delete[] D;
      delete[] resident;
    } else if (cmd == "geo") {
      ls >> a >> b >> c;
      std::printf("geo %d\n", geometry_code((Route)a, b != 0, c != 0));
    } else if (!cmd.empty()) {
      std::printf("unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
