// Host restatement of the walk's priority bands (gaussianvi_amd/csrc/walk_prio.hpp, orbits.hpp::walk_prio_costs) and the
// option row that switches them (options.hpp), for tests/test_walk_prio_host.py (plain and sanitized builds).
// usage: walk_prio_check table file d N   -- file: N x d doubles Z (row-major) followed by N doubles w, little endian.
//          Per chunk w of the four-chunk split: "chunk w total T tiles n costs c ... prio p ...": the chunk's total, the cost
//          of each of its tiles and the priority the wave takes in front of every tile and behind the last one, as
//          orbit_wave forms it (remaining cost against the cuts of the total); then "ok d N smax".
//        walk_prio_check option           -- "default v", then the field under GVI_WALK_PRIO = 0 / 1 (injected look-up) and
//          under option_set("walk_prio", 0 / 1), then an unknown name's refusal
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../gaussianvi_amd/csrc/options.hpp"
#include "../../gaussianvi_amd/csrc/orbits.hpp"

using namespace gvi;

static int table(int argc, char** argv) {
  if (argc != 5) { std::printf("FAIL usage\n"); return 1; }
  const int d = std::atoi(argv[3]);
  const long long N = std::atoll(argv[4]);
  if (d < 1 || N < 1) { std::printf("FAIL arguments\n"); return 1; }
  std::vector<double> Z((size_t)N * d), w((size_t)N);
  std::FILE* f = std::fopen(argv[2], "rb");
  if (!f) { std::printf("FAIL open\n"); return 1; }
  const bool read = std::fread(Z.data(), 8, Z.size(), f) == Z.size() && std::fread(w.data(), 8, w.size(), f) == w.size();
  std::fclose(f);
  if (!read) { std::printf("FAIL read\n"); return 1; }
  const OrbitHost o = build_orbits(d, N, Z.data(), w.data(), true);
  if (!o.ok) { std::printf("FAIL build_orbits\n"); return 1; }
  const std::vector<int32_t> b = orbit_chunk_bounds(o, 4);
  if (b.size() != 5) { std::printf("FAIL bounds\n"); return 1; }
  const WalkPrioSet p = walk_prio_costs(o, b);
  for (int c = 0; c < 4; ++c) {
    const WalkPrioCuts cut = walk_prio_cuts(p.total[c]);
    std::printf("chunk %d total %d tiles %d costs", c, p.total[c], b[(size_t)c + 1] - b[(size_t)c]);
    for (int t = b[(size_t)c]; t < b[(size_t)c + 1]; ++t) {
      const int cost = p.tile[o.tile_s[(size_t)t]];
      if (cost != (int)orbit_tile_cost(o.tile_s[(size_t)t], o.tile_g[(size_t)t])) { std::printf("\nFAIL tile cost\n"); return 1; }
      std::printf(" %d", cost);
    }
    std::printf(" prio");
    int rem = p.total[c];
    for (int t = b[(size_t)c]; t < b[(size_t)c + 1]; ++t) {
      std::printf(" %d", walk_prio_band(rem, cut));
      rem -= p.tile[o.tile_s[(size_t)t]];
    }
    std::printf(" %d\n", walk_prio_band(rem, cut));
  }
  std::printf("ok %d %lld %d\n", d, N, o.smax);
  return 0;
}

static int option() {
  Options o;
  std::printf("default %d\n", (int)o.walk_prio);
  for (int v = 0; v < 2; ++v) {
    Options e;
    const std::string value = std::to_string(v);
    options_from_env(e, [&](const char* asked) -> const char* { return std::strcmp(asked, "GVI_WALK_PRIO") == 0 ? value.c_str() : nullptr; });
    std::printf("env %d %d\n", v, (int)e.walk_prio);
    Options s;
    std::string msg;
    if (!option_set(s, "walk_prio", v, &msg)) { std::printf("FAIL %s\n", msg.c_str()); return 1; }
    std::printf("set %d %d\n", v, (int)s.walk_prio);
  }
  Options u;
  std::string msg;
  const bool known = option_set(u, "walk_priority", 1, &msg);
  std::printf("unknown %d %s\n", (int)known, msg.c_str());
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::strcmp(argv[1], "table") == 0) return table(argc, argv);
  if (argc == 2 && std::strcmp(argv[1], "option") == 0) return option();
  std::printf("FAIL usage\n");
  return 1;
}
