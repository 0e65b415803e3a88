// The lane records of the chain eliminations (gaussianvi_amd/csrc/chain_lane_record.hpp) against the expressions eliminate
// used before the record existed, restated below: for every lane 0 .. 63 of the two layouts (factorisation, solve; N = 6), the roles, the column
// inside the group, and -- on a stand-in for the pass's LDS with arbitrary contents -- the column a lane loads, the places its
// factor column is stored to and the accumulators it adds to.
// Build: g++ -std=c++17 -I gaussianvi_amd/csrc tests/stubs/chain_lane_record_check.cpp        (prints "ok <checks>", exit 0)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "chain_lane_record.hpp"

using namespace gvi::chain;

static long checks = 0;
static int failures = 0;
#define CHECK(c, ...) do { ++checks; if (!(c)) { if (++failures < 20) { std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

struct Roles { bool isD, isE, isA, isB, isY; int cc; };

// ---- the expressions of eliminate (two-row layout, one node per wave), as they were ----
template <bool HAS_E, bool HAS_Y, int N>
static Roles old_roles(const int lane) {
  Roles o;
  constexpr int G0 = 16 - 2 * N;
  constexpr int l1 = 16 + N, l2 = l1 + N - G0;
  const bool split0 = lane >= 16 - G0 && lane < 16, split1 = lane >= l1 && lane < l2;
  o.isD = lane < N || (lane >= 16 && lane < l1);
  o.isE = HAS_E && lane >= N && lane < 2 * N;
  o.isA = HAS_E ? (split0 || split1) : (lane >= N && lane < 2 * N);
  o.isB = HAS_E ? (lane >= l2 && lane < l2 + N) : (split0 || split1);
  o.isY = HAS_Y && lane == l2;
  const int cs = split0 ? lane - (16 - G0) : lane - l1 + G0;
  o.cc = o.isD ? (lane < N ? lane : lane - 16) : (o.isE ? lane - N : (o.isA ? (HAS_E ? cs : lane - N) : (o.isB ? (HAS_E ? lane - l2 : cs) : 0)));
  return o;
}

// the LDS stand-in: arrays of a pass at made-up places, arbitrary contents, then the record area (table, identity, zeros)
template <int N>
struct Lds {
  static constexpr int nn = N * N, S = 8;
  int oDl, oRl, oCt, oNU, oEl, oGAl, oGBl, ovl, oyl, oyR, oZero, oRec;
  std::vector<double> sm;
  Lds() {
    int o = 0;
    auto take = [&](int n) { const int at = o; o += n; return at; };
    oDl = take((S + 1) * nn); oRl = take((S + 1) * nn); oCt = take(S * nn); oNU = take(S * nn);
    oEl = take(S * nn); oGAl = take(S * nn); oGBl = take(S * nn);
    oyl = take((S + 1) * N); oyR = take((S + 1) * N); ovl = take(S * N);
    oZero = take(N + (N & 1));
    oRec = take(lane_record_doubles<N>());
    sm.resize(o);
    unsigned h = 12345u;
    for (auto& v : sm) { h = h * 1664525u + 1013904223u; v = 1.0 + (double)(h >> 8) / 16777216.0; }      // never 0 or 1: a wrong place shows
    for (int i = 0; i < N + (N & 1); ++i) sm[oZero + i] = 0.0;
    for (int e = 0; e < 2 * nn; ++e) sm[oRec + 128 + e] = (e < nn && e % (N + 1) == 0) ? 1.0 : 0.0;       // as forward_body fills them
  }
  double at(unsigned byte_off) const {
    if (byte_off % 8 != 0 || byte_off / 8 >= sm.size()) { std::printf("address %u outside the stand-in\n", byte_off); std::exit(2); }
    return sm[byte_off / 8];
  }
};

template <bool HAS_E, bool HAS_Y, int N>
static void check_one_node(const char* name) {
  constexpr int nn = N * N;
  const Lds<N> L;
  for (int lane = 0; lane < 64; ++lane) {
    const Roles o = old_roles<HAS_E, HAS_Y, N>(lane);
    const LaneRec rec = lane_record<HAS_E, HAS_Y, N>(lane);
    const unsigned role = rec_role(rec);
    const bool isD = role == ROLE_D, isE = HAS_E && role == ROLE_E, isA = role == ROLE_A, isB = role == ROLE_B, isY = HAS_Y && role == ROLE_Y;
    CHECK(isD == o.isD && isE == o.isE && isA == o.isA && isB == o.isB && isY == o.isY, "%s lane %d roles", name, lane);
    CHECK((int)rec_cc(rec) == o.cc, "%s lane %d cc %u != %d", name, lane, rec_cc(rec), o.cc);
    CHECK(rec_ccN8(rec) == 8u * N * o.cc && rec_cc8(rec) == 8u * o.cc, "%s lane %d cc offsets", name, lane);
    for (int j = 1; j < 6; j += 2)
      for (int nb = 0; nb < 4; ++nb) {                         // has_a, has_b
        const bool has_a = nb & 1, has_b = nb & 2;
        const int oD = L.oDl + j * nn, oR = L.oRl + j * nn, oUa = has_a ? L.oCt + (j - 1) * nn : -1, oUb = has_b ? L.oCt + j * nn : -1;
        const int oy = L.oyl + j * N, oyR = L.oyR + j * N;
        // before
        int p0 = L.oZero, s0 = 0, p1 = L.oZero;
        if (o.isD) { p0 = oD + o.cc * N; s0 = 1; p1 = oR + o.cc * N; }
        else if (o.isA) { if (has_a) { p0 = oUa + o.cc; s0 = N; } }
        else if (o.isB) { if (has_b) { p0 = oUb + o.cc * N; s0 = 1; } }
        else if (o.isY) { p0 = oy; s0 = 1; p1 = oyR; }
        // now (eliminate, REC)
        const int oI = L.oRec + 128, oZ = oI + nn;
        const int bA = has_a ? oUa : oZ, bB = has_b ? oUb : oZ;
        int b0 = oZ, b1 = oZ;
        b0 = isD ? oD : b0; b1 = isD ? oR : b1;
        if (HAS_E) b0 = isE ? oI : b0;
        b0 = isA ? bA : b0;
        b0 = isB ? bB : b0;
        if (HAS_Y) { b0 = isY ? oy : b0; b1 = isY ? oyR : b1; }
        const unsigned a0 = 8u * b0 + rec_off0(rec), a1 = 8u * b1 + rec_off1(rec), st0 = rec_s0(rec);
        for (int r = 0; r < N; ++r) {
          double was = L.sm[p0 + r * s0] + L.sm[p1 + r];
          if (HAS_E) was = o.isE ? (r == o.cc ? 1.0 : 0.0) : was;
          const double is = L.at(a0 + r * st0) + L.at(a1 + 8u * r);
          CHECK(std::memcmp(&was, &is, 8) == 0, "%s lane %d j %d has %d%d row %d column %.17g != %.17g", name, lane, j, has_a, has_b, r, is, was);
        }
        // factor store of the top pass, accumulator adds, the new coupling
        if (o.isE || o.isA || o.isB || o.isY) {
          const int was = o.isE ? L.oEl + o.cc : (o.isA ? L.oGAl + o.cc : (o.isB ? L.oGBl + o.cc : L.ovl));
          const int so = o.isY ? 1 : N;
          const int bf = isE ? L.oEl : (isA ? L.oGAl : (isB ? L.oGBl : L.ovl));
          for (int r = 0; r < N; ++r) CHECK(8u * (was + r * so) == 8u * bf + rec_cc8(rec) + r * rec_so(rec), "%s lane %d factor store", name, lane);
        }
        if (o.isA || o.isY) CHECK(8u * (o.isY ? oyR : oR + o.cc * N) == 8u * (isY ? oyR : oR) + rec_ccN8(rec), "%s lane %d add", name, lane);
        if (o.isB) CHECK(8u * (L.oNU + o.cc * N) == 8u * L.oNU + rec_ccN8(rec), "%s lane %d coupling", name, lane);
      }
  }
}

int main() {
  check_one_node<true, false, 6>("factorisation");
  check_one_node<false, true, 6>("solve");
  if (failures) { std::printf("%d of %ld checks failed\n", failures, checks); return 1; }
  std::printf("ok %ld\n", checks);
  return 0;
}
