// The route decisions of gaussianvi_amd/csrc/routes.hpp with the read-out-space rule on (RouteFacts::readout_order), the flag and
// P of the kinds (psi_kinds.hpp) and the accepted orders (readout_moments.hpp), checked on the CPU.  Built plain and with
// AddressSanitizer / UBSan by tests/test_readout_host.py; prints one line per check that fails and "ALL OK" when none does.
#include <cstdio>

#include "readout_moments.hpp"
#include "routes.hpp"

using namespace gvi;

static int failures = 0;
#define CHECK(cond, ...)                                         \
  do {                                                           \
    if (!(cond)) {                                               \
      ++failures;                                                \
      std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                  \
      std::printf("\n");                                         \
    }                                                            \
  } while (0)

static RouteFacts facts(int kind, int d, int K, int order) {
  RouteFacts f;
  f.kind = kind; f.d = d; f.K = K; f.readout_order = order;
  f.has_sdf = true; f.has_arm = true; f.arm_ndof = d;
  f.seg_J = 3;
  f.Np = 1024; f.p = 3;
  return f;
}

int main() {
  const int readout_kinds[6] = {KIND_HINGE_SDF_2D, KIND_HINGE_SDF_3D, KIND_HINGE_SDF_2D_SEG, KIND_HINGE_SDF_3D_SEG, KIND_HINGE_BALLS_2D, KIND_HINGE_BALLS_3D};
  const int P_of[6] = {2, 3, 2, 3, 2, 3};
  const int variants[6] = {0, 1, 2, 5, 6, 7};
  // the flag and P
  for (int kind = -1; kind <= KIND_COUNT; ++kind) {
    int want = 0;
    for (int q = 0; q < 6; ++q)
      if (readout_kinds[q] == kind) want = P_of[q];
    CHECK(psi_kind_readout_P(kind) == want, "kind %d", kind);
    CHECK(psi_kind_is<PSI_READOUT>(kind) == (want != 0), "kind %d", kind);
    CHECK(with_readout_instance(kind, any_instance) == (want != 0), "kind %d", kind);
  }
  // the accepted orders: 2 .. 16 with order^P <= 1024
  for (int order = -2; order <= 20; ++order) {
    CHECK(readout_order_ok(order, 2) == (order >= 2 && order <= 16), "order %d P 2", order);
    CHECK(readout_order_ok(order, 3) == (order >= 2 && order <= 10), "order %d P 3", order);
  }
  CHECK(readout_points(16, 2) == 256 && readout_points(10, 3) == 1000, "points");
  // rule on: Route::Readout, code 8, one wave per factor, under every variant and for both passes
  for (int q = 0; q < 6; ++q)
    for (int v = 0; v < 6; ++v)
      for (int full = 0; full < 2; ++full)
        for (int d : {P_of[q], 4, 8, 12, 32}) {
          if (d < P_of[q]) continue;
          RouteForce force = RouteForce::Auto;
          CHECK(route_force_of_variant(variants[v], &force), "variant %d", variants[v]);
          RouteRules r;
          r.force = force;
          const RouteDecision o = decide_route(facts(readout_kinds[q], d, 67, 8), r, full);
          CHECK(o.status == GVI_OK && o.route == Route::Readout && o.gx == 67u && o.gy == 1u && o.nchunk == 1, "kind %d variant %d d %d: route %d status %d",
                readout_kinds[q], variants[v], d, (int)o.route, (int)o.status);
          CHECK(geometry_code(o.route, false, false) == 8, "code");
          // the caller's psi values stay on the sparse table
          RouteFacts ext = facts(readout_kinds[q], d, 67, 8);
          ext.psi_ext = true;
          const RouteDecision e = decide_route(ext, r, full);
          CHECK(e.route != Route::Readout, "psi_ext kind %d", readout_kinds[q]);
          // order 0: the decision of a set that knows nothing of the rule
          const RouteDecision z = decide_route(facts(readout_kinds[q], d, 67, 0), r, full);
          CHECK(z.route != Route::Readout, "order 0 kind %d", readout_kinds[q]);
          CHECK(z.status != GVI_OK || geometry_code(z.route, false, false) != 8, "order 0 code");
        }
  {
    RouteRules r;
    const RouteDecision o = decide_route(facts(KIND_HINGE_SDF_2D_SEG, 33, 5, 8), r, 1);
    CHECK(o.status == GVI_ERR_UNSUPPORTED && o.why != nullptr, "d = 33");
    const RouteDecision empty = decide_route(facts(KIND_HINGE_SDF_2D_SEG, 8, 0, 8), r, 1);
    CHECK(empty.status == GVI_OK && empty.route == Route::Empty, "K = 0");
    RouteFacts nogrid = facts(KIND_HINGE_SDF_2D_SEG, 8, 5, 8);
    nogrid.has_sdf = false;
    CHECK(decide_route(nogrid, r, 1).status == GVI_ERR_STATE, "a grid kind still needs its grid");
    // a kind without the flag ignores a stray order
    RouteFacts box = facts(KIND_HINGE_BOX, 4, 5, 8);
    box.closed_form = true;
    CHECK(decide_route(box, r, 1).route == Route::Closed, "box");
    CHECK(decide_route(facts(KIND_HINGE_SDF_2D_BODY, 6, 5, 8), r, 1).route != Route::Readout, "body");
  }
  // the planning graph: the one-launch shapes are refused with the rule on the obstacle set
  {
    RouteFacts s[3];
    s[0] = facts(KIND_QUAD_PRIOR, 8, 8, 0); s[0].m = 4;
    s[1] = facts(KIND_HINGE_SDF_2D, 4, 9, 0);
    s[2] = facts(KIND_FIXED_PRIOR, 4, 2, 0); s[2].m = 4;
    CHECK(planar_shape(3, s, RouteForce::Auto), "planar shape without the rule");
    s[1].readout_order = 8;
    CHECK(!planar_shape(3, s, RouteForce::Auto), "planar shape with the rule");
    RouteRules r;
    RouteDecision p[3];
    for (int q = 0; q < 3; ++q) p[q] = decide_route(s[q], r, 1);
    CHECK(p[1].route == Route::Readout, "obstacle set");
    CHECK(decide_fuse(3, s, p, r, false, 1) == Fuse::None, "fuse");
    const bool resident[3] = {false, false, false};
    CHECK(decide_full(3, s, p, resident, r, false, true, 8) == FullFuse::Separate, "full");
  }
  if (failures == 0) std::printf("ALL OK\n");
  return failures == 0 ? 0 : 1;
}
