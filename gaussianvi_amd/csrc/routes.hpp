// Route selection of the factor stage: which kernel a set's moments (full) or cost pass runs on, how the pass is cut into
// chunks, and which launches of the resident iteration go out as one.  Everything here is arithmetic on a handful of facts
// about a set, its table and the options: decide_route / decide_fuse / decide_full allocate nothing and call no HIP function,
// so tests/test_routes_host.py runs them on the CPU (tests/stubs/routes_check.cpp, plain and sanitized builds).
// launch_factor.inc binds a decision to buffers and kernel arguments (plan_moments) and launches it.  Plain C++17, no HIP.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "options.hpp"
#include "orbits.hpp"
#include "psi_kinds.hpp"

namespace gvi {

// psi operand structs of the register kernels (kernels_reg.hpp defines them): the tags below only name them
template <int D, int M> struct PsiQuad;
struct PsiRange1D;
template <int D, int KIND> struct PsiHingeSdf;
template <int D, int P> struct PsiHingeSeg;
template <int D> struct PsiBoxHinge;

// ---- the compiled instances of the factor kernels ----
// Every kernel family has ONE list, with_<family>_instance: it hands f a tag that carries the template arguments of the
// instance compiled for the shape and returns true, or returns false where there is none.  <family>_supported asks the list
// with a no-op and the launch instantiates the kernel from the tag, so a new instance is registered by one line in its list.
// These lists and the shape predicates (chain_pair_shape, planar_shape) choose KERNELS by kind; every FACT about a kind --
// what it keeps, reads and offers -- is a row of psi_kinds.hpp.
template <int D, typename Psi> struct RegInst {};
template <int D, int M, bool PIPE> struct SregInst { static constexpr bool pipe = PIPE; };   // PIPE: the hand-pipelined body fits 256 registers
template <int D, int M> struct ScostInst {};
template <int D, int R> struct SplitInst {};
template <int M, int SMAX, int WAVES, bool PAIR> struct OrbitInst { static constexpr int waves = WAVES; static constexpr bool pair = PAIR; };
template <int KIND> struct OrbitPsiInst {};
template <int M, int SMAX, int WAVES, int D0, int D1> struct FusedInst {};
struct ClosedSumsq {};
struct ClosedBox {};
struct ClosedHalfspace {};
template <int P, int CLS> struct ReadoutInst {};   // CLS: READOUT_LEAD / _SEG / _BALLS, how the kind lays its read-outs out (psi_kinds.hpp)
template <int EPLP> struct PrepInst {};            // EPLP: elements of the d x d block a lane holds (kernels_prep.hpp)
constexpr auto any_instance = [](auto) {};
template <class F, class Inst> bool hit(F& f, Inst inst) { f(inst); return true; }

// moments_reg_kernel<D, Psi, full>: lane-per-point, psi operands in LDS
template <class F>
bool with_reg_instance(int kind, int d, int m, F&& f) {
  switch (kind) {
    case KIND_RANGE_1D:
      if (d == 1) return hit(f, RegInst<1, PsiRange1D>{});
      break;
    case KIND_HINGE_SDF_2D:
      if (d == 2) return hit(f, RegInst<2, PsiHingeSdf<2, KIND_HINGE_SDF_2D>>{});
      if (d == 4) return hit(f, RegInst<4, PsiHingeSdf<4, KIND_HINGE_SDF_2D>>{});
      if (d == 6) return hit(f, RegInst<6, PsiHingeSdf<6, KIND_HINGE_SDF_2D>>{});
      break;
    case KIND_HINGE_SDF_2D_BODY:
      if (d == 3) return hit(f, RegInst<3, PsiHingeSdf<3, KIND_HINGE_SDF_2D_BODY>>{});
      if (d == 6) return hit(f, RegInst<6, PsiHingeSdf<6, KIND_HINGE_SDF_2D_BODY>>{});
      break;
    case KIND_HINGE_SDF_3D:
      if (d == 3) return hit(f, RegInst<3, PsiHingeSdf<3, KIND_HINGE_SDF_3D>>{});
      if (d == 6) return hit(f, RegInst<6, PsiHingeSdf<6, KIND_HINGE_SDF_3D>>{});
      break;
    case KIND_HINGE_SDF_2D_SEG:
      if (d == 4) return hit(f, RegInst<4, PsiHingeSeg<4, 2>>{});
      if (d == 8) return hit(f, RegInst<8, PsiHingeSeg<8, 2>>{});
      if (d == 12) return hit(f, RegInst<12, PsiHingeSeg<12, 2>>{});
      break;
    case KIND_HINGE_SDF_3D_SEG:   // d = 12: 256 VGPRs + 18 AGPR copies under launch_bounds(256) -> generic kernel
      if (d == 6) return hit(f, RegInst<6, PsiHingeSeg<6, 3>>{});
      break;
    // analytic balls: the policy is PsiHingeBalls<D, P> (kernels_reg.hpp), handed out under the tag of every hinge on a
    // signed distance, PsiHingeSdf<D, KIND>.  Every listed instance compiles without scratch or spills
    case KIND_HINGE_BALLS_2D:
      if (d == 2) return hit(f, RegInst<2, PsiHingeSdf<2, KIND_HINGE_BALLS_2D>>{});
      if (d == 4) return hit(f, RegInst<4, PsiHingeSdf<4, KIND_HINGE_BALLS_2D>>{});
      if (d == 8) return hit(f, RegInst<8, PsiHingeSdf<8, KIND_HINGE_BALLS_2D>>{});
      if (d == 12) return hit(f, RegInst<12, PsiHingeSdf<12, KIND_HINGE_BALLS_2D>>{});
      break;
    case KIND_HINGE_BALLS_3D:
      if (d == 3) return hit(f, RegInst<3, PsiHingeSdf<3, KIND_HINGE_BALLS_3D>>{});
      if (d == 6) return hit(f, RegInst<6, PsiHingeSdf<6, KIND_HINGE_BALLS_3D>>{});
      if (d == 12) return hit(f, RegInst<12, PsiHingeSdf<12, KIND_HINGE_BALLS_3D>>{});
      break;
    case KIND_HINGE_BOX:          // above d = 8 the accumulators leave no room: generic kernel, or the closed form
      if (d == 2) return hit(f, RegInst<2, PsiBoxHinge<2>>{});
      if (d == 4) return hit(f, RegInst<4, PsiBoxHinge<4>>{});
      if (d == 6) return hit(f, RegInst<6, PsiBoxHinge<6>>{});
      if (d == 8) return hit(f, RegInst<8, PsiBoxHinge<8>>{});
      break;
    case KIND_QUAD_PRIOR:
      if (d != 2 * m) break;
      if (d == 2) return hit(f, RegInst<2, PsiQuad<2, 1>>{});
      if (d == 4) return hit(f, RegInst<4, PsiQuad<4, 2>>{});
      if (d == 6) return hit(f, RegInst<6, PsiQuad<6, 3>>{});
      if (d == 8) return hit(f, RegInst<8, PsiQuad<8, 4>>{});
      if (d == 12) return hit(f, RegInst<12, PsiQuad<12, 6>>{});
      break;
    case KIND_FIXED_PRIOR:
      if (d != m) break;
      if (d == 1) return hit(f, RegInst<1, PsiQuad<1, 1>>{});
      if (d == 2) return hit(f, RegInst<2, PsiQuad<2, 2>>{});
      if (d == 3) return hit(f, RegInst<3, PsiQuad<3, 3>>{});
      if (d == 4) return hit(f, RegInst<4, PsiQuad<4, 4>>{});
      if (d == 6) return hit(f, RegInst<6, PsiQuad<6, 6>>{});
      if (d == 8) return hit(f, RegInst<8, PsiQuad<8, 8>>{});
      if (d == 12) return hit(f, RegInst<12, PsiQuad<12, 12>>{});
      break;
  }
  return false;
}

// moments_sreg_kernel<D, M, full, pipelined>: lane-per-point, psi operands from SGPRs
template <class F>
bool with_sreg_instance(int kind, int d, int m, F&& f) {
  if (kind == KIND_QUAD_PRIOR && d == 2 * m) {
    if (d == 4) return hit(f, SregInst<4, 2, true>{});
    if (d == 8) return hit(f, SregInst<8, 4, true>{});
    if (d == 12) return hit(f, SregInst<12, 6, true>{});
  }
  if (kind == KIND_FIXED_PRIOR && d == m) {
    if (d == 6) return hit(f, SregInst<6, 6, true>{});
    if (d == 12) return hit(f, SregInst<12, 12, false>{});   // M = 12: the pipelined body does not fit 256 registers
  }
  return false;
}

// moments_scost_kernel<D, M, 2>: cost pass with two factors per wave (grid.x shrinks by 2); only the headline shapes
template <class F>
bool with_scost_instance(int kind, int d, int m, F&& f) {
  if (kind == KIND_QUAD_PRIOR && d == 12 && m == 6) return hit(f, ScostInst<12, 6>{});
  if (kind == KIND_FIXED_PRIOR && d == 6 && m == 6) return hit(f, ScostInst<6, 6>{});
  return false;
}

// moments_split_kernel<D, R, full> (one block per factor and chunk), R = ceil(m / 4) row blocks: m = d and m = d / 2
template <class F>
bool with_split_instance(int d, int m, F&& f) {
  if (d == 16 && m == 8) return hit(f, SplitInst<16, 2>{});
  if (d == 16 && m == 16) return hit(f, SplitInst<16, 4>{});
  if (d == 20 && m == 10) return hit(f, SplitInst<20, 3>{});
  if (d == 20 && m == 20) return hit(f, SplitInst<20, 5>{});
  if (d == 24 && m == 12) return hit(f, SplitInst<24, 3>{});
  if (d == 24 && m == 24) return hit(f, SplitInst<24, 6>{});
  return false;
}

// moments_orbit_kernel<M, SMAX, full, signed, WAVES>, and where PAIR moments_orbit_pair_kernel<M, SMAX, full, false, WAVES>:
// smax is the largest support of the table's orbits (of both tables for the pair).  m = 2 is instantiated for supports <= 4
// (every table of d <= 4, wider ones to degree 5), m = 14 (the d = 28 priors of the arm graph) likewise and on its own only.
template <class F>
bool with_orbit_instance(int m, int smax, F&& f) {
  if (smax < 1 || smax > ORBIT_SMAX) return false;
  if (m == 2 && smax <= 4) return hit(f, OrbitInst<2, 4, 4, true>{});
  if (m == 14 && smax <= 4) return hit(f, OrbitInst<14, 4, 2, false>{});
  if (m == 6) return smax <= 4 ? hit(f, OrbitInst<6, 4, 4, true>{}) : hit(f, OrbitInst<6, 6, 2, true>{});
  if (m == 12) return smax <= 4 ? hit(f, OrbitInst<12, 4, 3, true>{}) : hit(f, OrbitInst<12, 6, 2, true>{});
  return false;
}

// moments_orbit_psi_kernel<KIND, full>
template <class F>
bool with_orbit_psi_instance(int kind, F&& f) {
  switch (kind) {
    case KIND_RANGE_1D: return hit(f, OrbitPsiInst<KIND_RANGE_1D>{});
    case KIND_HINGE_SDF_2D: return hit(f, OrbitPsiInst<KIND_HINGE_SDF_2D>{});
    case KIND_HINGE_SDF_2D_BODY: return hit(f, OrbitPsiInst<KIND_HINGE_SDF_2D_BODY>{});
    case KIND_HINGE_SDF_3D: return hit(f, OrbitPsiInst<KIND_HINGE_SDF_3D>{});
    case KIND_HINGE_SDF_3D_ARM: return hit(f, OrbitPsiInst<KIND_HINGE_SDF_3D_ARM>{});
  }
  return false;
}

// factor_fused_kernel<M, SMAX, WAVES, D0, D1>: the chain patterns of BASELINE configs[1..3] (binary prior d = 2n + unary
// factor d = n); smax over both tables
template <class F>
bool with_fused_instance(int m, int smax, int d0, int d1, F&& f) {
  if (smax < 1 || smax > ORBIT_SMAX) return false;
  if (m == 6 && d0 == 12 && d1 == 6) return smax <= 4 ? hit(f, FusedInst<6, 4, 4, 12, 6>{}) : hit(f, FusedInst<6, 6, 2, 12, 6>{});
  if (m == 2 && d0 == 4 && d1 == 2 && smax <= 4) return hit(f, FusedInst<2, 4, 4, 4, 2>{});
  return false;
}

// the quadrature-free kernels (PSI_CLOSED kinds): moments_closed_kernel, moments_box_closed_kernel, moments_halfspace_closed_kernel
template <class F>
bool with_closed_instance(int kind, F&& f) {
  switch (kind) {
    case KIND_QUAD_PRIOR:
    case KIND_FIXED_PRIOR: return hit(f, ClosedSumsq{});
    case KIND_HINGE_BOX: return hit(f, ClosedBox{});
    case KIND_HINGE_HALFSPACE: return hit(f, ClosedHalfspace{});
  }
  return false;
}

// moments_readout_kernel<P, CLS> (kernels_readout.hpp): the PSI_READOUT kinds, any d <= 32
template <class F>
bool with_readout_instance(int kind, F&& f) {
  switch (kind) {
    case KIND_HINGE_SDF_2D: return hit(f, ReadoutInst<2, READOUT_LEAD>{});
    case KIND_HINGE_SDF_3D: return hit(f, ReadoutInst<3, READOUT_LEAD>{});
    case KIND_HINGE_SDF_2D_SEG: return hit(f, ReadoutInst<2, READOUT_SEG>{});
    case KIND_HINGE_SDF_3D_SEG: return hit(f, ReadoutInst<3, READOUT_SEG>{});
    case KIND_HINGE_BALLS_2D: return hit(f, ReadoutInst<2, READOUT_BALLS>{});
    case KIND_HINGE_BALLS_3D: return hit(f, ReadoutInst<3, READOUT_BALLS>{});
  }
  return false;
}

// prep_kernel<EPLP>, prep_all_kernel<EPLP, ROWB> (kernels_prep.hpp): one wave per factor, so the d x d block of the widest
// factor of the launch sets the elements per lane; any d <= 32
template <class F>
bool with_prep_instance(int d, F&& f) {
  if (d <= 8) return hit(f, PrepInst<1>{});
  if (d <= 16) return hit(f, PrepInst<4>{});
  if (d <= 32) return hit(f, PrepInst<16>{});
  return false;
}

inline bool reg_supported(int kind, int d, int m) { return with_reg_instance(kind, d, m, any_instance); }
inline bool sreg_supported(int kind, int d, int m) { return with_sreg_instance(kind, d, m, any_instance); }
inline bool scost_supported(int kind, int d, int m) { return with_scost_instance(kind, d, m, any_instance); }
// sum-of-squares kinds on a coded table
inline bool split_supported(int kind, int d, int m, bool coded) {
  return psi_kind_is<PSI_SUMSQ>(kind) && coded && with_split_instance(d, m, any_instance);
}
inline bool orbit_pair_supported(int m, int smax) {
  bool pair = false;
  with_orbit_instance(m, smax, [&](auto inst) { pair = inst.pair; });
  return pair;
}

// ---- route forcing (gvi_set_variant) ----
// Auto takes the fastest kernel there is for a set; the others are the A/B legs.  AutoOrbitPsi is Auto, but the
// non-polynomial psi kinds take the sign-orbit kernel also where a register kernel exists.
enum class RouteForce { Auto, Generic, Reg, SgprReg, Orbit, AutoOrbitPsi };

// the public integers of gvi_set_variant; false: not a variant (3 and 4, the round-1 A/B kernels, are gone)
inline bool route_force_of_variant(int variant, RouteForce* out) {
  switch (variant) {
    case 0: *out = RouteForce::Auto; return true;
    case 1: *out = RouteForce::Generic; return true;
    case 2: *out = RouteForce::Reg; return true;
    case 5: *out = RouteForce::SgprReg; return true;
    case 6: *out = RouteForce::Orbit; return true;
    case 7: *out = RouteForce::AutoOrbitPsi; return true;
  }
  return false;
}
// may take a register kernel (lane-per-point or split): everything but the forced generic kernel
constexpr bool may_take_reg(RouteForce f) { return f != RouteForce::Generic; }
// a pass without a register instance is refused
constexpr bool must_take_reg(RouteForce f) { return f == RouteForce::Reg; }
// may take the SGPR-operand kernels where instantiated (fastest for both passes); otherwise the operand-resident kernel for
// the cost pass and the LDS-operand kernel for the full pass
constexpr bool may_take_sgpr(RouteForce f) { return f == RouteForce::Auto || f == RouteForce::AutoOrbitPsi || f == RouteForce::SgprReg; }
// may take the sign-orbit kernel
constexpr bool may_take_orbit(RouteForce f) { return f == RouteForce::Auto || f == RouteForce::AutoOrbitPsi || f == RouteForce::Orbit; }
// prefers the non-polynomial sign-orbit kernel to a register kernel
constexpr bool prefers_orbit_psi(RouteForce f) { return f == RouteForce::AutoOrbitPsi; }

// ---- what a decision reads ----
struct RouteFacts {
  // of the set
  int kind = 0, d = 0, m = 0, K = 0;
  bool closed_form = false, all_pos = false;
  int readout_order = 0;              // > 0: the read-out-space rule is on (gvi_factors_set_readout_rule; PSI_READOUT kinds only)
  bool psi_ext = false;              // the caller supplies psi at the sigma points (gvi_moments_from_psi)
  bool has_arm = false, has_sdf = false;
  int arm_ndof = 0, seg_J = 0;
  int opsi_rows = 0;                  // leading coordinates the kind's register psi reads: psi_kind_lead (psi_kinds.hpp)
  // of its table
  int64_t Np = 0, Nmp = 0;
  int p = 0;
  bool coded = false, has_Zq = false;
  bool orb_ok = false;                // sign-orbit form (orbits.hpp): complete orbits, largest support, 64-lane tiles
  int orb_smax = 0;
  int64_t orb_tiles = 0;
};

struct RouteRules {
  RouteForce force = RouteForce::Auto;
  bool orbit = true, no_scost = false, sreg_pipe = true;
  int target_waves = 2048, orbit_waves = 4096, orbit_min_tiles = 6;
  bool pair_fuse = true, fused = true, chol_sqrt = true;   // decide_fuse / decide_full
};
inline RouteRules route_rules(const Options& o, RouteForce force) {
  RouteRules r;
  r.force = force;
  r.orbit = o.orbit; r.no_scost = o.no_scost; r.sreg_pipe = o.sreg_pipe;
  r.target_waves = o.target_waves; r.orbit_waves = o.orbit_waves; r.orbit_min_tiles = o.orbit_min_tiles;
  r.pair_fuse = o.pair_fuse; r.fused = o.fused; r.chol_sqrt = o.chol_sqrt;
  return r;
}

enum class Route { Empty, Closed, Orbit, OrbitPsi, Split, Sreg, Scost, Reg, Generic, Readout };
// lane-per-point register kernels: a block's four waves take four factors, grid ((K + 3) / 4, nchunk) but for Scost's own launch
constexpr bool lane_per_point(Route r) { return r == Route::Sreg || r == Route::Scost || r == Route::Reg; }

struct RouteDecision {
  gvi_status status = GVI_OK;
  const char* why = nullptr;          // text of the refusal
  Route route = Route::Empty;
  int nchunk = 1;
  int64_t chunk = 0, mchunk = 0;      // points per chunk of the table / of its mirror half
  unsigned gx = 0, gy = 1;            // grid of the set's own launch (Closed: K blocks, re-shaped by the bind step for HINGE_HALFSPACE)
  bool pipe = false;                  // Sreg: the hand-pipelined body
};

// ---- chunking ----
struct Chunks { int nchunk; int64_t chunk; };
// about nch chunks of whole 256-point tiles (Np is a multiple of 256)
inline Chunks chunk_tiles(int64_t Np, int64_t nch) {
  const int64_t iters = Np / 256;
  nch = std::min<int64_t>(std::max<int64_t>(1, nch), std::max<int64_t>(1, iters));
  const int64_t chunk = (iters + nch - 1) / nch * 256;
  return {(int)((Np + chunk - 1) / chunk), chunk};
}
// lane-per-point kernels: target_waves waves over the set; generic kernel: ~1024 blocks
inline Chunks plan_chunks(int64_t Np, int K, bool reg, int target_waves) { return chunk_tiles(Np, ((reg ? target_waves : 1024) + K - 1) / K); }
// sign-orbit kernels: enough waves to fill the chip, but at least orbit_min_tiles tiles per wave -- a wave's prologue (H into
// LDS, zeroing the accumulator copies) and its reduction of the copies cost about as much as two tiles
inline Chunks orbit_chunks(int64_t Np, int K, int64_t tiles, int orbit_waves, int orbit_min_tiles) {
  const int64_t by_waves = std::max<int64_t>(1, (orbit_waves + K - 1) / K);
  const int64_t by_tiles = std::max<int64_t>(1, tiles / std::max(1, orbit_min_tiles));
  return {(int)std::min<int64_t>(tiles, std::min(by_waves, by_tiles)), Np};
}
// split kernel: ~2 blocks per CU (K * nchunk >= 1024), and <= 16k points per lane, which bounds the rounding of the
// sequential sums (|w|_1 ~ 2e7 at (24,7))
inline Chunks split_chunks(int64_t Np, int K) {
  const int64_t tiles = Np / 64;
  int64_t nch = std::max<int64_t>(1, (1024 + K - 1) / K);
  nch = std::max<int64_t>(nch, (tiles + 16383) / 16384);
  nch = std::min<int64_t>(nch, tiles);
  const int64_t chunk = (tiles + nch - 1) / nch * 64;
  return {(int)((Np + chunk - 1) / chunk), chunk};
}
constexpr int cost_chunk_mult = 8;    // cost pass of the two-factor kernel: chunks per factor relative to the full pass

// sign-orbit kernel (kernels_orbit.hpp): sum-of-squares kinds on a table of complete sign orbits
inline bool orbit_supported(const RouteFacts& s, const RouteRules& r) {
  if (!r.orbit || !may_take_orbit(r.force)) return false;
  if (!psi_kind_is<PSI_SUMSQ>(s.kind)) return false;
  return s.d <= 32 && s.orb_ok && s.orb_tiles > 0 && with_orbit_instance(s.m, s.orb_smax, any_instance);
}
// its sibling for the non-polynomial psi kinds (kernels_orbit_psi.hpp).  Measured (profiles/r04_*): with a non-polynomial psi
// the evaluations themselves dominate and a lane that walks an orbit evaluates its 2^s points ONE AFTER THE OTHER -- planar
// hinge factors (d = 4, p = 7): 30.8 us against 19.0 us of the lane-per-point register kernel; the arm graph's 129 factors x
// 421 points: 120 us slower per pass than the generic kernel, which keeps 54 k points in flight.  It stays as the A/B leg and
// as the parity cross-check (three independent kernels for these kinds).
inline bool orbit_psi_supported(const RouteFacts& s, const RouteRules& r) {
  if (!r.orbit || !prefers_orbit_psi(r.force)) return false;
  if (!with_orbit_psi_instance(s.kind, any_instance)) return false;
  if (!(s.orb_ok && s.orb_smax >= 1 && s.orb_smax <= 4 && s.orb_tiles > 0) || s.d > 32) return false;
  if (psi_kind_is<PSI_ARM>(s.kind) && (s.arm_ndof < 1 || s.arm_ndof > s.opsi_rows)) return false;
  return s.opsi_rows <= s.d;
}

// The route of one set's pass, its chunking and the grid of its own launch.  Refusals that need size functions of the
// kernel headers (LDS budgets, accumulator copies, the half-space block shape) are the bind step's.
inline RouteDecision decide_route(const RouteFacts& s, const RouteRules& r, int full) {
  RouteDecision o;
  o.chunk = s.Np;
  auto refuse = [&](gvi_status st, const char* why) { o.status = st; o.why = why; return o; };
  if (s.K == 0) return o;             // empty shard
  if (psi_kind_is<PSI_ARM>(s.kind) && !s.psi_ext && !s.has_arm)
    return refuse(GVI_ERR_STATE, "HINGE_SDF_3D_ARM set without an arm model: call gvi_factors_set_arm");
  if (psi_kind_is<PSI_SDF>(s.kind) && !s.psi_ext && !s.has_sdf)
    return refuse(GVI_ERR_STATE, "HINGE_SDF set without a grid: call gvi_factors_set_sdf2d / gvi_factors_set_sdf3d");
  const bool closed = s.closed_form && !s.psi_ext;
  // the read-out-space rule is the set's own choice of quadrature, not a kernel variant: it holds under every force, before
  // the sparse routes and their refusals; a pass on the caller's psi values walks the caller's sigma points
  if (s.readout_order > 0 && !closed && !s.psi_ext && with_readout_instance(s.kind, any_instance)) {
    if (s.d > 32) return refuse(GVI_ERR_UNSUPPORTED, "read-out rule kernel supports d <= 32");
    o.route = Route::Readout;
    o.gx = (unsigned)s.K; o.gy = 1;   // one wave per factor, re-shaped by the bind step
    return o;
  }
  const bool reg_inst = reg_supported(s.kind, s.d, s.m) && !s.psi_ext && may_take_reg(r.force);
  if (must_take_reg(r.force) && !reg_inst && !s.psi_ext)
    return refuse(GVI_ERR_UNSUPPORTED, "register kernel not instantiated for this (kind, d)");
  const bool orbit = !closed && !s.psi_ext && orbit_supported(s, r);
  const bool opsi = !closed && !orbit && !s.psi_ext && orbit_psi_supported(s, r);
  const bool reg = reg_inst && !closed && !orbit && !opsi;
  const bool split = !closed && !orbit && !opsi && !reg_inst && !s.psi_ext && may_take_reg(r.force) && split_supported(s.kind, s.d, s.m, s.coded);
  Chunks c{1, s.Np};                  // the closed forms walk no table
  if (orbit || opsi) c = orbit_chunks(s.Np, s.K, s.orb_tiles, r.orbit_waves, r.orbit_min_tiles);
  else if (split) c = split_chunks(s.Np, s.K);
  else if (!closed) c = plan_chunks(s.Np, s.K, reg, r.target_waves);
  const bool sgpr = reg && may_take_sgpr(r.force);
  const bool scost = sgpr && !full && scost_supported(s.kind, s.d, s.m) && !r.no_scost;
  if (scost) c = chunk_tiles(s.Np, (int64_t)c.nchunk * cost_chunk_mult);   // two factors per wave: keep the wave count up with more, shorter chunks
  o.nchunk = c.nchunk; o.chunk = c.chunk;
  if (s.Nmp > 0) o.mchunk = (s.Nmp / 64 + c.nchunk - 1) / c.nchunk * 64;   // same number of chunks over the mirror-half table
  o.gx = (unsigned)((s.K + 3) / 4); o.gy = (unsigned)c.nchunk;
  if (closed) {
    o.route = Route::Closed;
    o.gx = (unsigned)s.K; o.gy = 1;
    if (s.kind == KIND_HINGE_HALFSPACE && s.d > 32) return refuse(GVI_ERR_UNSUPPORTED, "closed-form HINGE_HALFSPACE kernel supports d <= 32");
  } else if (orbit) {
    o.route = Route::Orbit;
  } else if (opsi) {
    o.route = Route::OrbitPsi;
  } else if (split) {
    o.route = Route::Split;
    o.gx = (unsigned)s.K;
  } else if (scost) {
    o.route = Route::Scost;
    o.gx = (unsigned)((s.K + 7) / 8);
  } else if (sgpr && sreg_supported(s.kind, s.d, s.m)) {
    o.route = Route::Sreg;
    with_sreg_instance(s.kind, s.d, s.m, [&](auto inst) { o.pipe = inst.pipe && r.sreg_pipe && s.has_Zq; });
  } else if (reg) {
    o.route = Route::Reg;
  } else {
    o.route = Route::Generic;
    o.gx = (unsigned)s.K;
    if (s.d > 32) return refuse(GVI_ERR_UNSUPPORTED, "generic kernel supports d <= 32");
  }
  return o;
}

// ---- which launches of the resident iteration go out as one ----
// the chain pattern of the two-set SGPR launches (moments_sreg_pair_kernel / moments_scost_pair_kernel <12, 6, 6, 6>): set 0
// binary priors d = 12, set 1 unary factors d = 6
inline bool chain_pair_shape(const RouteFacts& s0, const RouteFacts& s1) {
  return s0.kind == KIND_QUAD_PRIOR && s1.kind == KIND_FIXED_PRIOR && s0.d == 12 && s1.d == 6;
}

// the planning graph of the three-set launches (moments_planar3_kernel, factor_block3_kernel): d = 8 priors + d = 4
// hinge-on-SDF obstacle factors + d = 4 anchors, registered in this order, none empty
inline bool planar_shape(int nsets, const RouteFacts* s, RouteForce force) {
  if (nsets != 3 || force != RouteForce::Auto) return false;
  if (s[1].readout_order > 0) return false;   // moments_planar3_kernel / factor_block3_kernel are compiled for the sparse route
  return s[0].kind == KIND_QUAD_PRIOR && s[0].d == 8 && s[0].m == 4 && s[1].kind == KIND_HINGE_SDF_2D && s[1].d == 4 &&
         s[2].kind == KIND_FIXED_PRIOR && s[2].d == 4 && !s[0].closed_form && !s[2].closed_form && s[0].K > 0 && s[1].K > 0 && s[2].K > 0;
}

// All sets' moments (full = 1) or cost (full = 0) launches: two sign-orbit sets of one instance with sgn = +1, the chain
// pattern on the SGPR-operand kernels (Sreg / Sreg in the full pass, Scost / Scost in the cost pass) and the planning graph
// on three lane-per-point kernels go out as ONE launch; every other combination as one launch per set.
enum class Fuse { None, OrbitPair, SregPair, ScostPair, Planar3 };
inline Fuse decide_fuse(int nsets, const RouteFacts* s, const RouteDecision* p, const RouteRules& r, bool profile_all, int full) {
  if (!r.pair_fuse || profile_all) return Fuse::None;
  if (nsets == 2) {
    if (p[0].route == Route::Orbit && p[1].route == Route::Orbit && s[0].m == s[1].m && s[0].all_pos && s[1].all_pos &&
        orbit_pair_supported(s[0].m, std::max(s[0].orb_smax, s[1].orb_smax)))
      return Fuse::OrbitPair;
    const Route want = full ? Route::Sreg : Route::Scost;
    if (chain_pair_shape(s[0], s[1]) && p[0].route == want && p[1].route == want) return full ? Fuse::SregPair : Fuse::ScostPair;
  }
  if (planar_shape(nsets, s, r.force) && lane_per_point(p[0].route) && lane_per_point(p[1].route) && lane_per_point(p[2].route))
    return Fuse::Planar3;
  return Fuse::None;
}

// Cholesky factor instead of the symmetric root: sum-of-squares psi on a generated table of degree >= 3 (exact quadrature --
// kernels_prep.hpp, prep_chol_body), the instantiated dimensions, and not when the caller is going to look at the sigma
// points themselves (force_sym: gvi_expand / gvi_moments_from_psi) or runs the JKO map
inline bool chol_products(int kind, int d, int table_p, bool chol_sqrt, bool force_sym) {
  return chol_sqrt && !force_sym && psi_kind_is<PSI_SUMSQ>(kind) && table_p >= 3 && d <= 32;
}

// factor_fused_kernel: blocks that own items -- one per factor of the first (heavy) set; a longer second set wraps around
// (block b also takes its items b + nblk, ...).  0: more than max_items (FUSED_MAX_ITEMS) items per block would be needed.
inline int fused_nblk(int K0, int K1, int max_items) {
  const int nblk = K0;
  const int per = 1 + (K1 + nblk - 1) / nblk;
  return per <= max_items ? nblk : 0;
}
// key of the fused instance (with_fused_instance): m and the second dimension of a one-set problem as the chain pattern has them
struct FusedKey { int m, smax, d0, d1; };
inline FusedKey fused_key(int nsets, const RouteFacts* s) {
  FusedKey k{s[0].m, 0, s[0].d, nsets > 1 ? s[1].d : s[0].d / 2};
  for (int i = 0; i < nsets; ++i) k.smax = std::max(k.smax, s[i].orb_smax);
  return k;
}

// The full pass of the resident iteration.  Fused: factor_fused_kernel, every set on the sign-orbit kernel's walk with four
// chunks per factor, chosen whatever the sets' own decisions say.  Block3: factor_block3_kernel, the planning graph with
// three lane-per-point decisions of at most four chunks per factor (a workgroup's four waves take them).  Both need the
// natural-gradient rule (the JKO map reads the sets' Sigma^-1 after the pass), the products of the state not resident yet
// (resident[i]: the plain route would skip the prep) and the products the kernels are compiled for.
enum class FullFuse { Fused, Block3, Separate };
inline FullFuse decide_full(int nsets, const RouteFacts* s, const RouteDecision* p, const bool* resident, const RouteRules& r,
                            bool profile_all, bool ngd_rule, int fused_max_items) {
  if (!r.fused || !r.pair_fuse || profile_all || !ngd_rule || nsets < 1) return FullFuse::Separate;
  for (int i = 0; i < nsets; ++i)
    if (resident[i]) return FullFuse::Separate;
  auto chol = [&](int i) { return chol_products(s[i].kind, s[i].d, s[i].p, r.chol_sqrt, false); };
  if (nsets <= 2) {
    const FusedKey k = fused_key(nsets, s);
    for (int i = 0; i < nsets; ++i)
      if (!orbit_supported(s[i], r) || !s[i].all_pos || s[i].closed_form || s[i].K <= 0 || s[i].m != k.m || !chol(i)) return FullFuse::Separate;
    if (!with_fused_instance(k.m, k.smax, k.d0, k.d1, any_instance)) return FullFuse::Separate;
    return fused_nblk(s[0].K, nsets > 1 ? s[1].K : 0, fused_max_items) > 0 ? FullFuse::Fused : FullFuse::Separate;
  }
  if (!planar_shape(nsets, s, r.force)) return FullFuse::Separate;
  if (!chol(0) || chol(1) || !chol(2)) return FullFuse::Separate;     // the products the kernel is compiled for (kernels_block.hpp)
  for (int q = 0; q < 3; ++q)
    if (!lane_per_point(p[q].route) || p[q].nchunk > 4) return FullFuse::Separate;
  return FullFuse::Block3;
}

// ---- what was launched ----
// The record of a set's last moments / cost launch, for gvi_profile_geometry.  One writer: record_pass, called by the code
// that launches.  The default is what a set reports before any pass.
struct PassRecord {
  Route route = Route::Generic;
  bool fused_pair = false;            // went out in one launch with the other set
  int nchunk = 1;
  int64_t chunk = 0;
};
inline void record_pass(PassRecord& last, Route route, bool fused_pair, int nchunk, int64_t chunk) {
  last.route = route; last.fused_pair = fused_pair; last.nchunk = nchunk; last.chunk = chunk;
}

// the integers gvi_profile_geometry reports: 0 closed form, 7 / 6 sign-orbit kernels, 5 SGPR pair launch, 2 lane-per-point,
// 3 split, 1 generic, 8 read-out-space rule
inline int geometry_code(Route route, bool fused_pair, bool closed_form) {
  if (route == Route::Readout) return 8;
  if (closed_form) return 0;
  if (route == Route::OrbitPsi) return 7;
  if (route == Route::Orbit) return 6;
  if (fused_pair) return 5;
  if (lane_per_point(route)) return 2;
  if (route == Route::Split) return 3;
  return 1;
}

}  // namespace gvi
