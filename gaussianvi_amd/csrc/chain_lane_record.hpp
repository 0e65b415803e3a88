// What a lane of a two-row chain elimination (kernels_chain.hpp: eliminate<ROWB>) needs to know about ITSELF: its role in the
// tile [D | I | Ua^T | Ub | y], its column inside the group and the offsets that follow from the two.  None of it depends on the
// node or the level, so a pass forms it once per lane (forward_body), keeps it in LDS as packed words and every elimination
// reads it back with one 128-bit load and adds the wave-uniform bases of its node.  Plain C++ on the host as well
// (tests/stubs/chain_lane_record_check.cpp restates the expressions the elimination used before and compares every lane).
#pragma once
#include "chain_plan.hpp"   // lane_record_doubles: the LDS of the pass's table, identity and zero block
#include "hd.hpp"

namespace gvi {
namespace chain {

// a role >= ROLE_E holds a factor column (E / GA / GB / v)
enum : unsigned { ROLE_NONE = 0, ROLE_D = 1, ROLE_E = 2, ROLE_A = 3, ROLE_B = 4, ROLE_Y = 5 };

// All offsets and strides in BYTES of doubles.
//   w0  role [0:3) | cc [4:8) | so [8:16) row stride of the top pass's factor store (y: 8, else 8 N) | s0 [16:24) row stride of
//       the column's first operand (Ua^T: 8 N, else 8)
//   w1  off0 [0:16)  column offset inside the first operand's block (D, I, Ub: 8 N cc; Ua^T: 8 cc; y, none: 0)
//       off1 [16:32) the same for the second operand, the right-hand accumulator (D: 8 N cc; else 0)
//   w2  8 N cc [0:16) | 8 cc [16:32)
//   pad nothing; it makes the record the 16 bytes of one ds_read_b128
struct LaneRec { unsigned w0, w1, w2, pad; };

GVI_HD_INLINE unsigned rec_role(const LaneRec& r) { return r.w0 & 7u; }
GVI_HD_INLINE unsigned rec_cc(const LaneRec& r) { return (r.w0 >> 4) & 15u; }
GVI_HD_INLINE unsigned rec_so(const LaneRec& r) { return (r.w0 >> 8) & 255u; }
GVI_HD_INLINE unsigned rec_s0(const LaneRec& r) { return (r.w0 >> 16) & 255u; }
GVI_HD_INLINE unsigned rec_off0(const LaneRec& r) { return r.w1 & 0xffffu; }
GVI_HD_INLINE unsigned rec_off1(const LaneRec& r) { return r.w1 >> 16; }
GVI_HD_INLINE unsigned rec_ccN8(const LaneRec& r) { return r.w2 & 0xffffu; }
GVI_HD_INLINE unsigned rec_cc8(const LaneRec& r) { return r.w2 >> 16; }

// role and column of a lane in the two-row layout (kernels_chain.hpp, eliminate): lanes 0 .. 31 hold the tile, the rest nothing
//   factorisation   row 0: D(N) | I(N) | Ua^T[0 .. G0)      row 1: D'(N) | Ua^T[G0 .. N) | Ub(N)
//   solve           row 0: D(N) | Ua^T(N) | Ub[0 .. G0)     row 1: D'(N) | Ub[G0 .. N) | y
template <bool HAS_E, bool HAS_Y, int N>
GVI_HD constexpr void lane_role(const int lane, unsigned& role, int& cc) {
  constexpr int G0 = 16 - 2 * N;                                  // columns of the split group (Ua^T / Ub) that fit row 0
  static_assert(G0 > 0 && G0 <= N && 2 * N - G0 + (HAS_E ? N : 1) <= 16, "two-row layout");
  constexpr int l1 = 16 + N, l2 = l1 + N - G0;                    // row 1: rest of the split group, then Ub / y
  const bool split0 = lane >= 16 - G0 && lane < 16, split1 = lane >= l1 && lane < l2;
  const int cs = split0 ? lane - (16 - G0) : lane - l1 + G0;      // column of a lane of the split group
  role = ROLE_NONE;
  cc = 0;
  if (lane < N) { role = ROLE_D; cc = lane; }
  else if (lane >= 16 && lane < l1) { role = ROLE_D; cc = lane - 16; }
  else if (HAS_E && lane >= N && lane < 2 * N) { role = ROLE_E; cc = lane - N; }
  else if (HAS_E ? (split0 || split1) : (lane >= N && lane < 2 * N)) { role = ROLE_A; cc = HAS_E ? cs : lane - N; }
  else if (HAS_E ? (lane >= l2 && lane < l2 + N) : (split0 || split1)) { role = ROLE_B; cc = HAS_E ? lane - l2 : cs; }
  else if (HAS_Y && lane == l2) role = ROLE_Y;
}

// lane_role of all 64 lanes as bit planes (bit l of plane b = bit b of lane l's value), formed at compile time: on the device a
// lane picks its bits out of six constants instead of walking lane_role's branches (a pass forms its table once, in one wave,
// in front of the barrier every other wave waits at)
struct LanePlanes { unsigned long long role[3], cc[3]; };
template <bool HAS_E, bool HAS_Y, int N>
constexpr LanePlanes lane_planes() {
  static_assert(N <= 8, "three bits of cc");
  LanePlanes p{};
  for (int l = 0; l < 64; ++l) {
    unsigned role = 0;
    int cc = 0;
    lane_role<HAS_E, HAS_Y, N>(l, role, cc);
    for (int b = 0; b < 3; ++b) p.role[b] |= (unsigned long long)((role >> b) & 1u) << l;
    for (int b = 0; b < 3; ++b) p.cc[b] |= (unsigned long long)(((unsigned)cc >> b) & 1u) << l;
  }
  return p;
}

template <bool HAS_E, bool HAS_Y, int N>
GVI_HD_INLINE LaneRec lane_record(const int lane) {
  constexpr LanePlanes P = lane_planes<HAS_E, HAS_Y, N>();
  unsigned role = 0, cc = 0;
  GVI_UNROLL
  for (int b = 0; b < 3; ++b) role |= (unsigned)((P.role[b] >> lane) & 1ull) << b;
  GVI_UNROLL
  for (int b = 0; b < 3; ++b) cc |= (unsigned)((P.cc[b] >> lane) & 1ull) << b;
  const unsigned ccN8 = 8u * N * cc, cc8 = 8u * cc, n8 = 8u * N;
  const unsigned so = role == ROLE_Y ? 8u : n8, s0 = role == ROLE_A ? n8 : 8u;
  const unsigned off0 = (role == ROLE_D || role == ROLE_E || role == ROLE_B) ? ccN8 : (role == ROLE_A ? cc8 : 0u);
  const unsigned off1 = role == ROLE_D ? ccN8 : 0u;
  LaneRec r;
  r.w0 = role | (cc << 4) | (so << 8) | (s0 << 16);
  r.w1 = off0 | (off1 << 16);
  r.w2 = ccN8 | (cc8 << 16);
  r.pad = 0;
  return r;
}

// chain_plan.hpp's lane_record_doubles(N) -- the LDS behind the arrays of a two-row pass -- under the block size as a template argument
template <int N> GVI_HD constexpr int lane_record_doubles() { return lane_record_doubles(N); }

}  // namespace chain
}  // namespace gvi
