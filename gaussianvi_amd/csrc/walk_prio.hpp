// Progress-banded wave priority of the fused factor pass's walk (kernels_fused.hpp, phase 2): the arithmetic, shared by the
// host (orbits.hpp fills WalkPrioSet; tests/stubs/walk_prio_check.cpp restates a chunk's walk) and the device (orbit_wave).
// Plain C++17, no HIP.
//
// The fused launch is one residency round: the four blocks of a CU start the walk together and share its SIMDs one wave
// each.  A SIMD arbitrates VALU issue by priority first and by age second, so at equal priority the oldest block runs ahead
// and the youngest ends alone, at one wave per SIMD.  A wave therefore sets its priority from the share of its OWN modelled
// walk cost that is still ahead of it: 3 while more than half is left, then 2, 1, 0 as the rest halves.  A block that has run
// ahead drops a band and yields its issue slots to the blocks still in the band above; the bands are geometric because what
// a leading block can gain inside the last band stays unequalised.  Nothing that is computed depends on it.
//
// The cost model is the one that places the chunk bounds (orbits.hpp, orbit_tile_cost), in whole cycles; a wave's total is
// summed over all items of its block.
#pragma once
#include <stdint.h>

#include "hd.hpp"

namespace gvi {

// per factor set (table x four chunks), a kernel argument: modelled cost of chunk w and of one tile of every support class
struct WalkPrioSet {
  int32_t total[4];
  int32_t tile[8];              // [s], s = 1 .. ORBIT_SMAX (0 where the table has no such class)
};

// the cuts of a wave: remaining cost above cut[0] -> priority 3, above cut[1] -> 2, above cut[2] -> 1, else 0
struct WalkPrioCuts { int c3, c2, c1; };
GVI_HD_INLINE WalkPrioCuts walk_prio_cuts(const int total) { return {total >> 1, total >> 2, total >> 3}; }
GVI_HD_INLINE int walk_prio_band(const int remaining, const WalkPrioCuts& c) {
  return remaining > c.c3 ? 3 : remaining > c.c2 ? 2 : remaining > c.c1 ? 1 : 0;
}

}  // namespace gvi
