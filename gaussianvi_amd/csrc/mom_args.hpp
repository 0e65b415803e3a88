// MomArgs: the argument block of one set's moments launch, whichever kernel family runs it (closed, generic, reg, split, sreg /
// scost, read-out rule); factor_block3_kernel carries one per set.
#pragma once
#include <stdint.h>

#include "factor_dev.hpp"

namespace gvi {

struct MomArgs {
  FactorDev f;
  const double* mu;        // [K][d]
  const double* psi_ext;   // [K][N] host-evaluated psi (HOST_CALLBACK) or nullptr
  double* partial;         // [K][nchunk][npo]
  int64_t chunk;           // points per block (multiple of 256 for generic, 64 for register kernel)
  int nchunk;
  int full;                // 1: all moments, 0: m0 only (cost pass)
  int flush;               // split kernel: steps between second-level flushes (SPLIT_FLUSH; 0 = plain recursive sums, A/B only)
  int64_t mchunk;          // mirror-half table: representatives per chunk (same nchunk)
  const double* pred;      // predicated launch (device_common.hpp, pred_skip) or null
  double pred_val;
};

}  // namespace gvi
