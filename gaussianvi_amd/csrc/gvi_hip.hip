// C-ABI implementation (include/gvi_hip.h): the index of the library's ONE translation unit.  The kernel templates are
// instantiated from the host launchers, so the host code is not split into units of its own; it is cut into the .inc fragments
// below, each of which sees the headers included here and the fragments before it ("Where the host code lives").
// This file defines nothing.
#include "../../include/gvi_hip.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <map>
#include <set>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "host_linalg.hpp"
#include "kernels_bt.hpp"
#include "chain_launch.hpp"
#include "kernels_factor.hpp"
#include "kernels_orbit.hpp"
#include "kernels_fused.hpp"
#include "kernels_block.hpp"
#include "kernels_orbit_psi.hpp"
#include "kernels_readout.hpp"
#include "kernels_sample.hpp"
#include "kernels_solve.hpp"
#include "kernels_interp.hpp"
#include "kernels_sample_cost.hpp"
#include "options.hpp"
#include "orbits.hpp"
#include "routes.hpp"
#include "spgh.hpp"

using namespace gvi;

// types and helpers, then binding and launching; each fragment in an anonymous namespace of its own
#include "host_ctx.inc"
#include "launch_factor.inc"
#include "launch_chain.inc"

// =============================================================================================
extern "C" {

// context, tables, factor sets; per-pass and joint operators
#include "api_setup.inc"
#include "api_operators.inc"
// the resident iteration: stages over all sets, the sharded exchange, one iteration, the pipelined run, the proximal rule
#include "ngd_stage.inc"
#include "ngd_dist.inc"
#include "ngd_iter.inc"
#include "ngd_run.inc"
#include "prox.inc"
// transports of the exchange; counters, read-back, profiles, options
#include "dist_transport.inc"
#include "api_inspect.inc"

}  // extern "C"

// posterior queries: samples and log-density, many right-hand sides, dense-time posterior, costs of sampled trajectories
// (textually part of this translation unit: the kernel headers define __global__ functions and cannot be included twice)
#include "posterior_host.inc"
