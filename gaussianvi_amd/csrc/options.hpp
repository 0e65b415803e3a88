// The run-time switches of a context (gvi_ctx::opt): ONE struct with the defaults and ONE table that says, per switch, under
// which name gvi_set_option takes it, which environment variable gvi_ctx_create reads for it, and how a value is applied.  A
// new switch is a field and a row; include/gvi_hip.h and DESIGN.md section 4.5 describe the rows (tests/test_options_host.py
// compares the header's list with this table).  Plain C++17, no HIP.
//
// Not here, because they are no options of a context: GVI_SPGH_EXTENDED (table generation, spgh.cpp), GVI_RCCL_PATH (read
// when librccl is loaded), GVI_FUSED_DBG (timing builds only).
#pragma once
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <string>

namespace gvi {

struct Options {
  bool warm_start = true;             // resident NGD: Jacobi warm start from the previous eigenvectors
  // gvi_ngd_step: trial cost from the full moments pass at the trial point (one psi pass per accepted iteration).
  // 0 never, 1 always (first trial), 2 adaptive (default): fused while first trials keep being accepted, the m0-only
  // cost pass after a rejection (a rejected fused trial wastes the moment accumulation).  gvi_ngd_set_mode writes it too.
  int fuse_trial = 2;
  int target_waves = 2048;            // waves the lane-per-point kernels aim for over one set
  bool mirror = true;                 // 0: never pair z with -z (A/B; results agree to rounding)
  int split_flush = 64;               // (SPLIT_FLUSH of kernels_split.hpp) 0: plain recursive sums in the split kernel (A/B of the (24,7) rounding)
  bool sreg_pipe = true;              // 0: full pass on the compiler-scheduled body (A/B; bit-identical results)
  bool no_scost = false;              // 1: cost pass on the one-factor-per-wave kernel (A/B)
  // sum-of-squares sets on the sign-orbit kernel (kernels_orbit.hpp) when the table decomposes; 0: the lane-per-point
  // kernels (A/B; results agree to rounding)
  bool orbit = true;
  // full moments pass of the resident iteration as ONE launch (kernels_fused.hpp) where every set runs the sign-orbit kernel;
  // 0: the three-launch route prep -> psi -> epilogue (A/B; same numbers at four chunks per factor)
  bool fused = true;
  int orbit_waves = 4096;             // waves the orbit launch of one set aims for (chunks = orbit_waves / K, <= tiles)
  // prep: cyclic Jacobi stops when (sum of squared off-diagonals) <= jacobi_tol * (sum of squared diagonals); option
  // "jacobi_tol_exp" sets 10^value.  The threshold compares SQUARED off-diagonal mass with squared diagonal mass: anything
  // looser than 1e-20 (1e-10 relative) would break the 1e-9 operator parity, so it is refused rather than silently clamped
  double jacobi_tol = 1e-34;
  // sum-of-squares sets: per-pass products from the Cholesky factor of the marginal instead of its symmetric square root
  // (same moments -- the quadrature is exact there -- without the Jacobi sweeps)
  bool chol_sqrt = true;
  // the register Cholesky of the three-launch route's prep (prep_all_kernel) in its row-broadcast form (kernels_prep.hpp,
  // prep_chol_body<DT, ROWB>) instead of v_readlane; bit-identical (A/B inside one library), and slower in that launch
  // (profiles/r06_unit_top.txt section 4), hence off.  The fused pass takes the row-broadcast form unconditionally.
  bool chol_rowb = false;
  // a table handed to gvi_factors_add_table IS the Smolyak rule of the degree it is added under (e.g. the generator's own
  // table, produced once and broadcast to the other ranks); it may then take every route the generated table takes (Cholesky
  // factor for sum-of-squares psi).  Default 0: a caller's table keeps the symmetric root, as the reference maps the nodes.
  bool trust_table_degree = false;
  int orbit_min_tiles = 6;            // tiles a wave of the orbit launch walks at least (its prologue and reduction cost about two)
  int orbit_copies = 8;               // private LDS copies of the accumulators (1, 2, 4, 8, 16; fewer when LDS is short)
  bool pair_fuse = true;              // GVI_NO_PAIR=1: one launch per set
  bool fuse_gather = true;            // GVI_NO_FUSE_GATHER=1: stand-alone gather launch before the trial's prep
  // the chain solve of the gradients goes out beside the next trial factorisation (independent given Vddmu), as one dual
  // launch (dual_solve, NgdBook::solve_deferred); 0, or a one-state chain: the solve is launched at once
  bool side_solve = true;
  // assemble-on-load (0: the stand-alone assemble launch): on chain-structured graphs the ordered assemble of (g, V_D, V_U)
  // is not launched behind the factor pass but done by the first pass of the chain operations that consume it
  // (kernels_chain.hpp, AsmList; NgdBook::asm_pending)
  bool asm_on_load = true;
  // A/B legs of the chain kernels (chain_plan.hpp::ChainRules): 0 keeps short chains of 2 x 2 blocks (T <= 65, n <= 2) on the
  // generic kernels instead of the lane-per-node kernel / an assemble-on-load on the generic set loop instead of the batched
  // first-pass load / the N = 6 eliminations of every pass on the v_readlane kernels instead of the two-row form
  bool chain_wave = true;
  bool asm_dense = true;
  bool chain_pair = true;
  bool chain_merge = true;            // top pass + first backward pass of the chain in one launch (chain_launch.hpp::ChainSync)
  bool chain_merge_fault = false;     // option chain_merge = 2 only: the hand-over word is stored wrong (test of the bounded wait)
  // gvi_ngd_run queues iteration i + 1 (predicated) before it has read the cost of iteration i.  Round 2 measured no gain
  // (129.7 vs 130.5 us per C3 iteration: the early publish of the trial cost already gave the host its head start); with
  // the round-3 kernels the iteration is short enough for the host's hand-over to show again: 109.3 -> 107.4 us at C3,
  // 45.8 -> 44.3 us at C2.  On by default since then.
  bool pipeline = true;
  int spin_ms = 2;                    // wall-time bound of the host spin on the publish word
  bool safe_publish = false;          // checked publish + release / acquire arrival counters (device_common.hpp)
  bool sample_sweep = true;           // 0: the samplers and the multi-solve run the factorisation only (tools/*_bench.py)
  bool solve_lds = true;              // 0: the multi-solve sweep keeps its vectors in the output buffer whatever the size
  // fused factor pass: a walking wave sets its priority from the share of its modelled walk cost still ahead of it
  // (walk_prio.hpp), where the launch's item blocks fit one residency round; bit-identical (A/B inside one library)
  bool walk_prio = true;
};

// how a row applies an integer value v
enum OptionRule {
  OPT_FLAG,        // field = v != 0
  OPT_FLAG_INV,    // field = v == 0 (GVI_NO_*)
  OPT_MIN,         // field = max(lo, v)
  OPT_CLAMP,       // field = min(hi, max(lo, v))
  OPT_POW10_MAX    // field = 10^v; v > hi is refused
};

struct OptionRow {
  const char* name;              // gvi_set_option name, or null: environment only
  const char* env;               // environment variable read at gvi_ctx_create, or null: option only
  OptionRule rule;
  int lo, hi;
  bool Options::*flag;           // the field: exactly one of these three is set
  int Options::*num;
  double Options::*real;
};

constexpr OptionRow opt_flag(const char* name, const char* env, bool Options::*f) { return {name, env, OPT_FLAG, 0, 0, f, nullptr, nullptr}; }
constexpr OptionRow opt_flag_inv(const char* name, const char* env, bool Options::*f) { return {name, env, OPT_FLAG_INV, 0, 0, f, nullptr, nullptr}; }
constexpr OptionRow opt_min(const char* name, const char* env, int Options::*f, int lo) { return {name, env, OPT_MIN, lo, 0, nullptr, f, nullptr}; }
constexpr OptionRow opt_clamp(const char* name, const char* env, int Options::*f, int lo, int hi) { return {name, env, OPT_CLAMP, lo, hi, nullptr, f, nullptr}; }
constexpr OptionRow opt_pow10(const char* name, double Options::*f, int hi) { return {name, nullptr, OPT_POW10_MAX, 0, hi, nullptr, nullptr, f}; }

// A name with two rows (pair_fuse, fuse_gather) has its option under the plain sense and its environment variable inverted.
constexpr OptionRow OPTION_ROWS[] = {
  opt_flag("orbit", "GVI_ORBIT", &Options::orbit),
  opt_flag("fused", "GVI_FUSED", &Options::fused),
  opt_flag("assemble_on_load", "GVI_ASM_ON_LOAD", &Options::asm_on_load),
  opt_flag("pipeline", "GVI_PIPELINE", &Options::pipeline),
  opt_flag("chain_wave", "GVI_CHAIN_WAVE", &Options::chain_wave),          // A/B leg of kernels_chain_wave.hpp
  opt_flag("asm_dense", "GVI_ASM_DENSE", &Options::asm_dense),             // A/B leg of the batched first-pass load
  opt_flag("chain_pair", "GVI_CHAIN_PAIR", &Options::chain_pair),          // A/B leg of the row-broadcast eliminations
  opt_flag("chain_merge", "GVI_CHAIN_MERGE", &Options::chain_merge),       // (option value 2: gvi_set_option sets chain_merge_fault)
  opt_flag("chol_rowb", "GVI_CHOL_ROWB", &Options::chol_rowb),
  opt_clamp(nullptr, "GVI_FUSE_TRIAL", &Options::fuse_trial, 0, 2),
  opt_flag("side_solve", "GVI_SIDE_SOLVE", &Options::side_solve),
  opt_flag("pair_fuse", nullptr, &Options::pair_fuse),
  opt_flag_inv(nullptr, "GVI_NO_PAIR", &Options::pair_fuse),
  opt_flag("fuse_gather", nullptr, &Options::fuse_gather),
  opt_flag_inv(nullptr, "GVI_NO_FUSE_GATHER", &Options::fuse_gather),
  opt_flag("no_scost", "GVI_NO_SCOST", &Options::no_scost),
  opt_flag("sreg_pipe", "GVI_SREG_PIPE", &Options::sreg_pipe),
  opt_flag("mirror", "GVI_MIRROR", &Options::mirror),
  opt_flag("safe_publish", "GVI_SAFE_PUBLISH", &Options::safe_publish),    // (option: gvi_set_option drains the stream and resets the slot)
  opt_min(nullptr, "GVI_SPIN_MS", &Options::spin_ms, 0),
  opt_flag("chol_sqrt", nullptr, &Options::chol_sqrt),
  opt_flag("sample_sweep", nullptr, &Options::sample_sweep),
  opt_flag("solve_lds", nullptr, &Options::solve_lds),
  opt_flag("trust_table_degree", nullptr, &Options::trust_table_degree),
  opt_pow10("jacobi_tol_exp", &Options::jacobi_tol, -20),
  opt_min("split_flush", nullptr, &Options::split_flush, 0),
  opt_min("target_waves", nullptr, &Options::target_waves, 1),
  opt_min("orbit_waves", nullptr, &Options::orbit_waves, 1),
  opt_min("orbit_min_tiles", nullptr, &Options::orbit_min_tiles, 1),
  opt_clamp("orbit_copies", nullptr, &Options::orbit_copies, 1, 16),
  opt_flag("warm_start", nullptr, &Options::warm_start),
};
// Rows of the same kind, applied the same way, kept apart: tests/test_options_host.py holds the names and the environment
// variables of OPTION_ROWS as closed lists, so a switch that joins later stands here and is checked by a host test of its own
// (walk_prio: tests/test_walk_prio_host.py).  include/gvi_hip.h lists these rows under the table of OPTION_ROWS.
constexpr OptionRow OPTION_ROWS_LATER[] = {
  opt_flag("walk_prio", "GVI_WALK_PRIO", &Options::walk_prio),
};

// false and a text in *msg where the rule refuses the value
inline bool option_apply(Options& o, const OptionRow& r, int v, std::string* msg) {
  switch (r.rule) {
    case OPT_FLAG:
    case OPT_FLAG_INV: o.*r.flag = r.rule == OPT_FLAG ? v != 0 : v == 0; break;
    case OPT_MIN: o.*r.num = v > r.lo ? v : r.lo; break;
    case OPT_CLAMP: o.*r.num = v < r.lo ? r.lo : v > r.hi ? r.hi : v; break;
    case OPT_POW10_MAX:
      if (v > r.hi) {
        if (msg) *msg = std::string(r.name) + " must be <= " + std::to_string(r.hi) + " (threshold 10^value on squared magnitudes)";
        return false;
      }
      o.*r.real = pow(10.0, (double)v);
      break;
  }
  return true;
}

// gvi_ctx_create: every row with an environment name whose variable `lookup` finds (getenv, or a test's own function)
template <class Lookup>
void options_from_env(Options& o, Lookup&& lookup) {
  const auto read = [&](const OptionRow& r) {
    if (r.env)
      if (const char* w = lookup(r.env)) option_apply(o, r, atoi(w), nullptr);
  };
  for (const OptionRow& r : OPTION_ROWS) read(r);
  for (const OptionRow& r : OPTION_ROWS_LATER) read(r);
}

// gvi_set_option: the row named `name`; false and the text of the refusal in *msg
inline bool option_set(Options& o, const char* name, int value, std::string* msg) {
  for (const OptionRow& r : OPTION_ROWS)
    if (r.name && strcmp(r.name, name) == 0) return option_apply(o, r, value, msg);
  for (const OptionRow& r : OPTION_ROWS_LATER)
    if (r.name && strcmp(r.name, name) == 0) return option_apply(o, r, value, msg);
  *msg = std::string("unknown option: ") + name;
  return false;
}

}  // namespace gvi
