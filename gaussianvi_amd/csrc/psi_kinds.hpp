// The psi kinds of GVI_PSI_* (include/gvi_hip.h): ONE table, one row per kind, with everything the host code needs to know
// about a kind -- its operand rows m, the size of its parameter block, the condition on the factor dimension and what it
// keeps, reads and offers.  gvi_factors_add lays a set out with psi_kind_layout and checks the values of its parameter
// blocks with psi_kind_check_params; every other site asks psi_kind_is.  A new kind is one row here, its psi_* function in
// psi_point.hpp (psi_point) and, where it has compiled instances, a line in the with_*_instance lists of routes.hpp.
// Plain C++17 that also compiles without HIP (tests/stubs/psi_kinds_check.cpp runs it under AddressSanitizer / UBSan).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/gvi_hip.h"
#include "hd.hpp"

namespace gvi {

enum { KIND_RANGE_1D = GVI_PSI_RANGE_1D, KIND_QUAD_PRIOR = GVI_PSI_QUAD_PRIOR, KIND_FIXED_PRIOR = GVI_PSI_FIXED_PRIOR,
       KIND_HOST_CALLBACK = GVI_PSI_HOST_CALLBACK, KIND_HINGE_SDF_2D = GVI_PSI_HINGE_SDF_2D,
       KIND_HINGE_SDF_2D_BODY = GVI_PSI_HINGE_SDF_2D_BODY, KIND_HINGE_SDF_3D = GVI_PSI_HINGE_SDF_3D,
       KIND_HINGE_SDF_3D_ARM = GVI_PSI_HINGE_SDF_3D_ARM, KIND_HINGE_SDF_2D_SEG = GVI_PSI_HINGE_SDF_2D_SEG,
       KIND_HINGE_SDF_3D_SEG = GVI_PSI_HINGE_SDF_3D_SEG, KIND_HINGE_BOX = GVI_PSI_HINGE_BOX,
       KIND_HINGE_HALFSPACE = GVI_PSI_HINGE_HALFSPACE, KIND_HINGE_BALLS_2D = GVI_PSI_HINGE_BALLS_2D,
       KIND_HINGE_BALLS_3D = GVI_PSI_HINGE_BALLS_3D, KIND_COUNT = 15 };
// 12 is a hole: the host tests of this table and of routes.hpp pin it as the first number that is NO kind, so it stays unassigned
constexpr int KIND_HOLE = 12;

constexpr int SEG_MAX_J = GVI_SEG_MAX_J;               // check points of one HINGE_SDF_*_SEG factor
constexpr int HALFSPACE_MAX_J = GVI_HALFSPACE_MAX_J;   // rows of one HINGE_HALFSPACE factor
constexpr int BALLS_MAX_M = GVI_BALLS_MAX_M;           // ball slots of one HINGE_BALLS_* factor (its check points: SEG_MAX_J)
static_assert(SEG_MAX_J == 8 && HALFSPACE_MAX_J == 16 && BALLS_MAX_M == 8, "the refusal texts of psi_kind_layout spell the limits out");

// what a kind keeps, reads and offers
enum : unsigned {
  PSI_RAW = 1u << 0,              // the set keeps the raw parameter block on the device (FactorDev::raw); psi_point evaluates it
  PSI_SDF_2D = 1u << 1,           // psi reads a 2-D signed-distance grid (gvi_factors_set_sdf2d)
  PSI_SDF_3D = 1u << 2,           // psi reads a 3-D signed-distance grid (gvi_factors_set_sdf3d)
  PSI_ARM = 1u << 3,              // psi needs an arm model (gvi_factors_set_arm)
  PSI_CLEARANCE = 1u << 4,        // has a clearance (hinge_psi_clearance): distance to the obstacle, margin to the limits
  PSI_CLOSED = 1u << 5,           // has quadrature-free moments (gvi_factors_set_closed_form) ...
  PSI_CLOSED_DEFAULT = 1u << 6,   // ... and takes them by default: exact and cheaper than any rule on the kink
  PSI_SUMSQ = 1u << 7,            // sum of squares of m linear forms: operands (A, b, sgn) built at gvi_factors_add
  PSI_NO_DEVICE = 1u << 8,        // the host evaluates psi (gvi_expand + gvi_moments_from_psi)
  PSI_READOUT = 1u << 9,          // psi = sum_j f_j(W_j x + c_j) on P-dimensional linear read-outs (psi_kind_readout_P): offers the
                                  // read-out-space rule (gvi_factors_set_readout_rule; readout_moments.hpp)
  PSI_SDF = PSI_SDF_2D | PSI_SDF_3D
};

// how a PSI_READOUT kind lays its read-outs out (ReadoutView, readout_view.hpp): the first P coordinates of the slice (HINGE_SDF_2D / _3D),
// [W_j | c_j] blocks (the _SEG kinds), [W_j | c_j | tau_j] blocks and ball slots (HINGE_BALLS_*)
enum { READOUT_NONE = -1, READOUT_LEAD = 0, READOUT_SEG = 1, READOUT_BALLS = 2 };

// m: operand rows of the sum-of-squares form.  need: doubles of one factor's parameter block.
enum PsiRows { M_NONE, M_HALF_D, M_D };
enum PsiNeed {
  NEED_FIXED,       // `arg` doubles; a caller's stride may be longer
  NEED_QUAD,        // [Phi (m x m) | Qinv (m x m)]: 2 m^2
  NEED_MEAN_QUAD,   // [mu0 (d) | Qinv (d x d)]: d + d^2
  NEED_SEG,         // exactly 3 + J P (d + 1), P = `ro_P`, 1 <= J <= SEG_MAX_J: J is a property of the set
  NEED_BOX,         // exactly 4 d: [sigma | eps | lo | hi]
  NEED_HALFSPACE,   // exactly J (d + 3), 1 <= J <= HALFSPACE_MAX_J: J is a property of the set
  NEED_BALLS        // exactly 3 + J (P (d + 1) + 1) + BALLS_MAX_M (2 P + 1), P = `ro_P`, 1 <= J <= SEG_MAX_J: J is a property of the set
};
enum PsiDim { D_ANY, D_ONE, D_EVEN, D_MIN };   // D_MIN: d >= `dmin`

struct PsiKindRow {
  int kind;
  unsigned flags;
  PsiRows rows;
  PsiNeed need;
  int arg;
  PsiDim dim;
  int dmin;
  const char* dim_msg;
  int ro_P;     // dimension of the kind's read-outs (2: the planar grid / planar balls, 3: the 3-D field / balls); 0: no read-out
  int ro_cls;   // READOUT_*
  int lead;     // leading coordinates of the slice that the kind's point psi reads (the pose, the joint angles); 0: not a leading slice
};

constexpr PsiKindRow PSI_KINDS[KIND_COUNT] = {
  {KIND_RANGE_1D, PSI_RAW, M_NONE, NEED_FIXED, 5, D_ONE, 0, "RANGE_1D needs d == 1", 0, READOUT_NONE, 1},
  {KIND_QUAD_PRIOR, PSI_SUMSQ | PSI_CLOSED, M_HALF_D, NEED_QUAD, 0, D_EVEN, 0, "QUAD_PRIOR needs even d", 0, READOUT_NONE, 0},
  {KIND_FIXED_PRIOR, PSI_SUMSQ | PSI_CLOSED, M_D, NEED_MEAN_QUAD, 0, D_ANY, 0, nullptr, 0, READOUT_NONE, 0},
  {KIND_HOST_CALLBACK, PSI_NO_DEVICE, M_NONE, NEED_FIXED, 0, D_ANY, 0, nullptr, 0, READOUT_NONE, 0},
  {KIND_HINGE_SDF_2D, PSI_RAW | PSI_SDF_2D | PSI_CLEARANCE | PSI_READOUT, M_NONE, NEED_FIXED, 3, D_MIN, 2, "HINGE_SDF_2D needs d >= 2", 2, READOUT_LEAD, 2},
  {KIND_HINGE_SDF_2D_BODY, PSI_RAW | PSI_SDF_2D | PSI_CLEARANCE, M_NONE, NEED_FIXED, 6, D_MIN, 3, "HINGE_SDF_2D_BODY needs d >= 3", 0, READOUT_NONE, 3},
  {KIND_HINGE_SDF_3D, PSI_RAW | PSI_SDF_3D | PSI_CLEARANCE | PSI_READOUT, M_NONE, NEED_FIXED, 3, D_MIN, 3, "HINGE_SDF_3D needs d >= 3", 3, READOUT_LEAD, 3},
  {KIND_HINGE_SDF_3D_ARM, PSI_RAW | PSI_SDF_3D | PSI_ARM | PSI_CLEARANCE, M_NONE, NEED_FIXED, 2, D_ANY, 0, nullptr, 0, READOUT_NONE, 7},
  {KIND_HINGE_SDF_2D_SEG, PSI_RAW | PSI_SDF_2D | PSI_CLEARANCE | PSI_READOUT, M_NONE, NEED_SEG, 0, D_ANY, 0, nullptr, 2, READOUT_SEG, 0},
  {KIND_HINGE_SDF_3D_SEG, PSI_RAW | PSI_SDF_3D | PSI_CLEARANCE | PSI_READOUT, M_NONE, NEED_SEG, 0, D_ANY, 0, nullptr, 3, READOUT_SEG, 0},
  {KIND_HINGE_BOX, PSI_RAW | PSI_CLEARANCE | PSI_CLOSED | PSI_CLOSED_DEFAULT, M_NONE, NEED_BOX, 0, D_ANY, 0, nullptr, 0, READOUT_NONE, 0},
  {KIND_HINGE_HALFSPACE, PSI_RAW | PSI_CLEARANCE | PSI_CLOSED | PSI_CLOSED_DEFAULT, M_NONE, NEED_HALFSPACE, 0, D_ANY, 0, nullptr, 0, READOUT_NONE, 0},
  {KIND_HOLE, 0, M_NONE, NEED_FIXED, 0, D_ANY, 0, nullptr, 0, READOUT_NONE, 0},
  {KIND_HINGE_BALLS_2D, PSI_RAW | PSI_CLEARANCE | PSI_READOUT, M_NONE, NEED_BALLS, 0, D_ANY, 0, nullptr, 2, READOUT_BALLS, 0},
  {KIND_HINGE_BALLS_3D, PSI_RAW | PSI_CLEARANCE | PSI_READOUT, M_NONE, NEED_BALLS, 0, D_ANY, 0, nullptr, 3, READOUT_BALLS, 0},
};
constexpr bool psi_kind_known(int kind) { return kind >= 0 && kind < KIND_COUNT && kind != KIND_HOLE; }

constexpr bool psi_kinds_in_order() {
  for (int i = 0; i < KIND_COUNT; ++i)
    if (PSI_KINDS[i].kind != i) return false;
  return true;
}
static_assert(psi_kinds_in_order(), "row i of PSI_KINDS describes kind i");

// bit k set: kind k has one of `flags`
constexpr unsigned psi_kind_mask(unsigned flags) {
  unsigned mask = 0;
  for (int i = 0; i < KIND_COUNT; ++i)
    if (PSI_KINDS[i].flags & flags) mask |= 1u << i;
  return mask;
}

// Does `kind` have (one of) FLAGS?  The table folds into one word at compile time, so a kernel pays a shift and a test
// (sample_cost_kernel asks per block); false for a number that is no kind.
template <unsigned FLAGS>
GVI_HD constexpr bool psi_kind_is(int kind) {
  constexpr unsigned mask = psi_kind_mask(FLAGS);
  return kind >= 0 && kind < KIND_COUNT && ((mask >> kind) & 1u) != 0;
}

// P of a PSI_READOUT kind: the dimension of its read-outs (2: the planar grid / planar balls, 3: the 3-D field / balls); 0 for
// every other kind
GVI_HD constexpr int psi_kind_readout_P(int kind) { return psi_kind_known(kind) ? PSI_KINDS[kind].ro_P : 0; }
// the leading coordinates of the slice that the kind's point psi reads (RANGE_1D, the hinges on a pose, the arm); 0 for every other kind
GVI_HD constexpr int psi_kind_lead(int kind) { return psi_kind_known(kind) ? PSI_KINDS[kind].lead : 0; }

// doubles of one check point in a factor's block (SEG [W_j | c_j], BALLS [W_j | c_j | tau_j]; LEAD has none: its ONE read-out is the
// first P coordinates of the slice) and the check points of a factor whose set has seg_J of them; ReadoutView reads a block with these
constexpr int readout_stride(int cls, int P, int d) { return cls == READOUT_BALLS ? P * (d + 1) + 1 : P * (d + 1); }
constexpr int readout_check_points(int cls, int seg_J) { return cls == READOUT_LEAD ? 1 : seg_J; }

// Layout of a set of `kind` on factors of dimension d whose parameter blocks are params_per_factor doubles apart: operand
// rows m, check points / rows per factor J (0 for the kinds without), doubles `need` of a block.  GVI_ERR_ARG and the text
// in *msg where the kind, d or the block size is refused.
inline gvi_status psi_kind_layout(int kind, int d, int64_t params_per_factor, int* m, int* J, int64_t* need, const char** msg) {
  *m = 0; *J = 0; *need = 0; *msg = nullptr;
  if (!psi_kind_known(kind)) { *msg = "unknown psi kind"; return GVI_ERR_ARG; }
  const PsiKindRow& r = PSI_KINDS[kind];
  if ((r.dim == D_ONE && d != 1) || (r.dim == D_EVEN && d % 2 != 0) || (r.dim == D_MIN && d < r.dmin)) { *msg = r.dim_msg; return GVI_ERR_ARG; }
  *m = r.rows == M_HALF_D ? d / 2 : r.rows == M_D ? d : 0;
  switch (r.need) {
    case NEED_FIXED: *need = r.arg; break;
    case NEED_QUAD: *need = 2 * (int64_t)*m * *m; break;
    case NEED_MEAN_QUAD: *need = d + (int64_t)d * d; break;
    case NEED_SEG: {
      const int64_t per = readout_stride(r.ro_cls, r.ro_P, d), body = params_per_factor - 3;
      if (body < per || body % per != 0 || body / per > SEG_MAX_J) {
        *msg = "HINGE_SDF_*_SEG needs params_per_factor = 3 + J P (d + 1) with 1 <= J <= 8 check points "
               "(P = 2 for _2D_SEG, 3 for _3D_SEG)";
        return GVI_ERR_ARG;
      }
      *J = (int)(body / per);
      *need = params_per_factor;
      break;
    }
    case NEED_BOX:
      if (params_per_factor != 4 * (int64_t)d) { *msg = "HINGE_BOX needs params_per_factor = 4 d: [sigma | eps | lo | hi]"; return GVI_ERR_ARG; }
      *need = params_per_factor;
      break;
    case NEED_HALFSPACE: {
      const int64_t per = (int64_t)d + 3;
      if (params_per_factor < per || params_per_factor % per != 0 || params_per_factor / per > HALFSPACE_MAX_J) {
        *msg = "HINGE_HALFSPACE needs params_per_factor = J (d + 3) with 1 <= J <= 16 rows: [sigma (J) | eps (J) | b (J) | A (J x d)]";
        return GVI_ERR_ARG;
      }
      *J = (int)(params_per_factor / per);
      *need = params_per_factor;
      break;
    }
    case NEED_BALLS: {
      const int64_t per = readout_stride(r.ro_cls, r.ro_P, d), body = params_per_factor - 3 - BALLS_MAX_M * (2 * (int64_t)r.ro_P + 1);
      if (body < per || body % per != 0 || body / per > SEG_MAX_J) {
        *msg = "HINGE_BALLS_* needs params_per_factor = 3 + J (P (d + 1) + 1) + 8 (2 P + 1) with 1 <= J <= 8 check points "
               "(P = 2 for _2D, 3 for _3D)";
        return GVI_ERR_ARG;
      }
      *J = (int)(body / per);
      *need = params_per_factor;
      break;
    }
  }
  if (params_per_factor < *need) { *msg = "psi_params missing or params_per_factor too small for this kind"; return GVI_ERR_ARG; }
  return GVI_OK;
}

// The values of the K parameter blocks of a set that psi_kind_layout accepted (J from there): the blocks are there, and the
// limit kinds hold numbers their closed forms and kernels can take.
inline gvi_status psi_kind_check_params(int kind, int d, int J, int64_t params_per_factor, int64_t K, const double* params, const char** msg) {
  *msg = nullptr;
  auto refuse = [&](const char* text) -> gvi_status { *msg = text; return GVI_ERR_ARG; };
  if (!psi_kind_known(kind)) return refuse("unknown psi kind");
  const PsiNeed need = PSI_KINDS[kind].need;
  if (!params && !(need == NEED_FIXED && PSI_KINDS[kind].arg == 0)) return refuse("psi_params missing or params_per_factor too small for this kind");
  if (need == NEED_BOX) {
    for (int64_t k = 0; k < K; ++k) {
      const double* P = params + k * params_per_factor;
      for (int i = 0; i < d; ++i) {
        const double sg = P[i], ep = P[d + i], lo = P[2 * d + i], hi = P[3 * d + i];
        if (!isfinite(sg) || sg < 0.0) return refuse("HINGE_BOX: sigma must be finite and >= 0");
        if (!isfinite(ep)) return refuse("HINGE_BOX: eps must be finite");
        if (isnan(lo) || isnan(hi)) return refuse("HINGE_BOX: NaN limit");
        if (!(lo < hi)) return refuse("HINGE_BOX: lo must be below hi (lo = -inf / hi = +inf switch a side off)");
      }
    }
  }
  if (need == NEED_HALFSPACE) {
    for (int64_t k = 0; k < K; ++k) {
      const double* P = params + k * params_per_factor;
      for (int64_t e = 0; e < params_per_factor; ++e)
        if (isnan(P[e])) return refuse("HINGE_HALFSPACE: NaN in the parameter block");
      for (int j = 0; j < J; ++j) {
        if (!isfinite(P[j]) || P[j] < 0.0) return refuse("HINGE_HALFSPACE: sigma must be finite and >= 0");
        if (!isfinite(P[J + j])) return refuse("HINGE_HALFSPACE: eps must be finite");
        if (!isfinite(P[2 * J + j])) return refuse("HINGE_HALFSPACE: b must be finite");
        bool zero = true;
        for (int i = 0; i < d; ++i) {
          const double v = P[3 * J + (int64_t)j * d + i];
          if (!isfinite(v)) return refuse("HINGE_HALFSPACE: A must be finite");
          zero = zero && v == 0.0;
        }
        if (zero && P[j] > 0.0) return refuse("HINGE_HALFSPACE: an active row (sigma > 0) needs a non-zero normal a_j");
      }
    }
  }
  if (need == NEED_BALLS) {
    const int P = PSI_KINDS[kind].ro_P;
    const int64_t per = readout_stride(READOUT_BALLS, P, d), slot = 2 * (int64_t)P + 1;
    for (int64_t k = 0; k < K; ++k) {
      const double* B = params + k * params_per_factor;
      for (int64_t e = 0; e < params_per_factor; ++e)
        if (isnan(B[e])) return refuse("HINGE_BALLS: NaN in the parameter block");
      if (!isfinite(B[0]) || B[0] < 0.0) return refuse("HINGE_BALLS: sigma must be finite and >= 0");
      if (!isfinite(B[1]) || !isfinite(B[2])) return refuse("HINGE_BALLS: eps and r must be finite");
      for (int64_t e = 3; e < 3 + J * per; ++e)
        if (!isfinite(B[e])) return refuse("HINGE_BALLS: W, c and tau must be finite");
      const double* ball = B + 3 + J * per;
      for (int m = 0; m < BALLS_MAX_M; ++m, ball += slot) {
        const double R = ball[2 * P];
        if (R == -INFINITY) continue;             // an empty slot: never evaluated
        if (!isfinite(R) || R < 0.0) return refuse("HINGE_BALLS: a radius is finite and >= 0, or -inf for an empty slot");
        for (int e = 0; e < 2 * P; ++e)
          if (!isfinite(ball[e])) return refuse("HINGE_BALLS: a ball needs a finite centre and velocity");
      }
    }
  }
  return GVI_OK;
}

}  // namespace gvi
