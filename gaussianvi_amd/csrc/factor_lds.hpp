// The dynamic LDS of the factor stage: where every kernel of the stage headers (kernels_factor.hpp lists them), kernels_fused.hpp and kernels_block.hpp that
// carves its LDS by hand puts its regions, and how many bytes its launch asks for.  A layout is a small value whose members are
// offsets in doubles, each written as the region before it plus that region's length.  The kernel takes its pointers from the
// layout and the launch its size, so a kernel's idea of its LDS and its launch's cannot drift apart.
// A kernel with a run-time d steps from region to region -- double* Sg = M + (L.Sg() - L.M()) -- where sm + L.Sg() would do:
// a difference of neighbours folds to the region's length, and the compiler keeps a chain of pointer steps as written, which is
// the address arithmetic these kernels were tuned with (the short chains compile to the same code as a hand-written chain, the
// long ones of prep_body and moments_generic_kernel get re-associated: profiles/factor_lds_refactor.txt, section 2).
// An LDS access past the allocation raises no fault on this part -- it shows as wrong numbers, if at all -- hence the
// static_asserts at the end: regions ascending without overlap, every view inside its area, for d = 1 .. 32.  Every offset is a
// whole number of doubles, so double regions start on 8 bytes and the int regions too.
// tests/test_factor_lds_host.py runs the header on the CPU (tests/stubs/factor_lds_check.cpp, plain and sanitized builds) against
// an independent model.  Plain C++17, no HIP, no heap.
// No size here may change without a measurement: LDS per workgroup decides occupancy.  Where a launch has always asked for more
// than its kernel touches, the surplus is a named term.
#pragma once
#include <stddef.h>

#include <initializer_list>

#include "factor_dev.hpp"
#include "hd.hpp"

namespace gvi {

constexpr int FACTOR_DMAX = 32;          // largest factor dimension of the prep and epilogue kernels

// ---- the products area: the per-pass products of ONE factor by one wave (prep_body, prep_chol_body, prep_chol_lds_body) ----
struct ProductsLds {
  int d;
  GVI_HD constexpr int dd() const { return d * d; }
  GVI_HD constexpr int dp() const { return d + (d & 1); }          // d rounded up to even: the rotation partners of the Jacobi sweep
  // Jacobi view (prep_body): A0 A1 V0 V1 [d][d] | al be [dp] | lam [3][d] (sqrt, 1/sqrt, 1/x of lambda) | pa (int[dp])
  GVI_HD constexpr int A0() const { return 0; }
  GVI_HD constexpr int A1() const { return A0() + dd(); }
  GVI_HD constexpr int V0() const { return A1() + dd(); }
  GVI_HD constexpr int V1() const { return V0() + dd(); }
  GVI_HD constexpr int al() const { return V1() + dd(); }
  GVI_HD constexpr int be() const { return al() + dp(); }
  GVI_HD constexpr int lam() const { return be() + dp(); }
  GVI_HD constexpr int pa() const { return lam() + 3 * d; }
  GVI_HD constexpr int jacobi_end() const { return pa() + (dp() + 1) / 2; }      // dp ints
  // Cholesky view of the same area (prep_chol_body; prep_chol_lds_body uses Ll and Xl): Ll Xl [d][d] | Al [m][d], the rows of A
  // parked for u0 = b + A mu (only where m d <= 128)
  GVI_HD constexpr int Ll() const { return 0; }
  GVI_HD constexpr int Xl() const { return Ll() + dd(); }
  GVI_HD constexpr int Al() const { return Xl() + dd(); }
  GVI_HD constexpr int chol_end(int m) const { return Al() + m * d; }
  // the area: as the launches have always sized it, 4 * dd + 2 * dp + 3 * d + (dp + 1) / 2 -- the Jacobi view, the larger of
  // the two for every m <= d (the static_asserts below state the maximum)
  GVI_HD constexpr int doubles() const { return 4 * dd() + 2 * dp() + 3 * d + (dp() + 1) / 2; }
  // gather staging behind the area (prep_all_kernel, factor_fused_kernel, block_products): the factor's marginal pulled out of
  // the chain arrays, Sl [d][d] | ml [d], the inputs of the products
  static constexpr int STAGE_GAP = 1;    // one double between pa and Sl; nothing reads it
  GVI_HD constexpr int Sl() const { return doubles() + STAGE_GAP; }
  GVI_HD constexpr int ml() const { return Sl() + dd(); }
  GVI_HD constexpr int staged_end() const { return ml() + d; }
};

// two doubles (16 bytes) that every launch of the products asks for behind its last region; nothing reads them
constexpr int PRODUCTS_TAIL = 2;
// bytes of prep_kernel (one wave per factor, no staging) and of prep_all_kernel (staging, sized for the largest d of its sets)
GVI_HD constexpr size_t prep_lds_bytes(int d) { return (size_t)(ProductsLds{d}.doubles() + PRODUCTS_TAIL) * 8; }
GVI_HD constexpr size_t prep_all_lds_bytes(int dmax) { return (size_t)(ProductsLds{dmax}.staged_end() + PRODUCTS_TAIL) * 8; }

// ---- the epilogue area: packed moments Ms [npairs(d)] | M2 | one product Tm | the factor's Sinv and Lam staged once, [d][d]
// each (epilogue_body_t; Sv and Lv stay unused when the caller has S^-T in LDS already) ----
GVI_HD constexpr size_t epilogue_lds_doubles(int d) { return (size_t)npairs(d) + 4 * (size_t)d * d; }
struct EpilogueLds {
  int d;
  GVI_HD constexpr int dd() const { return d * d; }
  GVI_HD constexpr int Ms() const { return 0; }
  GVI_HD constexpr int M2() const { return Ms() + npairs(d); }
  GVI_HD constexpr int Tm() const { return M2() + dd(); }
  GVI_HD constexpr int Sv() const { return Tm() + dd(); }
  GVI_HD constexpr int Lv() const { return Tm() + 2 * dd(); }
  GVI_HD constexpr int end() const { return Lv() + dd(); }
  // behind the area: the tail's `last` word (an int) where a one-launch pass keeps it in LDS
  GVI_HD constexpr size_t last() const { return epilogue_lds_doubles(d); }
};
// epilogue_all_kernel at the largest d of its sets.  The 256 doubles behind the area held the 256-leaf tree of the tail's cost
// sum; epi_tail_arrive keeps the leaves in registers now and nothing reads them.
constexpr int EPILOGUE_ALL_TREE = 256;
GVI_HD constexpr size_t epilogue_all_tree(int dmax) { return epilogue_lds_doubles(dmax); }       // its position
GVI_HD constexpr size_t epilogue_all_lds_doubles(int dmax) { return epilogue_all_tree(dmax) + EPILOGUE_ALL_TREE; }

// ---- the item area of the one-launch passes (factor_fused_kernel, factor_block3_kernel): one wave's products phase (with
// staging) and, later, its epilogue phase in the same doubles; rounded to even so that the next wave's area starts on 16 bytes ----
constexpr int ITEM_LAST = 2;             // behind the epilogue view: the `last` word of the tail protocol (one int used)
// (the products side in size_t, term by term as the kernels have always computed it; the static_asserts hold it equal to the
// layout's staged_end() + PRODUCTS_TAIL)
GVI_HD constexpr size_t item_products_doubles(int d) {
  const size_t dd = (size_t)d * d, dp = d + (d & 1);
  return 4 * dd + 2 * dp + 3 * d + (dp + 1) / 2 + ProductsLds::STAGE_GAP + dd + d + PRODUCTS_TAIL;
}
GVI_HD constexpr size_t item_lds_doubles(int d) {
  const size_t prep = item_products_doubles(d);
  const size_t epi = epilogue_lds_doubles(d) + ITEM_LAST;
  return ((prep > epi ? prep : epi) + 1) & ~(size_t)1;
}
// per-wave region of the fused pass: the walk's LDS or the item area, whichever is larger, rounded to even
GVI_HD constexpr size_t fused_region_of(size_t walk_doubles, int dmax) {
  const size_t a = walk_doubles, b = item_lds_doubles(dmax);
  return ((a > b ? a : b) + 1) & ~(size_t)1;
}
// the helper wave of the fused pass (prep_chol_hu0) in its own region: Al [m][d] | mh [d], the item's mean
struct HelperLds {
  int d, m;
  GVI_HD constexpr size_t Al() const { return 0; }
  GVI_HD constexpr size_t mh() const { return (size_t)m * d; }
  GVI_HD constexpr size_t end() const { return mh() + d; }
};
// factor_block3_kernel: a wave's area at the largest d of its sets
constexpr int BLOCK3_DMAX = 8;
GVI_HD constexpr size_t block3_lds_doubles() { return item_lds_doubles(BLOCK3_DMAX); }

// ---- moments_generic_kernel, 256 threads: zs xs [256][d + 1] (z and the constant 1; x = mu + S z) | cs [256] | the factor's
// Ssh [d][d] | mush [d] | Ash [m][d] | bsh gsh [m] ----
constexpr int GEN_BS = 256;
constexpr size_t GENERIC_LDS_LIMIT = 160 * 1024;     // bytes; a larger (d, m) is refused
struct GenericLds {
  int d, m;
  GVI_HD constexpr int dz() const { return d + 1; }
  GVI_HD constexpr int zs() const { return 0; }
  GVI_HD constexpr int xs() const { return zs() + GEN_BS * dz(); }
  GVI_HD constexpr int cs() const { return xs() + GEN_BS * dz(); }
  GVI_HD constexpr int Ssh() const { return cs() + GEN_BS; }
  GVI_HD constexpr int mush() const { return Ssh() + d * d; }
  GVI_HD constexpr int Ash() const { return mush() + d; }
  GVI_HD constexpr int bsh() const { return Ash() + m * d; }
  GVI_HD constexpr int gsh() const { return bsh() + m; }
  GVI_HD constexpr int end() const { return gsh() + m; }
};
GVI_HD constexpr size_t generic_lds_bytes(int d, int m) { return (size_t)GenericLds{d, m}.end() * 8; }

// ---- jko_half_kernel: M = I - h S | Sg = Sigma | Tm = M Sigma, [d][d] each ----
struct JkoLds {
  int d;
  GVI_HD constexpr int dd() const { return d * d; }
  GVI_HD constexpr int M() const { return 0; }
  GVI_HD constexpr int Sg() const { return M() + dd(); }
  GVI_HD constexpr int Tm() const { return Sg() + dd(); }
  GVI_HD constexpr int end() const { return Tm() + dd(); }
};
GVI_HD constexpr size_t jko_half_lds_bytes(int d) { return (size_t)JkoLds{d}.end() * 8; }

// ---- kernels whose carve-up is a handful of fixed terms: the sizes alone ----
// moments_box_closed_kernel: Ss [d][d] | e1s e2s [d]
constexpr size_t BOX_CLOSED_LDS_LIMIT = 64 * 1024;   // bytes; a larger d is refused
GVI_HD constexpr size_t box_closed_lds_doubles(int d) { return (size_t)d * d + 2 * (size_t)d; }
// moments_halfspace_closed_kernel, per wave: Vs [d][64] | e1s e2s [64]
GVI_HD constexpr size_t halfspace_closed_lds_doubles(int d) { return 64 * (size_t)d + 128; }
// moments_split_kernel: lut [256] | hs (u0 | sgn) [2 D + 8] | px [2][4][64] | red [4][16][65] | lvl2 [4][2][SPLIT_LVL2_SLOTS]
constexpr int SPLIT_LVL2_SLOTS = 96;     // >= accumulators per wave (83 at D = 24)
constexpr int SPLIT_LDS_DOUBLES(int D) { return 256 + 2 * D + 8 + 2 * 4 * 64 + 4 * 16 * 65 + 4 * 2 * SPLIT_LVL2_SLOTS; }

// ---- the checks ----
namespace factor_lds_check {
// regions given as (start, end) pairs in layout order, the last value the size of what holds them: every region non-negative
// in length, starting at or behind the end of the one before it, the last one ending inside
constexpr bool ordered(std::initializer_list<int> bounds) {
  int prev = 0;
  for (int b : bounds) { if (b < prev) return false; prev = b; }
  return true;
}
constexpr bool products_ok(int d) {
  const ProductsLds L{d};
  const int dd = d * d, dp = L.dp(), area = L.doubles();
  return ordered({L.A0(), L.A0() + dd, L.A1(), L.A1() + dd, L.V0(), L.V0() + dd, L.V1(), L.V1() + dd, L.al(), L.al() + dp, L.be(), L.be() + dp,
                  L.lam(), L.lam() + 3 * d, L.pa(), L.pa() + (4 * dp + 7) / 8, L.jacobi_end(), area}) &&
         ordered({L.Ll(), L.Ll() + dd, L.Xl(), L.Xl() + dd, L.Al(), L.chol_end(d), area}) &&
         area == (L.jacobi_end() > L.chol_end(d) ? L.jacobi_end() : L.chol_end(d)) &&       // the area is the larger of its views
         ordered({area, L.Sl(), L.Sl() + dd, L.ml(), L.ml() + d, L.staged_end()}) &&
         prep_lds_bytes(d) >= (size_t)area * 8 && prep_all_lds_bytes(d) >= (size_t)L.staged_end() * 8;
}
constexpr bool epilogue_ok(int d) {
  const EpilogueLds E{d};
  const int dd = d * d, area = (int)epilogue_lds_doubles(d);
  return ordered({E.Ms(), E.Ms() + npairs(d), E.M2(), E.M2() + dd, E.Tm(), E.Tm() + dd, E.Sv(), E.Sv() + dd, E.Lv(), E.Lv() + dd, E.end(), area}) &&
         E.last() >= (size_t)E.end() && epilogue_all_tree(d) >= (size_t)E.end() &&
         epilogue_all_tree(d) + EPILOGUE_ALL_TREE <= epilogue_all_lds_doubles(d);
}
constexpr bool item_ok(int d) {
  const size_t item = item_lds_doubles(d);
  return item % 2 == 0 && item_products_doubles(d) == (size_t)(ProductsLds{d}.staged_end() + PRODUCTS_TAIL) && item_products_doubles(d) <= item && EpilogueLds{d}.last() * 8 + sizeof(int) <= item * 8;
}
constexpr bool generic_ok(int d, int m) {
  const GenericLds G{d, m};
  return ordered({G.zs(), G.zs() + GEN_BS * (d + 1), G.xs(), G.xs() + GEN_BS * (d + 1), G.cs(), G.cs() + GEN_BS, G.Ssh(), G.Ssh() + d * d,
                  G.mush(), G.mush() + d, G.Ash(), G.Ash() + m * d, G.bsh(), G.bsh() + m, G.gsh(), G.gsh() + m, G.end()}) &&
         generic_lds_bytes(d, m) >= (size_t)G.end() * 8;
}
constexpr bool helper_ok(int m, int dmax, size_t region) {       // the helper wave's view inside a region of the fused pass
  const HelperLds H{dmax, m};
  return H.Al() + (size_t)m * dmax <= H.mh() && H.mh() + dmax <= H.end() && H.end() <= region;
}
constexpr bool all_ok() {
  for (int d = 1; d <= FACTOR_DMAX; ++d) {
    const JkoLds K{d};
    if (!products_ok(d) || !epilogue_ok(d) || !item_ok(d)) return false;
    if (!ordered({K.M(), K.M() + d * d, K.Sg(), K.Sg() + d * d, K.Tm(), K.Tm() + d * d, K.end()}) || jko_half_lds_bytes(d) < (size_t)K.end() * 8) return false;
    for (int m = 0; m <= d; ++m)
      if (!generic_ok(d, m) || ProductsLds{d}.chol_end(m) > ProductsLds{d}.doubles()) return false;
  }
  return true;
}
static_assert(all_ok(), "factor stage LDS: regions ascending and disjoint, every view inside its area, d = 1 .. 32");
// the fused instances (routes.hpp, with_fused_instance): (M, dmax) = (6, 12) and (2, 4).  A region is at least the item area,
// which is what the walk's LDS leaves of it at copies = 1 (kernels_fused.hpp repeats the check on fused_region_doubles itself).
static_assert(helper_ok(6, 12, fused_region_of(0, 12)) && helper_ok(2, 4, fused_region_of(0, 4)), "fused pass: the helper wave's [Al | mh] inside its region");
}  // namespace factor_lds_check

}  // namespace gvi
