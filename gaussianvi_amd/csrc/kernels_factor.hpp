// Per-factor device kernels of the NGD Gauss-Hermite hot path (gfx950, wave64, fp64): the map of the factor stage.  Nothing is
// defined here; the translation unit includes this file, every other header includes the stage headers it uses.
//
//   kernels_prep.hpp      prep_kernel / prep_all_kernel: Sigma_k -> S_k = Sigma_k^{1/2} (one-wave parallel Jacobi) or its Cholesky
//                         factor (registers or LDS), S_k^{-1}, Lam_k = Sigma_k^{-1} and the per-pass psi operands H_k = A_k S_k, u0_k
//                         [SparseGaussHermite::update_sigmapoints, quadrature/SparseGaussHermite.h:231-243;
//                          update_precision_from_joint, gvibase/GVIFactorizedBase.h:111-114];
//                         jko_*: the factor-level proximal (JKO) map around the Jacobi
//   moments: c_i = w_i psi(mu + S z_i) and the z-space moments  sum_i c_i [1, z_i, z_i z_i^T]
//                         [SparseGaussHermite::Integrate x3, quadrature/SparseGaussHermite.h:197-221;
//                          closures ngd/NGDFactorizedBaseGH.h:46-48], every family on MomArgs (mom_args.hpp):
//   kernels_closed.hpp    closed / box_closed / halfspace_closed: quadrature-free moments of a quadratic psi (NGDFactorizedLinear),
//                         of the separable squared hinge of HINGE_BOX, of the row hinges of HINGE_HALFSPACE
//   kernels_reg.hpp       generic: any d <= 32, any psi kind, host psi.  reg: the policy-templated register kernel with its Psi*
//                         policies, the lane-per-point route of every psi kind that is not a polynomial
//   kernels_split.hpp     split: d = 16 / 20 / 24, four waves per factor, 8-bit coded table
//   kernels_sreg.hpp      sreg / sreg_pair / planar3: sum-of-squares psi, operands from SGPRs, accumulators in registers (dominant);
//                         scost / scost_pair: cost pass (m0 only), several factors per wave
//   kernels_epilogue.hpp  epilogue_kernel / epilogue_all_kernel: ordered sum of the chunk partials, back-transform to x-space,
//                         Vdmu_k / Vddmu_k [calculate_partial_V, ngd/NGDFactorizedBaseGH.h:53-74]; cost_tail_kernel: per-factor cost +
//                         ordered sum + publish for a cost pass, one launch; the tail protocol of the one-launch passes;
//                         expand_kernel: X = mu + S z for the host-callback psi route
//   factor_math.hpp       rcp_nr, rsq_nr, wave_sum
// Beside them: kernels_orbit.hpp / kernels_orbit_psi.hpp (sign-orbit walks), kernels_readout.hpp (read-out-space rule),
// kernels_fused.hpp / kernels_block.hpp (the one-launch passes, built from the bodies above).
//
// Formulation.  With x = mu + S z:  E[(x-mu) psi] = S m1,  E[(x-mu)(x-mu)^T psi] = S M2 S  where
// m1 = sum c_i z_i, M2 = sum c_i z_i z_i^T are accumulated in z-space, so the N x d x d expand GEMM of
// the reference disappears from the per-point work.  Because Lam S = S^{-1}:
//   Vdmu = S^{-1} m1 / T,   Vddmu = (S^{-1} M2 S^{-1} - Lam m0) / T.
// Sum-of-squares psi kinds (quadratic priors) are evaluated as psi = sum_r s_r (u0 + H z)_r^2 with
// H = A S folded per pass, A = diag(sqrt|e|) W^T [Phi, -I] from the eigen-decomposition of Qinv done
// once on the host at gvi_factors_add.
// FactorDev: factor_dev.hpp.  psi of the raw-block kinds at one state (look-ups, *_points walks, psi_point): psi_point.hpp.
#pragma once
#include "factor_math.hpp"
#include "kernels_prep.hpp"
#include "mom_args.hpp"
#include "kernels_closed.hpp"
#include "kernels_reg.hpp"
#include "kernels_split.hpp"
#include "kernels_sreg.hpp"
#include "kernels_epilogue.hpp"
