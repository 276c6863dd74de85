// aoc_passes.inc — kernels and their launch functions, generic over the arithmetic type.
// Included from aoc_kernels.hip once per type, right after aoc_device.h, with AOC_ARITH_NS / AOC_REAL set:
//   aoc64 / double  — the parity path (fp64, states optionally stored as float32)
//   aoc32 / float   — BASELINE config 3 ("fp32 arithmetic everywhere": every array is float32)
// `real` and R(literal) come from aoc_device.h.
namespace AOC_ARITH_NS {

#include "passes/layout.inc"
#include "passes/unit.inc"
#include "passes/cost_rollout.inc"
#include "passes/backward.inc"
#include "passes/forward.inc"
#include "passes/tracking.inc"
#include "passes/hcut.inc"
#include "passes/ltv_lqr.inc"
#include "passes/linesearch.inc"
#include "passes/mpc.inc"

#ifndef AOC_KERNELS_ONLY   // tools/probes/one_kernel.hip compiles single kernels for register / ISA studies
#include "passes/api.inc"
#include "passes/solve.inc"
#endif  // AOC_KERNELS_ONLY
#include "passes/ensemble.inc"   // kernel and launch function in one file (the latter uses make_const of api.inc)
#include "passes/covariance.inc" // likewise (the nominal's record is that of ensemble.inc)
#include "passes/lqg.inc"        // launch function only: k_cov_stage of covariance.inc, then the EST (with limits: EST && LIM) instance of ensemble.inc
#include "passes/filter.inc"     // the filter's gains: k_cov_stage without B K, then a chain kernel of its own
#include "passes/lqgcov.inc"     // the joint (dx, e) prediction of the LQG loop: both k_cov_stage instances, then a chain kernel

}  // namespace AOC_ARITH_NS
