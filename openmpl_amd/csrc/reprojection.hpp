// What the two refiners by reprojection error share beside views.hpp and takes_part (common.hpp): the Levenberg-Marquardt schedule,
// the status of an item and the launch refusals, each stated once.  refine.hip moves the points and refine_cameras.hip the cameras;
// the projection with its derivative, the cost and the solve stay with each kernel (DESIGN.md section 7 says why).
#pragma once
#include "views.hpp"

namespace mpl {

// (H + lambda diag H) delta = -g: lambda starts at LM_LAMBDA0, is divided by 10 (not below LM_LAMBDA_MIN) after a trial that lowers
// the cost strictly and multiplied by 10 after one that does not.  After every trial, in this order: a step below the tolerance ends
// the loop as converged, then lambda > LM_LAMBDA_MAX or max_iterations trials end it as capped
constexpr double LM_LAMBDA0 = 1e-3, LM_LAMBDA_MIN = 1e-15, LM_LAMBDA_MAX = 1e12;

// the status byte of an item; passed through: too few observations, max_iterations = 0 or (a view) fixed -- scored only
enum { LM_CONVERGED = 0, LM_CAPPED = 1, LM_PASSED_THROUGH = 2, LM_INVALID = 3 };

// what launch_refine_points and launch_refine_cameras refuse alike; out0, out1: the two outputs a call must have
inline int refine_args_check(const float* points, const float* pixels, const double* cams_dev, const void* out0, const void* out1, int B,
                             int V, int J, int max_iterations, double step_tolerance) {
    if (!points || !pixels || !cams_dev || !out0 || !out1 || B <= 0 || V <= 0 || J <= 0) return MPL_E_INVALID;
    if (V > MPL_MAX_VIEWS || J > 64 || (long long)B * V * J > (1ll << 30)) return MPL_E_INVALID;
    if (max_iterations < 0 || max_iterations > 1000 || !(step_tolerance >= 0.0) || !(step_tolerance <= FINITE_MAX))
        return MPL_E_UNSUPPORTED;
    return MPL_OK;
}

}  // namespace mpl
