// The arithmetic of input preparation for one (sample, view, joint), shared by prepare_inputs_kernel (inputs.hip) and the heatmap
// decoder (heatmaps.hip), which goes on with it in the thread that found the pixel.  Reference and layout: inputs.hip.
#pragma once
#include "common.hpp"

namespace mpl {

// c: the view's 16 doubles (fx fy cx cy | R row-major | t); (x, y) the pixel; po / ro the item's 3 floats in poses[v] / rays[v];
// co the sample's 3 floats in centers[v], or null in every thread but the one of joint 0.  fp64, every output rounded once.
__device__ __forceinline__ void prepare_point(const double* c, double x, double y, float cf, double w, double h, int norm_in,
                                              int norm_cam, float* po, float* ro, float* co) {
    double fx = c[0], fy = c[1], cx = c[2], cy = c[3];
    if (norm_in) {
        x = (x / w) * 2.0 - 1.0;
        y = (y / w) * 2.0 - h / w;
        if (norm_cam) {
            cx = (cx / w) * 2.0 - 1.0;
            cy = (cy / w) * 2.0 - h / w;
            fx = fx / w * 2.0;
            fy = fy / w * 2.0;
        }
    }
    const double u0 = (x - cx) / fx, u1 = (y - cy) / fy, u2 = 1.0;
    po[0] = (float)x;
    po[1] = (float)y;
    po[2] = cf;
#pragma unroll
    for (int d = 0; d < 3; ++d) ro[d] = (float)(u0 * c[4 + d] + u1 * c[7 + d] + u2 * c[10 + d] + c[13 + d]);   // R^T u + t
    if (co) {
#pragma unroll
        for (int d = 0; d < 3; ++d) co[d] = (float)c[13 + d];
    }
}

}  // namespace mpl
